// Block streaming through the C++ facade: a model fused from the first two of three 64x48 uint16 sensor images (2^11 buckets,
// 4 cm voxels, 512 blocks, PINHOLE semantics), SDF_Hashtable::streamOut of everything outside a sphere, then streamIn of what
// came out.
//   stream_demo <frames.bin: 3 * 64*48 uint16> <poses.bin: 3 * 16 floats> <kinv.bin: 9 floats> <cx> <cy> <cz> <radius>
// prints "moved=<n> left=<blocks still in the model>", per record "out x y z <checksum>", the stats of the stream-in on one
// line, then per allocated block of the model "key x y z <checksum>": the sum over the block's 1024 32-bit words of
// word[i] * (2 i + 1), modulo 2^64
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SDF_Hashtable.h"

static bool read_all(const char *path, void *dst, size_t bytes)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(dst, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static unsigned long long checksum(const Voxel *voxels)
{
    const uint32_t *words = reinterpret_cast<const uint32_t *>(voxels);
    unsigned long long sum = 0;
    for (unsigned i = 0; i < 1024; ++i) sum += (unsigned long long)words[i] * (2ull * i + 1ull);
    return sum;
}

int main(int argc, char **argv)
{
    if (argc < 8) return 2;
    const int W = 64, H = 48;
    const size_t n = (size_t)W * H;
    std::vector<uint16_t> images(3 * n);
    float poses[3][16], kInv[9];
    if (!read_all(argv[1], images.data(), images.size() * sizeof(uint16_t)) || !read_all(argv[2], poses, sizeof poses) ||
        !read_all(argv[3], kInv, sizeof kInv))
        return 3;
    uint16_t *d_images = nullptr;
    if (hipMalloc((void **)&d_images, images.size() * sizeof(uint16_t)) != hipSuccess) return 4;
    (void)hipMemcpy(d_images, images.data(), images.size() * sizeof(uint16_t), hipMemcpyHostToDevice);

    HashTableParams p;
    vh_default_params(&p);
    p.numBuckets = 1u << 11;
    p.voxelSize = 0.04f;
    p.numVoxelBlocks = 512;
    SDF_Hashtable table(p, W, H, VH_SEM_PINHOLE);
    table.integrate(float4x4(poses[0]), d_images, kInv);
    table.integrate(float4x4(poses[1]), d_images + n, kInv);

    vh_stream_region region{};
    region.kind = VH_STREAM_SPHERE;
    region.invert = 1;
    for (int a = 0; a < 3; ++a) region.centre[a] = (float)std::atof(argv[4 + a]);
    region.radius = (float)std::atof(argv[7]);
    std::vector<vh_view_record> records;
    const uint64_t moved = table.streamOut(region, records);

    std::vector<VoxelEntry> entries((size_t)p.numBuckets * p.bucketSize);
    std::vector<Voxel> voxels((size_t)p.numVoxelBlocks * 512);
    if (vh_download(table.context(), VH_BUF_HASH_TABLE, entries.data(), entries.size() * sizeof(VoxelEntry)) != VH_OK) return 5;
    unsigned left = 0;
    for (const VoxelEntry &e : entries) left += e.ptr != VH_FREE_BLOCK;
    std::printf("moved=%llu left=%u\n", (unsigned long long)moved, left);
    for (const vh_view_record &r : records) std::printf("out %d %d %d %llu\n", r.pos[0], r.pos[1], r.pos[2], checksum(r.voxels));

    vh_stream_stats st;
    std::vector<int32_t> status;
    table.streamIn(records, nullptr, &status, &st);
    unsigned placed = 0;
    for (int32_t s : status) placed += s == VH_STREAM_PLACED;
    std::printf("placed=%llu present=%llu unplaced=%llu foreign=%llu rounds=%u status_placed=%u\n", (unsigned long long)st.placed,
                (unsigned long long)st.present, (unsigned long long)st.unplaced, (unsigned long long)st.foreign, st.rounds, placed);
    if (vh_download(table.context(), VH_BUF_HASH_TABLE, entries.data(), entries.size() * sizeof(VoxelEntry)) != VH_OK ||
        vh_download(table.context(), VH_BUF_SDF_BLOCKS, voxels.data(), voxels.size() * sizeof(Voxel)) != VH_OK)
        return 5;
    for (const VoxelEntry &e : entries) {
        if (e.ptr == VH_FREE_BLOCK) continue;
        std::printf("key %d %d %d %llu\n", e.pos[0], e.pos[1], e.pos[2], checksum(voxels.data() + e.ptr));
    }
    (void)hipFree(d_images);
    return 0;
}
