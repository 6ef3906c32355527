// Merging through the C++ facade: two small models fused from 64x48 uint16 sensor images (src from the first two, dst from the
// third; 2^11 buckets, 4 cm voxels, PINHOLE semantics, pools of 512 and 4096 blocks), then SDF_Hashtable::merge(src, T, mode).
//   merge_demo <frames.bin: 3 * 64*48 uint16> <poses.bin: 3 * 16 floats> <kinv.bin: 9 floats> <transform.bin: 16 floats> <mode>
// prints the stats on one line, then per allocated block of dst "key x y z <checksum>": the sum over the block's 1024 32-bit
// words of word[i] * (2 i + 1), modulo 2^64
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

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int W = 64, H = 48;
    const size_t n = (size_t)W * H;
    std::vector<uint16_t> images(3 * n);
    float poses[3][16], kInv[9], T[16];
    if (!read_all(argv[1], images.data(), images.size() * sizeof(uint16_t)) || !read_all(argv[2], poses, sizeof poses) ||
        !read_all(argv[3], kInv, sizeof kInv) || !read_all(argv[4], T, sizeof T))
        return 3;
    const int mode = std::atoi(argv[5]);
    uint16_t *d_images = nullptr;
    if (hipMalloc((void **)&d_images, images.size() * sizeof(uint16_t)) != hipSuccess) return 4;
    (void)hipMemcpy(d_images, images.data(), images.size() * sizeof(uint16_t), hipMemcpyHostToDevice);

    HashTableParams p;
    vh_default_params(&p);
    p.numBuckets = 1u << 11;
    p.voxelSize = 0.04f;
    p.numVoxelBlocks = 512;
    SDF_Hashtable src(p, W, H, VH_SEM_PINHOLE);
    p.numVoxelBlocks = 4096;
    SDF_Hashtable dst(p, W, H, VH_SEM_PINHOLE);
    src.integrate(float4x4(poses[0]), d_images, kInv);
    src.integrate(float4x4(poses[1]), d_images + n, kInv);
    dst.integrate(float4x4(poses[2]), d_images + 2 * n, kInv);
    vh_merge_stats st;
    dst.merge(src, T, mode, &st);
    std::printf("source_blocks=%u skipped_blocks=%u candidates=%llu allocated=%u blocks=%u unplaced=%llu rounds=%u\n", st.source_blocks,
                st.skipped_blocks, (unsigned long long)st.candidates, st.allocated, st.blocks, (unsigned long long)st.unplaced,
                st.rounds);

    std::vector<VoxelEntry> table((size_t)p.numBuckets * p.bucketSize);
    std::vector<Voxel> voxels((size_t)p.numVoxelBlocks * 512);
    if (vh_download(dst.context(), VH_BUF_HASH_TABLE, table.data(), table.size() * sizeof(VoxelEntry)) != VH_OK ||
        vh_download(dst.context(), VH_BUF_SDF_BLOCKS, voxels.data(), voxels.size() * sizeof(Voxel)) != VH_OK)
        return 5;
    for (const VoxelEntry &e : table) {
        if (e.ptr == VH_FREE_BLOCK) continue;
        const uint32_t *words = reinterpret_cast<const uint32_t *>(voxels.data() + e.ptr);
        unsigned long long sum = 0;
        for (unsigned i = 0; i < 1024; ++i) sum += (unsigned long long)words[i] * (2ull * i + 1ull);
        std::printf("key %d %d %d %llu\n", e.pos[0], e.pos[1], e.pos[2], sum);
    }
    (void)hipFree(d_images);
    return 0;
}
