// Incremental meshing through the C++ facade: a model fused from the first of three 64x48 uint16 sensor images (2^11 buckets,
// 4 cm voxels, 512 blocks, PINHOLE semantics), SDF_Hashtable::changedBlocks against an empty state and extractMeshBlocks of what
// it lists; then the second image, and the same two calls again.
//   mesh_blocks_demo <frames.bin: 3 * 64*48 uint16> <poses.bin: 3 * 16 floats> <kinv.bin: 9 floats>
// prints per round "round <r> changed=<n> removed=<n> triangles=<n>", then per listed block "key x y z <flags> <triangles>
// <checksum>": the sum over the words of its positions and normals of word[i] * (2 i + 1), modulo 2^64
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
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

static unsigned long long checksum(const float *a, const float *b, size_t n)
{
    unsigned long long sum = 0, i = 0;
    for (const float *p : {a, b})
        for (size_t k = 0; k < n; ++k, ++i) {
            uint32_t w;
            std::memcpy(&w, p + k, sizeof w);
            sum += (unsigned long long)w * (2ull * i + 1ull);
        }
    return sum;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
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
    void *d_state = nullptr;
    const uint64_t bytes = table.changesStateBytes();
    if (bytes != 64 + 32ull * p.numVoxelBlocks || hipMalloc(&d_state, bytes) != hipSuccess) return 4;
    (void)hipMemset(d_state, 0, bytes);

    for (int round = 0; round < 2; ++round) {
        table.integrate(float4x4(poses[round]), d_images + round * n, kInv);
        std::vector<int32_t> changed, removed;
        std::vector<float> positions, normals;
        std::vector<uint64_t> first;
        const uint64_t listed = table.changedBlocks(d_state, changed, removed, nullptr, VH_CHANGES_VOXELS, VH_CHANGES_HALO_NORMALS);
        const uint64_t triangles = table.extractMeshBlocks(changed, positions, first, &normals);
        if (changed.size() != listed * 4 || first.size() != listed + 1 || first[listed] != triangles) return 5;
        std::printf("round %d changed=%llu removed=%zu triangles=%llu\n", round, (unsigned long long)listed, removed.size() / 4,
                    (unsigned long long)triangles);
        for (uint64_t j = 0; j < listed; ++j) {
            const size_t a = (size_t)first[j] * 9, len = (size_t)(first[j + 1] - first[j]) * 9;
            std::printf("key %d %d %d %d %llu %llu\n", changed[4 * j], changed[4 * j + 1], changed[4 * j + 2], changed[4 * j + 3],
                        (unsigned long long)(first[j + 1] - first[j]), checksum(positions.data() + a, normals.data() + a, len));
        }
    }
    // nothing happened since: nothing is listed
    std::vector<int32_t> changed, removed;
    if (table.changedBlocks(d_state, changed, removed) != 0 || !removed.empty()) return 6;
    (void)hipFree(d_state);
    (void)hipFree(d_images);
    return 0;
}
