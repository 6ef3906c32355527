// Colour through merging, de-integration and a saved file, by the C++ facade: two small coloured models fused from 64x48 RGB-D
// frames (src from the first two, dst from the third; 2^11 buckets, 4 cm voxels, PINHOLE semantics, pools of 512 and 4096 blocks).
// src's second frame is moved to the first pose with reintegrateDepthColor(), then dst.mergeColor(src, T, mode, weight max),
// saveColor(), deintegrateDepthColor() of dst's own frame, and loadColor() of the file saved before it.
//   merge_color_demo <frames.bin: 3 * 64*48 uint16> <colors.bin: 3 * 64*48 uint32> <poses.bin: 3 * 16 floats> <kinv.bin: 9 floats>
//                    <transform.bin: 16 floats> <mode> <band> <weight max> <colour file to write>
// prints the merge stats on one line, then per allocated block of dst "key x y z <voxels> <colour> <loaded>": the checksum of
// the block's 1024 voxel words and of its 512 colour words after the de-integration, and of the colour words after the load;
// a checksum is the sum of word[i] * (2 i + 1), modulo 2^64
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

static unsigned long long checksum(const uint32_t *words, unsigned n)
{
    unsigned long long sum = 0;
    for (unsigned i = 0; i < n; ++i) sum += (unsigned long long)words[i] * (2ull * i + 1ull);
    return sum;
}

int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const int W = 64, H = 48;
    const size_t n = (size_t)W * H;
    std::vector<uint16_t> images(3 * n);
    std::vector<uint32_t> colors(3 * n);
    float poses[3][16], kInv[9], T[16];
    if (!read_all(argv[1], images.data(), images.size() * sizeof(uint16_t)) ||
        !read_all(argv[2], colors.data(), colors.size() * sizeof(uint32_t)) || !read_all(argv[3], poses, sizeof poses) ||
        !read_all(argv[4], kInv, sizeof kInv) || !read_all(argv[5], T, sizeof T))
        return 3;
    const int mode = std::atoi(argv[6]);
    const float band = (float)std::atof(argv[7]);
    const int weightMax = std::atoi(argv[8]);
    const char *colorFile = argv[9];
    uint16_t *d_images = nullptr;
    uint32_t *d_colors = nullptr;
    if (hipMalloc((void **)&d_images, images.size() * sizeof(uint16_t)) != hipSuccess ||
        hipMalloc((void **)&d_colors, colors.size() * sizeof(uint32_t)) != hipSuccess)
        return 4;
    (void)hipMemcpy(d_images, images.data(), images.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    (void)hipMemcpy(d_colors, colors.data(), colors.size() * sizeof(uint32_t), hipMemcpyHostToDevice);

    HashTableParams p;
    vh_default_params(&p);
    p.numBuckets = 1u << 11;
    p.voxelSize = 0.04f;
    p.numVoxelBlocks = 512;
    SDF_Hashtable src(p, W, H, VH_SEM_PINHOLE);
    p.numVoxelBlocks = 4096;
    SDF_Hashtable dst(p, W, H, VH_SEM_PINHOLE);
    for (int i = 0; i < 2; ++i)
        src.integrateColor(float4x4(poses[i]), d_images + i * n, kInv, d_colors + i * n, band, 255, true);
    dst.integrateColor(float4x4(poses[2]), d_images + 2 * n, kInv, d_colors + 2 * n, band, 255, true);
    src.reintegrateDepthColor(float4x4(poses[1]), float4x4(poses[0]), d_images + n, kInv, d_colors + n, band, 255);
    vh_merge_stats st;
    dst.mergeColor(src, T, mode, weightMax, &st);
    std::printf("source_blocks=%u skipped_blocks=%u candidates=%llu allocated=%u blocks=%u unplaced=%llu rounds=%u\n", st.source_blocks,
                st.skipped_blocks, (unsigned long long)st.candidates, st.allocated, st.blocks, (unsigned long long)st.unplaced,
                st.rounds);
    dst.saveColor(colorFile);
    dst.deintegrateDepthColor(float4x4(poses[2]), d_images + 2 * n, kInv, d_colors + 2 * n, band);

    std::vector<VoxelEntry> table((size_t)p.numBuckets * p.bucketSize);
    std::vector<Voxel> voxels((size_t)p.numVoxelBlocks * 512);
    std::vector<uint32_t> words(voxels.size()), loaded(voxels.size());
    if (vh_download(dst.context(), VH_BUF_HASH_TABLE, table.data(), table.size() * sizeof(VoxelEntry)) != VH_OK ||
        vh_download(dst.context(), VH_BUF_SDF_BLOCKS, voxels.data(), voxels.size() * sizeof(Voxel)) != VH_OK ||
        vh_download_color(dst.context(), 0, words.data(), words.size()) != VH_OK)
        return 5;
    dst.loadColor(colorFile);
    if (vh_download_color(dst.context(), 0, loaded.data(), loaded.size()) != VH_OK) return 5;
    for (const VoxelEntry &e : table) {
        if (e.ptr == VH_FREE_BLOCK) continue;
        std::printf("key %d %d %d %llu %llu %llu\n", e.pos[0], e.pos[1], e.pos[2],
                    checksum(reinterpret_cast<const uint32_t *>(voxels.data() + e.ptr), 1024), checksum(words.data() + e.ptr, 512),
                    checksum(loaded.data() + e.ptr, 512));
    }
    (void)hipFree(d_images);
    (void)hipFree(d_colors);
    return 0;
}
