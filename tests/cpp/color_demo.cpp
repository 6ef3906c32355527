// Colour through the C++ SDF_Hashtable facade: a small model fused from three 64x48 RGB-D frames (uint16 sensor images with their
// registered colour images; 2^11 buckets, 4 cm voxels, 512 blocks, PINHOLE semantics) with integrateColor(), then sampleColor()
// at the given points in both modes.
//   color_demo <frames.bin: 3 * 64*48 uint16> <colors.bin: 3 * 64*48 uint32> <poses.bin: 3 * 16 floats> <kinv.bin: 9 floats>
//              <points.bin: n*3 floats> <band> <weight max>
// prints "points=<n> colours0=<k> colours1=<k>", then per mode (nearest, trilinear) one line of n words in hex, then per allocated
// block "key x y z <checksum>": the sum over the block's 512 colour words of word[i] * (2 i + 1), modulo 2^64
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
    if (argc < 8) return 2;
    const int W = 64, H = 48;
    const size_t n = (size_t)W * H;
    std::vector<uint16_t> images(3 * n);
    std::vector<uint32_t> colors(3 * n);
    float poses[3][16], kInv[9];
    if (!read_all(argv[1], images.data(), images.size() * sizeof(uint16_t)) ||
        !read_all(argv[2], colors.data(), colors.size() * sizeof(uint32_t)) || !read_all(argv[3], poses, sizeof poses) ||
        !read_all(argv[4], kInv, sizeof kInv))
        return 3;
    std::vector<float> points;
    FILE *f = std::fopen(argv[5], "rb");
    if (!f) return 3;
    float xyz[3];
    while (std::fread(xyz, sizeof(float), 3, f) == 3) points.insert(points.end(), xyz, xyz + 3);
    std::fclose(f);
    const float band = (float)std::atof(argv[6]);
    const int weightMax = std::atoi(argv[7]);
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
    SDF_Hashtable table(p, W, H, VH_SEM_PINHOLE);
    // frame 0 as depth then colour, frames 1 and 2 as one RGB-D call each
    table.integrate(float4x4(poses[0]), d_images, kInv);
    table.integrateColor(float4x4(poses[0]), d_images, kInv, d_colors, band, weightMax);
    for (int i = 1; i < 3; ++i)
        table.integrateColor(float4x4(poses[i]), d_images + i * n, kInv, d_colors + i * n, band, weightMax, true);

    std::vector<uint32_t> rgba[2];
    size_t have[2] = {0, 0};
    const int modes[2] = {VH_SAMPLE_NEAREST, VH_SAMPLE_TRILINEAR};
    for (int m = 0; m < 2; ++m) {
        table.sampleColor(points, modes[m], rgba[m]);
        if (rgba[m].size() != points.size() / 3) return 6;
        for (uint32_t c : rgba[m]) have[m] += c != 0u;
    }
    std::printf("points=%zu colours0=%zu colours1=%zu\n", points.size() / 3, have[0], have[1]);
    for (int m = 0; m < 2; ++m) {
        for (uint32_t c : rgba[m]) std::printf("%08x ", c);
        std::printf("\n");
    }
    std::vector<VoxelEntry> entries((size_t)p.numBuckets * p.bucketSize);
    std::vector<uint32_t> words((size_t)p.numVoxelBlocks * 512);
    if (!vh_has_color(table.context()) ||
        vh_download(table.context(), VH_BUF_HASH_TABLE, entries.data(), entries.size() * sizeof(VoxelEntry)) != VH_OK ||
        vh_download_color(table.context(), 0, words.data(), words.size()) != VH_OK)
        return 5;
    for (const VoxelEntry &e : entries) {
        if (e.ptr == VH_FREE_BLOCK) continue;
        unsigned long long sum = 0;
        for (unsigned i = 0; i < 512; ++i) sum += (unsigned long long)words[(size_t)e.ptr + i] * (2ull * i + 1ull);
        std::printf("key %d %d %d %llu\n", e.pos[0], e.pos[1], e.pos[2], sum);
    }
    (void)hipFree(d_images);
    (void)hipFree(d_colors);
    return 0;
}
