// Tracking against the model's colour and shape through the C++ facade: a model fused from n 160x120 RGB-D frames (uint16
// sensor images with their registered colour images; 2^16 buckets, 2^14 blocks, truncation 0.06, PINHOLE semantics) with
// integrateColor(), then CameraTracking::AlignToModelColor of one more frame from the given start pose.
//   sdf_color_track_demo <n> <frames.bin: (n + 1) * 160*120 uint16> <colors.bin: (n + 1) * 160*120 uint32>
//                        <poses.bin: n * 16 floats> <kinv.bin: 9 floats> <start.bin: 16 floats> <band> <out.bin>
// writes the 16 floats of the aligned pose; prints "steps=<k> error=<summed residual>"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "CameraTracking.h"

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
    if (argc < 9) return 2;
    const int W = 160, H = 120;
    const size_t n = (size_t)W * H;
    const int frames = std::atoi(argv[1]);
    if (frames < 1 || frames > 16) return 2;
    std::vector<uint16_t> images((frames + 1) * n);
    std::vector<uint32_t> colors((frames + 1) * n);
    std::vector<float> poses((size_t)frames * 16);
    float kInv[9];
    float4x4 pose;
    if (!read_all(argv[2], images.data(), images.size() * sizeof(uint16_t)) ||
        !read_all(argv[3], colors.data(), colors.size() * sizeof(uint32_t)) ||
        !read_all(argv[4], poses.data(), poses.size() * sizeof(float)) || !read_all(argv[5], kInv, sizeof kInv) ||
        !read_all(argv[6], pose.entries, sizeof(float) * 16))
        return 3;
    const float band = (float)std::atof(argv[7]);
    uint16_t *d_images = nullptr;
    uint32_t *d_colors = nullptr;
    vh_float4 *d_verts = nullptr, *d_normals = nullptr;
    if (hipMalloc((void **)&d_images, images.size() * sizeof(uint16_t)) != hipSuccess ||
        hipMalloc((void **)&d_colors, colors.size() * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&d_verts, n * sizeof(vh_float4)) != hipSuccess ||
        hipMalloc((void **)&d_normals, n * sizeof(vh_float4)) != hipSuccess)
        return 4;
    (void)hipMemcpy(d_images, images.data(), images.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    (void)hipMemcpy(d_colors, colors.data(), colors.size() * sizeof(uint32_t), hipMemcpyHostToDevice);

    HashTableParams p;
    vh_default_params(&p);
    p.numBuckets = 1u << 16;
    p.numVoxelBlocks = 1u << 14;
    p.truncation = 0.06f;
    SDF_Hashtable table(p, W, H, VH_SEM_PINHOLE);
    for (int i = 0; i < frames; ++i)
        table.integrateColor(float4x4(poses.data() + 16 * i), d_images + i * n, kInv, d_colors + i * n, band, 255, true);
    if (vh_preprocess(d_images + frames * n, kInv, W, H, d_verts, d_normals, nullptr) != VH_OK) return 5;
    CameraTracking tracker(W, H);
    const int steps = tracker.AlignToModelColor(table, d_verts, d_colors + frames * n, pose);
    FILE *out = std::fopen(argv[8], "wb");
    if (!out) return 5;
    std::fwrite(pose.entries, sizeof(float), 16, out);
    std::fclose(out);
    std::printf("steps=%d error=%.9g\n", steps, (double)tracker.lastError());
    (void)hipFree(d_images);
    (void)hipFree(d_colors);
    (void)hipFree(d_verts);
    (void)hipFree(d_normals);
    return 0;
}
