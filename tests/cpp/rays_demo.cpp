// Rays against the model through the C++ SDF_Hashtable facade: two frames of one vertex map at the identity pose (as
// sample_demo.cpp), then castRays() on the given rays, once along each ray and once with the given shared plane.
//   rays_demo <verts.bin: 640*480 float4> <rays.bin: n*8 floats, then 4 floats: the plane> <out.bin>
// writes, per pass (along each ray, shared plane), n t, 3n normal floats and 4n voxel int32; prints "rays=<n> hits0=<k> hits1=<k>"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "SDF_Hashtable.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const size_t n = 640 * 480;
    std::vector<vh_float4> h_verts(n);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(h_verts.data(), sizeof(vh_float4), n, f) != n) return 3;
    std::fclose(f);
    std::vector<float> rays;
    f = std::fopen(argv[2], "rb");
    if (!f) return 3;
    float word;
    while (std::fread(&word, sizeof(float), 1, f) == 1) rays.push_back(word);
    std::fclose(f);
    if (rays.size() < 4 || (rays.size() - 4) % 8 != 0) return 3;
    const float plane[4] = {rays[rays.size() - 4], rays[rays.size() - 3], rays[rays.size() - 2], rays[rays.size() - 1]};
    rays.resize(rays.size() - 4);
    vh_float4 *d_verts = nullptr;
    if (hipMalloc((void **)&d_verts, n * sizeof(vh_float4)) != hipSuccess) return 4;
    (void)hipMemcpy(d_verts, h_verts.data(), n * sizeof(vh_float4), hipMemcpyHostToDevice);

    SDF_Hashtable table;                         // common.h defaults, REFERENCE semantics
    float4x4 pose;
    pose.setIdentity();
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 5;
    size_t hits[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<float> t, normals;
        std::vector<int32_t> voxels;
        table.castRays(rays, pass ? plane : nullptr, t, &normals, &voxels);
        if (t.size() != rays.size() / 8 || normals.size() != 3 * t.size() || voxels.size() != 4 * t.size()) return 6;
        for (size_t i = 0; i < t.size(); ++i) hits[pass] += voxels[4 * i + 3] == 1;
        std::fwrite(t.data(), sizeof(float), t.size(), out);
        std::fwrite(normals.data(), sizeof(float), normals.size(), out);
        std::fwrite(voxels.data(), sizeof(int32_t), voxels.size(), out);
    }
    std::fclose(out);
    std::printf("rays=%zu hits0=%zu hits1=%zu\n", rays.size() / 8, hits[0], hits[1]);
    (void)hipFree(d_verts);
    return 0;
}
