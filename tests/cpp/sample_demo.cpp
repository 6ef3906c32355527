// The model as a distance field through the C++ SDF_Hashtable facade: two frames of one vertex map at the identity pose (as
// mesh_demo.cpp), then sampleSdf() at the given points in both modes.
//   sample_demo <verts.bin: 640*480 float4> <points.bin: n*3 floats> <out.bin>
// writes, per mode (nearest, trilinear), n sdf, n weights and 3n gradient floats; prints "points=<n> samples0=<k> samples1=<k>"
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
    std::vector<float> points;
    f = std::fopen(argv[2], "rb");
    if (!f) return 3;
    float xyz[3];
    while (std::fread(xyz, sizeof(float), 3, f) == 3) points.insert(points.end(), xyz, xyz + 3);
    std::fclose(f);
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
    size_t samples[2] = {0, 0};
    const int modes[2] = {VH_SAMPLE_NEAREST, VH_SAMPLE_TRILINEAR};
    for (int m = 0; m < 2; ++m) {
        std::vector<float> sdf, weight, gradient;
        table.sampleSdf(points, modes[m], sdf, &weight, &gradient);
        if (sdf.size() != points.size() / 3 || weight.size() != sdf.size() || gradient.size() != points.size()) return 6;
        for (float s : sdf) samples[m] += s == s;
        std::fwrite(sdf.data(), sizeof(float), sdf.size(), out);
        std::fwrite(weight.data(), sizeof(float), weight.size(), out);
        std::fwrite(gradient.data(), sizeof(float), gradient.size(), out);
    }
    std::fclose(out);
    std::printf("points=%zu samples0=%zu samples1=%zu\n", points.size() / 3, samples[0], samples[1]);
    (void)hipFree(d_verts);
    return 0;
}
