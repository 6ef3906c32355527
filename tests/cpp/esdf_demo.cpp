// The Euclidean distance to the surface through the C++ SDF_Hashtable facade: two frames of one vertex map at the identity pose
// (as sample_demo.cpp), then esdfLattice() over the given box.
//   esdf_demo <verts.bin: 640*480 float4> <lo x> <lo y> <lo z> <dims x> <dims y> <dims z> <radius> <unknown> <out.bin>
// writes the int32 squared distances, then the float metres; prints "voxels=<n> none=<k> far=<k> near=<k>"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SDF_Hashtable.h"

int main(int argc, char **argv)
{
    if (argc < 11) return 2;
    const size_t n = 640 * 480;
    std::vector<vh_float4> h_verts(n);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(h_verts.data(), sizeof(vh_float4), n, f) != n) return 3;
    std::fclose(f);
    int32_t lo[3], dims[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int32_t)std::atoi(argv[2 + a]);
        dims[a] = (int32_t)std::atoi(argv[5 + a]);
    }
    const int radius = std::atoi(argv[8]), unknown = std::atoi(argv[9]);
    vh_float4 *d_verts = nullptr;
    if (hipMalloc((void **)&d_verts, n * sizeof(vh_float4)) != hipSuccess) return 4;
    (void)hipMemcpy(d_verts, h_verts.data(), n * sizeof(vh_float4), hipMemcpyHostToDevice);

    SDF_Hashtable table;                         // common.h defaults, REFERENCE semantics
    float4x4 pose;
    pose.setIdentity();
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    std::vector<int32_t> dist2;
    std::vector<float> distance;
    table.esdfLattice(lo, dims, radius, unknown, &dist2, &distance);
    if (dist2.size() != (size_t)dims[0] * dims[1] * dims[2] || distance.size() != dist2.size()) return 6;
    // each output alone gives the same
    std::vector<int32_t> only2;
    std::vector<float> onlyF;
    table.esdfLattice(lo, dims, radius, unknown, &only2, nullptr);
    table.esdfLattice(lo, dims, radius, unknown, nullptr, &onlyF);
    if (only2 != dist2 || onlyF.size() != distance.size()) return 7;
    size_t none = 0, far = 0, near = 0;
    for (size_t i = 0; i < dist2.size(); ++i) {
        const int32_t d = dist2[i];
        none += d == VH_ESDF_NONE;
        far += d == VH_ESDF_FAR || d == -VH_ESDF_FAR;
        near += d != VH_ESDF_NONE && d != VH_ESDF_FAR && d != -VH_ESDF_FAR;
        if (!(onlyF[i] == distance[i] || (onlyF[i] != onlyF[i] && distance[i] != distance[i]))) return 7;
    }
    FILE *out = std::fopen(argv[10], "wb");
    if (!out) return 5;
    std::fwrite(dist2.data(), sizeof(int32_t), dist2.size(), out);
    std::fwrite(distance.data(), sizeof(float), distance.size(), out);
    std::fclose(out);
    std::printf("voxels=%zu none=%zu far=%zu near=%zu\n", dist2.size(), none, far, near);
    (void)hipFree(d_verts);
    return 0;
}
