// The mesh of the model through the C++ SDF_Hashtable facade: two frames of one vertex map at the identity pose (as
// facade_demo.cpp), then extractMesh() and saveMeshPly().
//   mesh_demo <verts.bin: 640*480 float4> <out.ply>     prints "triangles=<n> floats=<n>"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "SDF_Hashtable.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const size_t n = 640 * 480;
    std::vector<vh_float4> h_verts(n);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(h_verts.data(), sizeof(vh_float4), n, f) != n) return 3;
    std::fclose(f);
    vh_float4 *d_verts = nullptr;
    if (hipMalloc((void **)&d_verts, n * sizeof(vh_float4)) != hipSuccess) return 4;
    (void)hipMemcpy(d_verts, h_verts.data(), n * sizeof(vh_float4), hipMemcpyHostToDevice);

    SDF_Hashtable table;                         // common.h defaults, REFERENCE semantics
    float4x4 pose;
    pose.setIdentity();
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    std::vector<float> positions, normals;
    const uint64_t count = table.extractMesh(positions, &normals);
    if (positions.size() != count * 9 || normals.size() != count * 9) return 5;
    if (table.saveMeshPly(argv[2]) != count) return 6;
    std::printf("triangles=%llu floats=%zu\n", (unsigned long long)count, positions.size());
    (void)hipFree(d_verts);
    return 0;
}
