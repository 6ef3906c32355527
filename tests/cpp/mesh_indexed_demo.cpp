// The indexed mesh of the model through the C++ SDF_Hashtable facade: two frames of one vertex map at the identity pose (as
// mesh_demo.cpp), then extractMeshIndexed() and saveMeshPlyIndexed().
//   mesh_indexed_demo <verts.bin: 640*480 float4> <out.ply>     prints "triangles=<n> vertices=<n>"
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
    std::vector<float> vertices, normals;
    std::vector<uint32_t> indices;
    const uint64_t count = table.extractMeshIndexed(vertices, indices, &normals);
    if (indices.size() != count * 3 || normals.size() != vertices.size()) return 5;
    for (uint32_t i : indices)
        if ((size_t)i * 3 >= vertices.size()) return 6;
    if (table.saveMeshPlyIndexed(argv[2]) != count) return 7;
    std::printf("triangles=%llu vertices=%zu\n", (unsigned long long)count, vertices.size() / 3);
    (void)hipFree(d_verts);
    return 0;
}
