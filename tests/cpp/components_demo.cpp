// The connected pieces of the model through the C++ SDF_Hashtable facade: two frames of one vertex map at the identity pose
// (as esdf_demo.cpp), then components() with the labels of the given box, then removeComponents() and components() again.
//   components_demo <verts.bin: 640*480 float4> <target> <connectivity> <lo x> <lo y> <lo z> <dims x> <dims y> <dims z>
//                   <min size> <out.bin>
// writes the records (16 bytes each), the labels of the box, then the records after the removal; prints
// "blocks=<n> nodes=<n> components=<n> largest=<n> removed_components=<n> removed_voxels=<n> freed_blocks=<n> after=<n>"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SDF_Hashtable.h"

int main(int argc, char **argv)
{
    if (argc < 12) return 2;
    const size_t n = 640 * 480;
    std::vector<vh_float4> h_verts(n);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(h_verts.data(), sizeof(vh_float4), n, f) != n) return 3;
    std::fclose(f);
    const int target = std::atoi(argv[2]), connectivity = std::atoi(argv[3]);
    int32_t lo[3], dims[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int32_t)std::atoi(argv[4 + a]);
        dims[a] = (int32_t)std::atoi(argv[7 + a]);
    }
    const uint64_t minSize = std::strtoull(argv[10], nullptr, 10);
    vh_float4 *d_verts = nullptr;
    if (hipMalloc((void **)&d_verts, n * sizeof(vh_float4)) != hipSuccess) return 4;
    (void)hipMemcpy(d_verts, h_verts.data(), n * sizeof(vh_float4), hipMemcpyHostToDevice);

    SDF_Hashtable table;                         // common.h defaults, REFERENCE semantics
    float4x4 pose;
    pose.setIdentity();
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    std::vector<vh_component> pieces, plain, after;
    std::vector<uint32_t> labels;
    const vh_component_stats st = table.components(nullptr, target, connectivity, pieces, lo, dims, &labels);
    if (pieces.size() != st.components || labels.size() != (size_t)dims[0] * dims[1] * dims[2]) return 6;
    // without the labels the records are the same
    const vh_component_stats st2 = table.components(nullptr, target, connectivity, plain);
    if (st2.components != st.components || st2.nodes != st.nodes || plain.size() != pieces.size()) return 7;
    for (size_t i = 0; i < pieces.size(); ++i)
        if (plain[i].size != pieces[i].size || plain[i].voxel[0] != pieces[i].voxel[0] || plain[i].voxel[1] != pieces[i].voxel[1] ||
            plain[i].voxel[2] != pieces[i].voxel[2])
            return 7;
    const vh_component_stats rm = table.removeComponents(minSize, nullptr, target, connectivity);
    if (rm.components != st.components || rm.nodes != st.nodes) return 8;
    const vh_component_stats st3 = table.components(nullptr, target, connectivity, after);
    FILE *out = std::fopen(argv[11], "wb");
    if (!out) return 5;
    std::fwrite(pieces.data(), sizeof(vh_component), pieces.size(), out);
    std::fwrite(labels.data(), sizeof(uint32_t), labels.size(), out);
    std::fwrite(after.data(), sizeof(vh_component), after.size(), out);
    std::fclose(out);
    std::printf("blocks=%llu nodes=%llu components=%llu largest=%llu removed_components=%llu removed_voxels=%llu freed_blocks=%llu after=%llu\n",
                (unsigned long long)st.blocks, (unsigned long long)st.nodes, (unsigned long long)st.components,
                (unsigned long long)st.largest, (unsigned long long)rm.removed_components, (unsigned long long)rm.removed_voxels,
                (unsigned long long)rm.freed_blocks, (unsigned long long)st3.components);
    (void)hipFree(d_verts);
    return 0;
}
