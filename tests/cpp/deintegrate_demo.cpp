// A frame in and out again through the C++ SDF_Hashtable facade: one vertex map at a pose into an empty table,
// deintegrate() at the same pose, garbageCollect(0).
//   deintegrate_demo <verts.bin: 640*480 float4>
// prints "fused=<voxels with weight > 0 after the frame> left=<the same after taking it out> blocks=<entries still allocated>";
// left and blocks must be 0
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "SDF_Hashtable.h"

static size_t weighted(SDF_Hashtable &table, std::vector<Voxel> &vox)
{
    if (vh_download(table.context(), VH_BUF_SDF_BLOCKS, vox.data(), vox.size() * sizeof(Voxel)) != VH_OK) return (size_t)-1;
    size_t n = 0;
    for (const Voxel &v : vox) n += v.weight > 0.0f;
    return n;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
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
    pose(0, 3) = 0.1f;
    std::vector<Voxel> vox((size_t)table.params().numVoxelBlocks * 512);
    table.integrate(pose, d_verts, (const vh_float4 *)nullptr);
    const size_t fused = weighted(table, vox);
    table.deintegrate(pose, d_verts);
    const size_t left = weighted(table, vox);
    table.garbageCollect(0.0f);                  // the pairing: frees the blocks the removal emptied
    std::vector<VoxelEntry> entries((size_t)table.params().numBuckets * table.params().bucketSize);
    if (vh_download(table.context(), VH_BUF_HASH_TABLE, entries.data(), entries.size() * sizeof(VoxelEntry)) != VH_OK) return 5;
    size_t blocks = 0;
    for (const VoxelEntry &e : entries) blocks += e.ptr != VH_FREE_BLOCK;
    std::printf("fused=%zu left=%zu blocks=%zu\n", fused, left, blocks);
    (void)hipFree(d_verts);
    return 0;
}
