// vh_api_mesh.hip -- C-ABI, the way out of the volume: vh_extract_mesh (kernels: vh_mesh.hip).
// Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, flush_pending()).

// Scratch of the extraction, allocated at the first call and kept (grown when a view context imports more records): the block
// list, the slice and block counts, the scans' tile totals and two result words.  All or nothing: a failed allocation leaves
// the context as it was.
static int mesh_reserve(vh_context *c, size_t slices, size_t blocks)
{
    const size_t counts = slices + blocks;
    const size_t totals = (slices + kMeshScanTile - 1) / kMeshScanTile + (blocks + kMeshScanTile - 1) / kMeshScanTile + 2;
    if (c->meshItems.size() >= blocks && c->meshCounts.size() >= counts && c->meshTotals.size() >= totals) return VH_OK;
    VH_HIP(hipStreamSynchronize(c->stream));           // (before an older, smaller set is freed)
    DevBuf<int4> items;
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> tot;
    int rc;
    if ((rc = items.alloc(blocks, "mesh block list")) || (rc = cnt.alloc(counts, "mesh counts")) ||
        (rc = tot.alloc(totals, "mesh scan totals")))
        return rc;
    c->meshItems = std::move(items);
    c->meshCounts = std::move(cnt);
    c->meshTotals = std::move(tot);
    return VH_OK;
}

template <bool kApron>
static void mesh_launch_blocks(vh_context *c, const FrameParams &fp, const DevPtrs &dp, unsigned grid, const unsigned long long *numItems,
                               uint32_t listCapacity, uint32_t *blockCount, const unsigned long long *tileBase, bool emit,
                               unsigned long long capacity, float *positions, float *normals)
{
    const int4 *items = c->meshItems;
    if (!emit)
        hipLaunchKernelGGL((mesh_block_kernel<kApron, false, false>), dim3(grid), dim3(256), 0, c->stream, fp, dp, items, numItems,
                           listCapacity, blockCount, tileBase, 0ull, (float *)nullptr, (float *)nullptr);
    else if (normals)
        hipLaunchKernelGGL((mesh_block_kernel<kApron, true, true>), dim3(grid), dim3(256), 0, c->stream, fp, dp, items, numItems,
                           listCapacity, blockCount, tileBase, capacity, positions, normals);
    else
        hipLaunchKernelGGL((mesh_block_kernel<kApron, true, false>), dim3(grid), dim3(256), 0, c->stream, fp, dp, items, numItems,
                           listCapacity, blockCount, tileBase, capacity, positions, normals);
}

extern "C" int vh_extract_mesh(vh_context *c, const vh_mesh_region *region, uint64_t capacity_triangles, float *d_positions,
                               float *d_normals, uint64_t *triangles_out)
{
    VH_TRACE("vh_extract_mesh");
    if (!c || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity_triangles > 0 && !d_positions) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a position buffer");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // the frames queued so far are part of the model

    MeshRegion rg;
    for (int a = 0; a < 3; ++a) {
        rg.lo[a] = region ? region->block_lo[a] : INT32_MIN;
        rg.hi[a] = region ? region->block_hi[a] : INT32_MAX;
    }
    const size_t slices = ((size_t)c->ownedBuckets + kMeshSliceBuckets - 1) / kMeshSliceBuckets;
    // a table holds at most numVoxelBlocks blocks, a view table one per imported record
    const size_t blocks = std::max<size_t>(1, std::min<size_t>(c->numEntries, c->viewBlocks ? (size_t)c->viewCount : (size_t)c->params.numVoxelBlocks));
    { const int rc = mesh_reserve(c, slices, blocks); if (rc != VH_OK) return rc; }
    const uint32_t listCapacity = (uint32_t)c->meshItems.size();
    uint32_t *sliceCount = c->meshCounts, *blockCount = sliceCount + slices;
    unsigned long long *sliceTiles = c->meshTotals;
    unsigned long long *blockTiles = sliceTiles + (slices + kMeshScanTile - 1) / kMeshScanTile;
    unsigned long long *result = blockTiles + (c->meshItems.size() + kMeshScanTile - 1) / kMeshScanTile;   // {listed blocks, triangles}

    FrameParams fp = c->fp;
    DevPtrs dp = c->dp;
    if (c->viewBlocks) dp.blocks = const_cast<Voxel *>(c->viewBlocks);     // view table: voxels live in the records
    hipStream_t s = c->stream;
    const unsigned listGrid = (unsigned)grid_for(slices, 4), sliceTileGrid = (unsigned)grid_for(slices, kMeshScanTile);
    hipLaunchKernelGGL(mesh_list_kernel<false>, dim3(listGrid), dim3(256), 0, s, fp, dp, rg, c->ownedBuckets, (uint32_t)slices,
                       sliceCount, (const unsigned long long *)sliceTiles, (int4 *)c->meshItems, listCapacity);
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(sliceTileGrid), dim3(256), 0, s, sliceCount, (const unsigned long long *)nullptr,
                       (uint32_t)slices, sliceTiles);
    hipLaunchKernelGGL(mesh_scan_totals_kernel, dim3(1), dim3(256), 0, s, sliceTiles, (const unsigned long long *)nullptr,
                       (uint32_t)slices, (unsigned long long)listCapacity, result);
    hipLaunchKernelGGL(mesh_list_kernel<true>, dim3(listGrid), dim3(256), 0, s, fp, dp, rg, c->ownedBuckets, (uint32_t)slices,
                       sliceCount, (const unsigned long long *)sliceTiles, (int4 *)c->meshItems, listCapacity);

    const unsigned blockGrid = (unsigned)std::min<size_t>(c->meshItems.size(), 8192);
    const unsigned blockTileGrid = (unsigned)grid_for(c->meshItems.size(), kMeshScanTile);
    const bool apron = c->meshVariant == 0;
    if (apron) mesh_launch_blocks<true>(c, fp, dp, blockGrid, result, listCapacity, blockCount, blockTiles, false, 0, nullptr, nullptr);
    else mesh_launch_blocks<false>(c, fp, dp, blockGrid, result, listCapacity, blockCount, blockTiles, false, 0, nullptr, nullptr);
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(blockTileGrid), dim3(256), 0, s, blockCount, (const unsigned long long *)result, 0u,
                       blockTiles);
    hipLaunchKernelGGL(mesh_scan_totals_kernel, dim3(1), dim3(256), 0, s, blockTiles, (const unsigned long long *)result, 0u, ~0ull, result + 1);
    if (capacity_triangles > 0) {
        if (apron) mesh_launch_blocks<true>(c, fp, dp, blockGrid, result, listCapacity, blockCount, blockTiles, true, capacity_triangles, d_positions, d_normals);
        else mesh_launch_blocks<false>(c, fp, dp, blockGrid, result, listCapacity, blockCount, blockTiles, true, capacity_triangles, d_positions, d_normals);
    }
    VH_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    VH_HIP(hipMemcpyAsync(h, result, sizeof h, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    *triangles_out = h[1];
    return check_spin_timeouts(c);
}

// The same into HOST buffers, for callers without a HIP runtime of their own (the C++ facade): device buffers for the call's
// lifetime, one copy back.  Not a hot path.
extern "C" int vh_extract_mesh_host(vh_context *c, const vh_mesh_region *region, uint64_t capacity_triangles, float *h_positions,
                                    float *h_normals, uint64_t *triangles_out)
{
    if (!c || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity_triangles == 0) return vh_extract_mesh(c, region, 0, nullptr, nullptr, triangles_out);
    if (!h_positions) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a position buffer");
    DeviceGuard guard(c->device);
    DevBuf<float> pos, nrm;
    int rc = pos.alloc(capacity_triangles * 9, "mesh positions");
    if (rc == VH_OK && h_normals) rc = nrm.alloc(capacity_triangles * 9, "mesh normals");
    if (rc != VH_OK) return rc;
    rc = vh_extract_mesh(c, region, capacity_triangles, pos, h_normals ? nrm.get() : nullptr, triangles_out);
    if (rc != VH_OK) return rc;
    const size_t bytes = sizeof(float) * 9 * (size_t)std::min<uint64_t>(*triangles_out, capacity_triangles);
    if (bytes) {
        VH_HIP(hipMemcpy(h_positions, pos, bytes, hipMemcpyDeviceToHost));
        if (h_normals) VH_HIP(hipMemcpy(h_normals, nrm, bytes, hipMemcpyDeviceToHost));
    }
    return VH_OK;
}
