// vh_api_mesh.hip -- C-ABI, the way out of the volume: vh_extract_mesh, vh_extract_mesh_indexed (kernels: vh_mesh.hip).
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

// ---------------------------------------------------------------------------
// the indexed form
// ---------------------------------------------------------------------------
// Scratch of the indexed call alone, beside mesh_reserve's: 2 KB of words and a vertex count per listed block, and the map
// from a block's ptr >> 9 to its list position (unique per block: heap blocks lie 512 voxels apart, view records 514).
static int mesh_reserve_indexed(vh_context *c, size_t blocks, size_t listPosSize)
{
    const size_t words = blocks * 512 + blocks + listPosSize, totals = (blocks + kMeshScanTile - 1) / kMeshScanTile + 3;
    if (c->meshWords.size() >= words && c->meshVertexTotals.size() >= totals) return VH_OK;
    VH_HIP(hipStreamSynchronize(c->stream));
    DevBuf<uint32_t> w;
    DevBuf<unsigned long long> tot;
    int rc;
    if ((rc = w.alloc(words, "mesh vertex words")) || (rc = tot.alloc(totals, "mesh vertex scan totals"))) return rc;
    c->meshWords = std::move(w);
    c->meshVertexTotals = std::move(tot);
    return VH_OK;
}

static int32_t mesh_grow(int32_t hi) { return hi == INT32_MAX ? hi : hi + 1; }

extern "C" int vh_extract_mesh_indexed(vh_context *c, const vh_mesh_region *region, uint64_t capacity_vertices,
                                       uint64_t capacity_triangles, float *d_vertices, float *d_vertex_normals, uint32_t *d_indices,
                                       uint64_t *vertices_out, uint64_t *triangles_out)
{
    VH_TRACE("vh_extract_mesh_indexed");
    if (!c || !vertices_out || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity_vertices > 0 && !d_vertices) return fail(VH_ERR_INVALID_ARGUMENT, "a vertex capacity needs a vertex buffer");
    if (capacity_triangles > 0 && !d_indices) return fail(VH_ERR_INVALID_ARGUMENT, "a triangle capacity needs an index buffer");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }

    MeshRegion rg, grown;                  // the cells' blocks; the vertices' blocks: one more towards +
    for (int a = 0; a < 3; ++a) {
        rg.lo[a] = grown.lo[a] = region ? region->block_lo[a] : INT32_MIN;
        rg.hi[a] = region ? region->block_hi[a] : INT32_MAX;
        grown.hi[a] = mesh_grow(rg.hi[a]);
    }
    const size_t slices = ((size_t)c->ownedBuckets + kMeshSliceBuckets - 1) / kMeshSliceBuckets;
    const size_t blocks = std::max<size_t>(1, std::min<size_t>(c->numEntries, c->viewBlocks ? (size_t)c->viewCount : (size_t)c->params.numVoxelBlocks));
    const size_t listPosSize = c->viewBlocks ? (((size_t)c->viewCount * 514 + 2) >> 9) + 1 : (size_t)c->params.numVoxelBlocks;
    { const int rc = mesh_reserve(c, slices, blocks); if (rc != VH_OK) return rc; }
    const size_t listed = c->meshItems.size();
    { const int rc = mesh_reserve_indexed(c, listed, listPosSize); if (rc != VH_OK) return rc; }
    const uint32_t listCapacity = (uint32_t)listed;
    const size_t tiles = (listed + kMeshScanTile - 1) / kMeshScanTile;
    uint32_t *sliceCount = c->meshCounts, *triangleCount = sliceCount + slices;
    unsigned long long *sliceTiles = c->meshTotals;
    unsigned long long *triangleTiles = sliceTiles + (slices + kMeshScanTile - 1) / kMeshScanTile;
    uint32_t *word = c->meshWords, *vertexCount = word + listed * 512, *listPos = vertexCount + listed;
    unsigned long long *vertexTiles = c->meshVertexTotals, *result = vertexTiles + tiles;    // {listed blocks, vertices, triangles}

    FrameParams fp = c->fp;
    DevPtrs dp = c->dp;
    if (c->viewBlocks) dp.blocks = const_cast<Voxel *>(c->viewBlocks);
    hipStream_t s = c->stream;
    const unsigned listGrid = (unsigned)grid_for(slices, 4), sliceTileGrid = (unsigned)grid_for(slices, kMeshScanTile);
    hipLaunchKernelGGL(mesh_list_kernel<false>, dim3(listGrid), dim3(256), 0, s, fp, dp, grown, c->ownedBuckets, (uint32_t)slices,
                       sliceCount, (const unsigned long long *)sliceTiles, (int4 *)c->meshItems, listCapacity);
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(sliceTileGrid), dim3(256), 0, s, sliceCount, (const unsigned long long *)nullptr,
                       (uint32_t)slices, sliceTiles);
    hipLaunchKernelGGL(mesh_scan_totals_kernel, dim3(1), dim3(256), 0, s, sliceTiles, (const unsigned long long *)nullptr,
                       (uint32_t)slices, (unsigned long long)listCapacity, result);
    hipLaunchKernelGGL(mesh_list_kernel<true>, dim3(listGrid), dim3(256), 0, s, fp, dp, grown, c->ownedBuckets, (uint32_t)slices,
                       sliceCount, (const unsigned long long *)sliceTiles, (int4 *)c->meshItems, listCapacity);

    const unsigned blockGrid = (unsigned)std::min<size_t>(listed, 8192), tileGrid = (unsigned)grid_for(listed, kMeshScanTile);
    const int4 *items = c->meshItems;
    hipLaunchKernelGGL(mesh_indexed_count_kernel, dim3(blockGrid), dim3(256), 0, s, fp, dp, rg, items, (const unsigned long long *)result,
                       listCapacity, listPos, (uint32_t)listPosSize, word, vertexCount, triangleCount);
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(tileGrid), dim3(256), 0, s, vertexCount, (const unsigned long long *)result, 0u, vertexTiles);
    hipLaunchKernelGGL(mesh_scan_totals_kernel, dim3(1), dim3(256), 0, s, vertexTiles, (const unsigned long long *)result, 0u, ~0ull, result + 1);
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(tileGrid), dim3(256), 0, s, triangleCount, (const unsigned long long *)result, 0u, triangleTiles);
    hipLaunchKernelGGL(mesh_scan_totals_kernel, dim3(1), dim3(256), 0, s, triangleTiles, (const unsigned long long *)result, 0u, ~0ull, result + 2);
    if (capacity_vertices > 0 || capacity_triangles > 0) {
        if (d_vertex_normals)
            hipLaunchKernelGGL(mesh_indexed_emit_kernel<true>, dim3(blockGrid), dim3(256), 0, s, fp, dp, rg, items,
                               (const unsigned long long *)result, listCapacity, (const uint32_t *)listPos, (uint32_t)listPosSize,
                               (const uint32_t *)word, (const uint32_t *)vertexCount, (const unsigned long long *)vertexTiles,
                               (const uint32_t *)triangleCount, (const unsigned long long *)triangleTiles,
                               (unsigned long long)capacity_vertices, (unsigned long long)capacity_triangles, d_vertices,
                               d_vertex_normals, d_indices);
        else
            hipLaunchKernelGGL(mesh_indexed_emit_kernel<false>, dim3(blockGrid), dim3(256), 0, s, fp, dp, rg, items,
                               (const unsigned long long *)result, listCapacity, (const uint32_t *)listPos, (uint32_t)listPosSize,
                               (const uint32_t *)word, (const uint32_t *)vertexCount, (const unsigned long long *)vertexTiles,
                               (const uint32_t *)triangleCount, (const unsigned long long *)triangleTiles,
                               (unsigned long long)capacity_vertices, (unsigned long long)capacity_triangles, d_vertices,
                               d_vertex_normals, d_indices);
    }
    VH_HIP(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    VH_HIP(hipMemcpyAsync(h, result, sizeof h, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    *vertices_out = h[1];
    *triangles_out = h[2];
    if (h[1] > 0xffffffffull) return fail(VH_ERR_INVALID_ARGUMENT, "more vertices than a 32-bit index names: extract by regions");
    return check_spin_timeouts(c);
}

extern "C" int vh_extract_mesh_indexed_host(vh_context *c, const vh_mesh_region *region, uint64_t capacity_vertices,
                                            uint64_t capacity_triangles, float *h_vertices, float *h_vertex_normals,
                                            uint32_t *h_indices, uint64_t *vertices_out, uint64_t *triangles_out)
{
    if (!c || !vertices_out || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity_vertices > 0 && !h_vertices) return fail(VH_ERR_INVALID_ARGUMENT, "a vertex capacity needs a vertex buffer");
    if (capacity_triangles > 0 && !h_indices) return fail(VH_ERR_INVALID_ARGUMENT, "a triangle capacity needs an index buffer");
    DeviceGuard guard(c->device);
    DevBuf<float> pos, nrm;
    DevBuf<uint32_t> idx;
    int rc = VH_OK;
    if (capacity_vertices) rc = pos.alloc(capacity_vertices * 3, "mesh vertices");
    if (rc == VH_OK && capacity_vertices && h_vertex_normals) rc = nrm.alloc(capacity_vertices * 3, "mesh vertex normals");
    if (rc == VH_OK && capacity_triangles) rc = idx.alloc(capacity_triangles * 3, "mesh indices");
    if (rc != VH_OK) return rc;
    const bool normals = capacity_vertices && h_vertex_normals;
    rc = vh_extract_mesh_indexed(c, region, capacity_vertices, capacity_triangles, capacity_vertices ? pos.get() : nullptr,
                                 normals ? nrm.get() : nullptr, capacity_triangles ? idx.get() : nullptr, vertices_out, triangles_out);
    if (rc != VH_OK) return rc;
    const size_t vbytes = sizeof(float) * 3 * (size_t)std::min<uint64_t>(*vertices_out, capacity_vertices);
    const size_t ibytes = sizeof(uint32_t) * 3 * (size_t)std::min<uint64_t>(*triangles_out, capacity_triangles);
    if (vbytes) {
        VH_HIP(hipMemcpy(h_vertices, pos, vbytes, hipMemcpyDeviceToHost));
        if (normals) VH_HIP(hipMemcpy(h_vertex_normals, nrm, vbytes, hipMemcpyDeviceToHost));
    }
    if (ibytes) VH_HIP(hipMemcpy(h_indices, idx, ibytes, hipMemcpyDeviceToHost));
    return VH_OK;
}
