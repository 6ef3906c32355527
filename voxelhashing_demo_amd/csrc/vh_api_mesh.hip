// vh_api_mesh.hip -- C-ABI, the way out of the volume: vh_extract_mesh, vh_extract_mesh_indexed (kernels: vh_mesh.hip).
// Included by vh_api.hip behind vh_api_blocklist.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, flush_pending(),
// the block list and its scans).

// one pass of mesh_block_kernel over the listed blocks: the count pass, or the emitting one
template <bool kApron>
static void mesh_launch_blocks(vh_context *c, const FrameParams &fp, const DevPtrs &dp, const BlockListScratch &sc, bool emit,
                               unsigned long long capacity, float *positions, float *normals)
{
    const unsigned grid = (unsigned)std::min<size_t>(sc.listCapacity, 8192);
    const int4 *items = sc.items;
    const unsigned long long *numItems = sc.result, *tileBase = sc.blockTiles;
    if (!emit)
        hipLaunchKernelGGL((mesh_block_kernel<kApron, false, false>), dim3(grid), dim3(256), 0, c->stream, fp, dp, items, numItems,
                           sc.listCapacity, sc.blockCount, tileBase, 0ull, (float *)nullptr, (float *)nullptr);
    else if (normals)
        hipLaunchKernelGGL((mesh_block_kernel<kApron, true, true>), dim3(grid), dim3(256), 0, c->stream, fp, dp, items, numItems,
                           sc.listCapacity, sc.blockCount, tileBase, capacity, positions, normals);
    else
        hipLaunchKernelGGL((mesh_block_kernel<kApron, true, false>), dim3(grid), dim3(256), 0, c->stream, fp, dp, items, numItems,
                           sc.listCapacity, sc.blockCount, tileBase, capacity, positions, normals);
}

extern "C" int vh_extract_mesh(vh_context *c, const vh_mesh_region *region, uint64_t capacity_triangles, float *d_positions,
                               float *d_normals, uint64_t *triangles_out)
{
    VH_TRACE("vh_extract_mesh");
    if (!c || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity_triangles > 0 && !d_positions) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a position buffer");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // the frames queued so far are part of the model

    const FrameParams fp = c->fp;
    const DevPtrs dp = model_ptrs(c);
    hipStream_t s = c->stream;
    BlockListScratch sc;
    { const int rc = list_blocks(c, fp, dp, block_box(region), true, sc); if (rc != VH_OK) return rc; }
    unsigned long long *result = sc.result;            // {listed blocks, triangles}

    const auto pass = c->meshVariant == 0 ? mesh_launch_blocks<true> : mesh_launch_blocks<false>;
    pass(c, fp, dp, sc, false, 0, nullptr, nullptr);
    scan_counts(s, sc.blockCount, result, sc.listCapacity, sc.blockTiles, ~0ull, result + 1);
    if (capacity_triangles > 0) pass(c, fp, dp, sc, true, capacity_triangles, d_positions, d_normals);
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
// Scratch of the indexed call alone, beside the block list's, and the only place that knows its layout.  meshWords: 2 KB of
// words per listed block, a vertex count per block, then the map from a block's ptr >> 9 to its list position.
// meshVertexTotals: the vertex scan's tile totals, then the call's three result words.
struct IndexedMeshScratch {
    uint32_t *word = nullptr, *vertexCount = nullptr, *listPos = nullptr;
    uint32_t listPosSize = 0;
    unsigned long long *vertexTiles = nullptr, *result = nullptr;
};

static int mesh_reserve_indexed(vh_context *c, size_t blocks, IndexedMeshScratch &ix)
{
    const size_t listPosSize = ptr_map_size(c);
    const size_t words = blocks * 512 + blocks + listPosSize, totals = scan_tiles(blocks) + 3;
    if (c->meshWords.size() < words || c->meshVertexTotals.size() < totals) {
        VH_HIP(hipStreamSynchronize(c->stream));
        DevBuf<uint32_t> w;
        DevBuf<unsigned long long> tot;
        int rc;
        if ((rc = w.alloc(words, "mesh vertex words")) || (rc = tot.alloc(totals, "mesh vertex scan totals"))) return rc;
        c->meshWords = std::move(w);
        c->meshVertexTotals = std::move(tot);
    }
    ix.word = c->meshWords;
    ix.vertexCount = ix.word + blocks * 512;
    ix.listPos = ix.vertexCount + blocks;
    ix.listPosSize = (uint32_t)listPosSize;
    ix.vertexTiles = c->meshVertexTotals;
    ix.result = ix.vertexTiles + scan_tiles(blocks);
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

    const BlockBox rg = block_box(region);  // the cells' blocks
    BlockBox grown = rg;                    // the vertices' blocks: one more towards +
    for (int a = 0; a < 3; ++a) grown.hi[a] = mesh_grow(rg.hi[a]);
    BlockListScratch sc;
    IndexedMeshScratch ix;
    { const int rc = block_list_reserve(c, sc); if (rc != VH_OK) return rc; }
    { const int rc = mesh_reserve_indexed(c, sc.listCapacity, ix); if (rc != VH_OK) return rc; }
    sc.result = ix.result;                  // one set of result words for the call: {listed blocks, vertices, triangles}
    const unsigned long long *result = ix.result;
    uint32_t *triangleCount = sc.blockCount;
    unsigned long long *triangleTiles = sc.blockTiles;

    const FrameParams fp = c->fp;
    const DevPtrs dp = model_ptrs(c);
    hipStream_t s = c->stream;
    { const int rc = list_blocks(c, fp, dp, grown, true, sc); if (rc != VH_OK) return rc; }

    const unsigned blockGrid = (unsigned)std::min<size_t>(sc.listCapacity, 8192);
    const int4 *items = sc.items;
    hipLaunchKernelGGL(mesh_indexed_count_kernel, dim3(blockGrid), dim3(256), 0, s, fp, dp, rg, items, result, sc.listCapacity,
                       ix.listPos, ix.listPosSize, ix.word, ix.vertexCount, triangleCount);
    scan_counts(s, ix.vertexCount, result, sc.listCapacity, ix.vertexTiles, ~0ull, ix.result + 1);
    scan_counts(s, triangleCount, result, sc.listCapacity, triangleTiles, ~0ull, ix.result + 2);
    if (capacity_vertices > 0 || capacity_triangles > 0) {
        const auto emit = d_vertex_normals ? mesh_indexed_emit_kernel<true> : mesh_indexed_emit_kernel<false>;
        hipLaunchKernelGGL(emit, dim3(blockGrid), dim3(256), 0, s, fp, dp, rg, items, result, sc.listCapacity,
                           (const uint32_t *)ix.listPos, ix.listPosSize, (const uint32_t *)ix.word, (const uint32_t *)ix.vertexCount,
                           (const unsigned long long *)ix.vertexTiles, (const uint32_t *)triangleCount,
                           (const unsigned long long *)triangleTiles, (unsigned long long)capacity_vertices,
                           (unsigned long long)capacity_triangles, d_vertices, d_vertex_normals, d_indices);
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
