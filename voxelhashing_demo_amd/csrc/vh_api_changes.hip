// vh_api_changes.hip -- C-ABI, incremental meshing: vh_changes_state_bytes, vh_changes, vh_extract_mesh_blocks and their _host
// forms (kernels: vh_changes.hip).  Included by vh_api.hip after everything else (same translation unit: shares
// fail(), VH_HIP, DeviceGuard, flush_pending(), reserve_scratch(), the block list and its scans, mesh_launch_blocks()).

// Scratch of vh_changes beside the block list's, and the only place that knows its layout (ChangesScratch::words / ::wide).
struct ChangesParts {
    uint32_t *flags = nullptr, *listPos = nullptr, *slotFlags = nullptr, *slotCount = nullptr;
    unsigned long long *digest = nullptr, *slotTiles = nullptr, *result = nullptr;
};

static int changes_reserve(vh_context *c, size_t blocks, size_t slots, ChangesParts &cp)
{
    const size_t words = blocks + 3 * slots, wide = 2 * blocks + scan_tiles(slots) + 3;
    ChangesScratch &cs = c->changes;
    if (cs.words.size() < words || cs.wide.size() < wide) {
        VH_HIP(hipStreamSynchronize(c->stream));
        DevBuf<uint32_t> w;
        DevBuf<unsigned long long> d;
        int rc;
        if ((rc = w.alloc(words, "change flags")) || (rc = d.alloc(wide, "change digests"))) return rc;
        VH_HIP(hipMemsetAsync(w, 0xff, sizeof(uint32_t) * words, c->stream));       // (listPos: no slot is listed yet)
        cs.words = std::move(w);
        cs.wide = std::move(d);
    }
    cp.flags = cs.words;
    cp.listPos = cp.flags + blocks;
    cp.slotFlags = cp.listPos + slots;
    cp.slotCount = cp.slotFlags + slots;
    cp.digest = cs.wide;
    cp.slotTiles = cp.digest + 2 * blocks;
    cp.result = cp.slotTiles + scan_tiles(slots);
    return VH_OK;
}

extern "C" int vh_changes_state_bytes(vh_context *c, uint64_t *bytes)
{
    if (!c || !bytes) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    *bytes = (uint64_t)kChangesHeaderBytes + (uint64_t)sizeof(ChangesSlot) * ptr_map_size(c);
    return VH_OK;
}

static int changes_check(vh_context *c, const void *state, int32_t what, int32_t halo, uint64_t capacity_changed,
                         const int32_t *changed, uint64_t capacity_removed, const int32_t *removed, const uint64_t *changed_out,
                         const uint64_t *removed_out)
{
    if (!c || !state || !changed_out || !removed_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (!(what & VH_CHANGES_VOXELS) || (what & ~(VH_CHANGES_VOXELS | VH_CHANGES_COLOR)))
        return fail(VH_ERR_INVALID_ARGUMENT, "what must be VH_CHANGES_VOXELS, with or without VH_CHANGES_COLOR");
    if (halo != VH_CHANGES_HALO_NONE && halo != VH_CHANGES_HALO_MESH && halo != VH_CHANGES_HALO_NORMALS)
        return fail(VH_ERR_INVALID_ARGUMENT, "unknown halo");
    if ((capacity_changed > 0 && !changed) || (capacity_removed > 0 && !removed))
        return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a buffer");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table is rebuilt by import, not edited: it has no changes");
    return VH_OK;
}

extern "C" int vh_changes(vh_context *c, void *d_state, const vh_mesh_region *region, int32_t what, int32_t halo,
                          uint64_t capacity_changed, int32_t *d_changed, uint64_t capacity_removed, int32_t *d_removed,
                          uint64_t *changed_out, uint64_t *removed_out)
{
    VH_TRACE("vh_changes");
    int rc = changes_check(c, d_state, what, halo, capacity_changed, d_changed, capacity_removed, d_removed, changed_out, removed_out);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = flush_pending(c)) != VH_OK) return rc;         // the frames queued so far are part of the model

    const BlockBox rg = block_box(region);
    BlockBox grown = rg;                                     // the halo's blocks: one more on every side
    for (int a = 0; a < 3; ++a) {
        grown.lo[a] = rg.lo[a] == INT32_MIN ? rg.lo[a] : rg.lo[a] - 1;
        grown.hi[a] = mesh_grow(rg.hi[a]);
    }
    BlockListScratch sc;
    ChangesParts cp;
    if ((rc = block_list_reserve(c, sc)) != VH_OK) return rc;
    const uint32_t slots = (uint32_t)ptr_map_size(c);
    if ((rc = changes_reserve(c, sc.listCapacity, slots, cp)) != VH_OK) return rc;
    sc.result = cp.result;                                   // one set of result words for the call: {listed, changed, removed}
    const unsigned long long *result = cp.result;

    const FrameParams fp = c->fp;
    const DevPtrs dp = c->dp;
    hipStream_t s = c->stream;
    if ((rc = list_blocks(c, fp, dp, grown, true, sc)) != VH_OK) return rc;

    unsigned long long *epoch = static_cast<unsigned long long *>(d_state);
    ChangesSlot *state = reinterpret_cast<ChangesSlot *>(static_cast<uint8_t *>(d_state) + kChangesHeaderBytes);
    const int4 *items = sc.items;
    const unsigned blockGrid = (unsigned)std::min<size_t>(sc.listCapacity, 8192);
    const unsigned laneGrid = (unsigned)grid_for((size_t)sc.listCapacity + slots, 256);
    hipLaunchKernelGGL(changes_digest_kernel, dim3(blockGrid), dim3(256), 0, s, dp, (const uint32_t *)c->color.get(), rg,
                       (uint32_t)what, items, result, sc.listCapacity, (const ChangesSlot *)state, slots, cp.listPos, cp.flags,
                       cp.digest);
    hipLaunchKernelGGL(changes_stale_kernel, dim3((unsigned)grid_for(slots, 256)), dim3(256), 0, s, fp, dp, rg, items, result,
                       sc.listCapacity, (const ChangesSlot *)state, slots, (const uint32_t *)cp.listPos, cp.slotFlags, cp.slotCount);
    if (halo != VH_CHANGES_HALO_NONE)
        hipLaunchKernelGGL(changes_halo_kernel, dim3(laneGrid), dim3(256), 0, s, fp, dp, (int)halo, items, result, sc.listCapacity,
                           (const ChangesSlot *)state, slots, (const uint32_t *)cp.listPos, (const uint32_t *)cp.slotFlags, cp.flags);
    hipLaunchKernelGGL(changes_count_kernel, dim3((unsigned)grid_for(sc.listCapacity, 256)), dim3(256), 0, s, result,
                       sc.listCapacity, (const uint32_t *)cp.flags, sc.blockCount);
    scan_counts(s, sc.blockCount, result, sc.listCapacity, sc.blockTiles, ~0ull, cp.result + 1);
    scan_counts(s, cp.slotCount, nullptr, slots, cp.slotTiles, ~0ull, cp.result + 2);
    hipLaunchKernelGGL(changes_commit_kernel, dim3(laneGrid), dim3(256), 0, s, rg, items, result, sc.listCapacity, state, slots,
                       epoch, (const uint32_t *)cp.listPos, (const uint32_t *)cp.flags, (const unsigned long long *)cp.digest,
                       (const uint32_t *)sc.blockCount, (const unsigned long long *)sc.blockTiles,
                       (const uint32_t *)cp.slotFlags, (const uint32_t *)cp.slotCount, (const unsigned long long *)cp.slotTiles,
                       (unsigned long long)capacity_changed, reinterpret_cast<int4 *>(d_changed),
                       (unsigned long long)capacity_removed, reinterpret_cast<int4 *>(d_removed));
    VH_HIP(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    VH_HIP(hipMemcpyAsync(h, result, sizeof h, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    *changed_out = h[1];
    *removed_out = h[2];
    return check_spin_timeouts(c);
}

// The same with HOST lists (the state stays a device buffer): device lists the context keeps, one copy back of what a call that
// advanced the state wrote.
extern "C" int vh_changes_host(vh_context *c, void *d_state, const vh_mesh_region *region, int32_t what, int32_t halo,
                               uint64_t capacity_changed, int32_t *h_changed, uint64_t capacity_removed, int32_t *h_removed,
                               uint64_t *changed_out, uint64_t *removed_out)
{
    int rc = changes_check(c, d_state, what, halo, capacity_changed, h_changed, capacity_removed, h_removed, changed_out, removed_out);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    const size_t limit = block_list_capacity(c);             // (no call lists more blocks, or removes more keys, than the pool holds)
    const size_t nc = (size_t)std::min<uint64_t>(capacity_changed, limit), nr = (size_t)std::min<uint64_t>(capacity_removed, ptr_map_size(c));
    if ((rc = reserve_scratch(c, c->changes.hostKeys, 4 * (nc + nr) + 4, "change lists")) != VH_OK) return rc;
    int32_t *dc = c->changes.hostKeys, *dr = dc + 4 * nc;
    // (a clipped capacity that the counts exceed would also exceed the caller's: the call reports and writes nothing either way,
    // unless the caller's capacity is beyond what can ever be listed -- then the clipped one holds everything too)
    rc = vh_changes(c, d_state, region, what, halo, nc, nc ? dc : nullptr, nr, nr ? dr : nullptr, changed_out, removed_out);
    if (rc != VH_OK) return rc;
    if (*changed_out > nc || *removed_out > nr) return VH_OK;
    if (*changed_out) VH_HIP(hipMemcpy(h_changed, dc, sizeof(int32_t) * 4 * (size_t)*changed_out, hipMemcpyDeviceToHost));
    if (*removed_out) VH_HIP(hipMemcpy(h_removed, dr, sizeof(int32_t) * 4 * (size_t)*removed_out, hipMemcpyDeviceToHost));
    return VH_OK;
}

// ---------------------------------------------------------------------------
// the triangles of a list of blocks
// ---------------------------------------------------------------------------
extern "C" int vh_extract_mesh_blocks(vh_context *c, uint64_t n, const int32_t *d_keys, uint64_t capacity_triangles,
                                      float *d_positions, float *d_normals, uint64_t *d_first, uint64_t *triangles_out)
{
    VH_TRACE("vh_extract_mesh_blocks");
    if (!c || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 0 && !d_keys) return fail(VH_ERR_INVALID_ARGUMENT, "keys need a key buffer");
    if (capacity_triangles > 0 && !d_positions) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a position buffer");
    if (n > block_list_capacity(c)) return fail(VH_ERR_INVALID_ARGUMENT, "more keys than the table can hold blocks: extract in parts");
    *triangles_out = 0;
    if (n == 0) return VH_OK;
    DeviceGuard guard(c->device);
    int rc = flush_pending(c);                              // the frames queued so far are part of the model
    if (rc != VH_OK) return rc;

    BlockListScratch sc;
    if ((rc = block_list_reserve(c, sc)) != VH_OK) return rc;
    ChangesScratch &cs = c->changes;
    if ((rc = reserve_scratch(c, cs.keyWords, 2 * (size_t)sc.listCapacity, "mesh key places")) != VH_OK) return rc;
    if ((rc = reserve_scratch(c, cs.keyTiles, scan_tiles(sc.listCapacity), "mesh key scan totals")) != VH_OK) return rc;
    int32_t *keyPtr = reinterpret_cast<int32_t *>(cs.keyWords.get());
    uint32_t *keyCount = cs.keyWords.get() + sc.listCapacity;
    unsigned long long *keyTiles = cs.keyTiles, *result = sc.result;      // {present keys = items, triangles}

    const FrameParams fp = c->fp;
    const DevPtrs dp = model_ptrs(c);
    hipStream_t s = c->stream;
    const int4 *keys = reinterpret_cast<const int4 *>(d_keys);
    const unsigned keyGrid = (unsigned)grid_for((size_t)n + 1, 256);
    hipLaunchKernelGGL(mesh_keys_resolve_kernel, dim3(keyGrid), dim3(256), 0, s, fp, dp, keys, (uint32_t)n, keyPtr, keyCount);
    scan_counts(s, keyCount, nullptr, (size_t)n, keyTiles, sc.listCapacity, result);
    hipLaunchKernelGGL(mesh_keys_items_kernel, dim3(keyGrid), dim3(256), 0, s, keys, (uint32_t)n, (const int32_t *)keyPtr,
                       (const uint32_t *)keyCount, (const unsigned long long *)keyTiles, sc.items, sc.listCapacity);

    const auto pass = c->meshVariant == 0 ? mesh_launch_blocks<true> : mesh_launch_blocks<false>;
    pass(c, fp, dp, sc, false, 0, nullptr, nullptr);
    scan_counts(s, sc.blockCount, result, sc.listCapacity, sc.blockTiles, ~0ull, result + 1);
    if (capacity_triangles > 0) pass(c, fp, dp, sc, true, capacity_triangles, d_positions, d_normals);
    if (d_first)
        hipLaunchKernelGGL(mesh_keys_first_kernel, dim3(keyGrid), dim3(256), 0, s, (uint32_t)n, (const uint32_t *)keyCount,
                           (const unsigned long long *)keyTiles, (const uint32_t *)sc.blockCount,
                           (const unsigned long long *)sc.blockTiles, (const unsigned long long *)result,
                           reinterpret_cast<unsigned long long *>(d_first));
    VH_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    VH_HIP(hipMemcpyAsync(h, result, sizeof h, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    *triangles_out = h[1];
    return check_spin_timeouts(c);
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade).  Not a hot path.
extern "C" int vh_extract_mesh_blocks_host(vh_context *c, uint64_t n, const int32_t *h_keys, uint64_t capacity_triangles,
                                           float *h_positions, float *h_normals, uint64_t *h_first, uint64_t *triangles_out)
{
    if (!c || !triangles_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 0 && !h_keys) return fail(VH_ERR_INVALID_ARGUMENT, "keys need a key buffer");
    if (capacity_triangles > 0 && !h_positions) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a position buffer");
    if (n > block_list_capacity(c)) return fail(VH_ERR_INVALID_ARGUMENT, "more keys than the table can hold blocks: extract in parts");
    *triangles_out = 0;
    if (n == 0) return VH_OK;
    DeviceGuard guard(c->device);
    DevBuf<float> pos, nrm;
    int rc = reserve_scratch(c, c->changes.hostKeys, 4 * (size_t)n, "mesh keys");
    if (rc == VH_OK) rc = reserve_scratch(c, c->changes.hostFirst, (size_t)n + 1, "mesh offsets");
    if (rc == VH_OK && capacity_triangles) rc = pos.alloc(capacity_triangles * 9, "mesh positions");
    if (rc == VH_OK && capacity_triangles && h_normals) rc = nrm.alloc(capacity_triangles * 9, "mesh normals");
    if (rc != VH_OK) return rc;
    const bool normals = capacity_triangles && h_normals;
    VH_HIP(hipMemcpyAsync(c->changes.hostKeys, h_keys, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    rc = vh_extract_mesh_blocks(c, n, c->changes.hostKeys, capacity_triangles, capacity_triangles ? pos.get() : nullptr,
                                normals ? nrm.get() : nullptr, reinterpret_cast<uint64_t *>(c->changes.hostFirst.get()), triangles_out);
    if (rc != VH_OK) return rc;
    const size_t bytes = sizeof(float) * 9 * (size_t)std::min<uint64_t>(*triangles_out, capacity_triangles);
    if (bytes) {
        VH_HIP(hipMemcpy(h_positions, pos, bytes, hipMemcpyDeviceToHost));
        if (normals) VH_HIP(hipMemcpy(h_normals, nrm, bytes, hipMemcpyDeviceToHost));
    }
    if (h_first) VH_HIP(hipMemcpy(h_first, c->changes.hostFirst, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    return VH_OK;
}
