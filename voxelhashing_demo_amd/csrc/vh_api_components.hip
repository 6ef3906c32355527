// vh_api_components.hip -- C-ABI, connected pieces of the model: vh_components, vh_components_host, vh_remove_components
// (kernels: vh_components.hip).  Included by vh_api.hip after everything else (same translation unit: shares fail(), VH_HIP,
// DeviceGuard, launch(), settle(), the block list and its scans, sweep_and_release(), reserve_scratch()).
// Both calls read their stats back: they synchronise the context's stream.

// What a call labels and, optionally, writes.
struct ComponentsCall {
    const vh_mesh_region *region = nullptr;
    int32_t target = 0, connectivity = 0;
    uint64_t capacity = 0;
    vh_component *records = nullptr;
    bool haveBox = false;
    LatticeBox box{};
    unsigned long long bricks = 0;
    uint32_t *labels = nullptr;
    bool remove = false;
    uint64_t minSize = 0;
};

// The argument checks of both calls; the box follows vh_sample_lattice.
static int components_check(vh_context *c, int32_t target, int32_t connectivity, const int32_t lo[3], const int32_t dims[3],
                            uint32_t *d_labels, ComponentsCall *call)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (target != VH_COMPONENT_INSIDE && target != VH_COMPONENT_OUTSIDE) return fail(VH_ERR_INVALID_ARGUMENT, "unknown component target");
    if (connectivity != 6 && connectivity != 14) return fail(VH_ERR_INVALID_ARGUMENT, "connectivity must be 6 or 14");
    call->target = target;
    call->connectivity = connectivity;
    if (!lo && !dims && !d_labels) return VH_OK;
    if (!lo || !dims || !d_labels) return fail(VH_ERR_INVALID_ARGUMENT, "a label box needs lo, dims and a label buffer");
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 0) return fail(VH_ERR_INVALID_ARGUMENT, "negative lattice dimension");
        if ((int64_t)lo[a] + (int64_t)dims[a] > (int64_t)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "lo + dims beyond int32");
        empty = empty || dims[a] == 0;
        call->box.lo[a] = lo[a];
        call->box.dims[a] = dims[a];
        call->box.brick0[a] = lo[a] >> 3;
        call->box.bricks[a] = dims[a] ? ((lo[a] + dims[a] - 1) >> 3) - call->box.brick0[a] + 1 : 0;
    }
    if (empty) return VH_OK;                            // nothing to label
    unsigned long long bricks = (unsigned long long)call->box.bricks[0] * (unsigned long long)call->box.bricks[1];
    if (bricks > (~0ull >> 30)) return fail(VH_ERR_INVALID_ARGUMENT, "lattice too large");
    call->bricks = bricks * (unsigned long long)call->box.bricks[2];
    call->haveBox = true;
    call->labels = d_labels;
    return VH_OK;
}

// Everything up to the stats on the host: the list, the labelling, the records, the labels of the box, the removal's clearing
// pass.  One synchronisation.
static int components_run(vh_context *c, const ComponentsCall &call, vh_component_stats *stats)
{
    vh_component_stats st{};
    *stats = st;
    int rc = settle(c);                                 // the frames queued so far are part of the model
    if (rc != VH_OK) return rc;
    const BlockBox rg = block_box(call.region);
    bool emptyRegion = false;
    for (int a = 0; a < 3; ++a) emptyRegion = emptyRegion || rg.lo[a] >= rg.hi[a];
    const FrameParams fp = c->fp;
    const DevPtrs dp = model_ptrs(c);
    hipStream_t s = c->stream;
    if (emptyRegion) {                                  // no block is listed: no component, every label of the box is NONE
        if (call.haveBox) {
            const size_t n = (size_t)call.box.dims[0] * (size_t)call.box.dims[1] * (size_t)call.box.dims[2];
            VH_HIP(hipMemsetAsync(call.labels, 0xFF, sizeof(uint32_t) * n, s));
            VH_HIP(hipStreamSynchronize(s));
        }
        return VH_OK;
    }

    // 1. the ordered block list with the region as predicate (its scratch first: it sizes this call's own)
    BlockListScratch sc;
    if ((rc = block_list_reserve(c, sc)) != VH_OK) return rc;
    const size_t rankSize = ptr_map_size(c);
    const uint32_t listCapacity = sc.listCapacity;
    const size_t labelled = std::min<size_t>(listCapacity, kCompMaxBlocks);       // (beyond the limit nothing is labelled)
    ComponentScratch &cs = c->components;
    if ((rc = reserve_scratch(c, cs.parent, labelled * kBlockVoxels, "component parents")) != VH_OK) return rc;
    if ((rc = reserve_scratch(c, cs.rank, rankSize, "component block ranks")) != VH_OK) return rc;
    if ((rc = reserve_scratch(c, cs.rootBits, labelled * 8 + kCompWords, "component root bits")) != VH_OK) return rc;
    if (call.remove && (rc = reserve_scratch(c, cs.keys, labelled, "component key list")) != VH_OK) return rc;
    uint32_t *rootCount = sc.blockCount;
    unsigned long long *rootTiles = sc.blockTiles, *result = sc.result;             // {listed blocks, components}
    unsigned long long *rootBits = cs.rootBits, *words = rootBits + labelled * 8;
    uint32_t *parent = cs.parent, *rank = cs.rank;
    const int4 *items = sc.items;
    const unsigned long long *numItems = result;

    VH_HIP(hipMemsetAsync(rank, 0xFF, sizeof(uint32_t) * rankSize, s));     // no block is listed yet
    VH_HIP(hipMemsetAsync(words, 0, sizeof(unsigned long long) * kCompWords, s));
    VH_HIP(hipMemsetAsync(result, 0, sizeof(unsigned long long) * 2, s));
    if ((rc = list_blocks(c, fp, dp, rg, true, sc)) != VH_OK) return rc;

    // 2. the labelling.  ("components_launches" k = 1..6: a timing run stops behind stage k and returns no result)
    const int stages = c->componentsLaunches ? c->componentsLaunches : 7;
    const unsigned blockGrid = (unsigned)std::min<size_t>(labelled, 8192);
    if (stages >= 2)
        hipLaunchKernelGGL(comp_local_kernel, dim3(blockGrid), dim3(256), 0, s, dp, items, numItems, listCapacity, (int)call.target,
                           (int)call.connectivity, parent, rank, (uint32_t)rankSize);
    if (stages >= 3)
        hipLaunchKernelGGL(comp_seam_kernel, dim3(blockGrid), dim3(256), 0, s, fp, dp, items, numItems, listCapacity,
                           (int)call.connectivity, parent, (const uint32_t *)rank, (uint32_t)rankSize);
    if (stages >= 4)
        hipLaunchKernelGGL(comp_flatten_kernel, dim3(blockGrid), dim3(256), 0, s, numItems, listCapacity, parent, rootBits, rootCount);
    if (stages >= 5)
        hipLaunchKernelGGL(comp_count_kernel, dim3(blockGrid), dim3(256), 0, s, numItems, listCapacity, parent,
                           (const unsigned long long *)rootBits, words);
    if (stages >= 6) {
        // 3. the roots in id order: the scan over the roots per block, then the records
        scan_counts(s, rootCount, numItems, listCapacity, rootTiles, ~0ull, result + 1);
        hipLaunchKernelGGL(comp_records_kernel, dim3(blockGrid), dim3(256), 0, s, items, numItems, listCapacity, (const uint32_t *)parent,
                           (const unsigned long long *)rootBits, (const uint32_t *)rootCount, (const unsigned long long *)rootTiles,
                           (unsigned long long)call.capacity, reinterpret_cast<CompRecord *>(call.records), words);
    }
    if (stages >= 7 && call.haveBox) {
        const unsigned grid = (unsigned)std::min<unsigned long long>(call.bricks, 1ull << 20);
        hipLaunchKernelGGL(comp_labels_kernel, dim3(grid), dim3(256), 0, s, fp, dp, call.box, call.bricks, numItems, listCapacity,
                           (const uint32_t *)parent, (const unsigned long long *)rootBits, (const uint32_t *)rootCount,
                           (const unsigned long long *)rootTiles, (const uint32_t *)rank, (uint32_t)rankSize, call.labels);
    }
    if (stages >= 7 && call.remove)
        hipLaunchKernelGGL(comp_remove_kernel, dim3(blockGrid), dim3(256), 0, s, dp, c->color.get(), items, numItems, listCapacity,
                           (const uint32_t *)parent, (const unsigned long long *)rootBits, (unsigned long long)call.minSize,
                           cs.keys.get(), words);
    VH_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0}, w[kCompWords] = {};
    VH_HIP(hipMemcpyAsync(h, result, sizeof h, hipMemcpyDeviceToHost, s));
    VH_HIP(hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    if ((rc = check_spin_timeouts(c)) != VH_OK) return rc;
    st.blocks = h[0];
    if (h[0] > (unsigned long long)kCompMaxBlocks) {
        *stats = st;
        return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^23 - 1 listed blocks: label by regions");
    }
    st.components = h[1];
    st.nodes = w[kCompNodes];
    st.largest = w[kCompLargest];
    st.removed_components = w[kCompRemovedComponents];
    st.removed_voxels = w[kCompRemovedVoxels];
    st.freed_blocks = w[kCompFreedBlocks];
    *stats = st;
    return VH_OK;
}

extern "C" int vh_components(vh_context *c, const vh_mesh_region *region, int32_t target, int32_t connectivity, uint64_t capacity,
                             vh_component *d_components, const int32_t lo[3], const int32_t dims[3], uint32_t *d_labels,
                             vh_component_stats *stats)
{
    VH_TRACE("vh_components");
    if (!c || !stats) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity > 0 && !d_components) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a record buffer");
    ComponentsCall call;
    const int rc = components_check(c, target, connectivity, lo, dims, d_labels, &call);
    if (rc != VH_OK) return rc;
    call.region = region;
    call.capacity = capacity;
    call.records = d_components;
    DeviceGuard guard(c->device);
    return components_run(c, call, stats);
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade): device buffers for the call's
// lifetime, one copy back.  Not a hot path.
extern "C" int vh_components_host(vh_context *c, const vh_mesh_region *region, int32_t target, int32_t connectivity,
                                  uint64_t capacity, vh_component *h_components, const int32_t lo[3], const int32_t dims[3],
                                  uint32_t *h_labels, vh_component_stats *stats)
{
    if (!c || !stats) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity > 0 && !h_components) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a record buffer");
    ComponentsCall call;
    int rc = components_check(c, target, connectivity, lo, dims, h_labels, &call);       // (before anything is allocated)
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    DevBuf<vh_component> rec;
    DevBuf<uint32_t> lab;
    const size_t voxels = call.haveBox ? (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2] : 0;
    if (capacity && (rc = rec.alloc((size_t)capacity, "component records")) != VH_OK) return rc;
    if (voxels && (rc = lab.alloc(voxels, "component labels")) != VH_OK) return rc;
    const bool box = lo && dims && h_labels;
    rc = vh_components(c, region, target, connectivity, capacity, capacity ? rec.get() : nullptr, box ? lo : nullptr,
                       box ? dims : nullptr, box ? (voxels ? lab.get() : h_labels) : nullptr, stats);
    if (rc != VH_OK) return rc;
    const size_t got = (size_t)std::min<uint64_t>(stats->components, capacity);
    if (got) VH_HIP(hipMemcpy(h_components, rec, got * sizeof(vh_component), hipMemcpyDeviceToHost));
    if (voxels) VH_HIP(hipMemcpy(h_labels, lab, voxels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VH_OK;
}

extern "C" int vh_remove_components(vh_context *c, const vh_mesh_region *region, int32_t target, int32_t connectivity,
                                    uint64_t min_size, vh_component_stats *stats)
{
    VH_TRACE("vh_remove_components");
    ComponentsCall call;
    int rc = components_check(c, target, connectivity, nullptr, nullptr, nullptr, &call);
    if (rc != VH_OK) return rc;
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    call.region = region;
    call.remove = true;
    call.minSize = min_size;
    DeviceGuard guard(c->device);
    vh_component_stats st{};
    if (stats) *stats = st;
    if ((rc = components_run(c, call, &st)) != VH_OK) return rc;
    if (stats) *stats = st;
    // the blocks that emptied: vh_delete_blocks on their keys, in a lock epoch of its own (none: the call of no keys)
    if ((rc = vh_reset_mutexes(c)) != VH_OK) return rc;
    if (st.freed_blocks > 0) {
        rc = launch(c, kPhaseGc, gc_mark_keys_kernel, dim3((unsigned)grid_for((size_t)st.freed_blocks, 256)), dim3(256), c->fp, c->dp,
                    (const int4 *)c->components.keys.get(), (int32_t)st.freed_blocks);
        if (rc != VH_OK) return rc;
    }
    if ((rc = sweep_and_release(c)) != VH_OK) return rc;
    VH_HIP(hipStreamSynchronize(c->stream));
    VH_HIP(hipGetLastError());
    return VH_OK;
}
