// vh_api_labels.hip -- C-ABI, the model with labels: vh_integrate_labels*, vh_sample_labels*, vh_raycast_labels, vh_label_counts,
// vh_remove_label, the label volume's housekeeping (kernels: vh_labels.hip).  Included by vh_api.hip after
// everything else (same translation unit: shares fail(), VH_HIP, DeviceGuard, launch(), flush_pending(), settle(), vh_set_pose(),
// vh_flatten(), vh_raycast_maps(), the block list and its scans, sweep_and_release(), reserve_scratch()).
// The fusing, reading and counting calls only enqueue; vh_remove_label and vh_download_labels read back and synchronise.  The
// one allocation a fusing call makes is the label volume itself, made and zeroed by the first one into a context and kept.

static size_t label_words(const vh_context *c) { return (size_t)c->params.numVoxelBlocks * kBlockVoxels; }

// The volume of the first label-fusing call: all or nothing.
static int ensure_labels(vh_context *c)
{
    if (c->labels) return VH_OK;
    DevBuf<uint32_t> fresh;
    const int rc = fresh.alloc(label_words(c), "label volume");
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemsetAsync(fresh, 0, sizeof(uint32_t) * label_words(c), c->stream));
    c->labels = std::move(fresh);
    return VH_OK;
}

// sweep_and_release, ahead of gc_release_kernel: the freed blocks' label words go back to zero (colour's launch, this volume)
static int release_labels(vh_context *c)
{
    if (!c->labels) return VH_OK;
    return launch(c, kPhaseGc, color_release_kernel, dim3(1024), dim3(256), c->dp, c->labels.get());
}

// vh_load_snapshot re-deals the ptrs and snapshots carry no labels: the volume, if there is one, starts over
static hipError_t reset_labels(vh_context *c)
{
    if (!c->labels) return hipSuccess;
    return hipMemsetAsync(c->labels, 0, sizeof(uint32_t) * label_words(c), c->stream);
}

static int check_label_frame(const vh_context *c, float band, int32_t vote_max)
{
    if (!std::isfinite(band) || !(band > 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "band must be finite and positive");
    if (vote_max < 0 || vote_max > 65535) return fail(VH_ERR_INVALID_ARGUMENT, "vote_max must be 0..65535");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks: its voxels live in the caller's records");
    return VH_OK;
}

// pose -> the step-level flatten, called as it is -> one launch over the list it left (integrate_color_impl's shape)
template <class Depth>
static int integrate_labels_impl(vh_context *c, const float pose[16], const Depth &depth, const uint16_t *d_labels, float band,
                                 int32_t vote_max)
{
    int rc = check_label_frame(c, band, vote_max);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = ensure_labels(c)) != VH_OK) return rc; // (before anything changes)
    rc = flush_pending(c);                           // the frames queued so far are part of the model
    if (rc == VH_OK) rc = vh_set_pose(c, pose);
    if (rc == VH_OK) rc = vh_flatten(c, nullptr);    // (no occupied_out: the count stays on the device)
    if (rc != VH_OK) return rc;
    rc = launch(c, kPhaseIntegrate, label_integrate_kernel<Depth>, dim3((unsigned)c->integrateGrid), dim3(256), c->fp, c->dp, depth,
                c->labels.get(), d_labels, band, (uint32_t)vote_max);
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_integrate_labels(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                                   const uint16_t *d_labels, float band, int32_t vote_max)
{
    VH_TRACE("vh_integrate_labels");
    if (!c || !pose || !d_depth || !k_inv || !d_labels) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return integrate_labels_impl(c, pose, DepthSensor{d_depth, k_inv[6], k_inv[7], k_inv[8], 5000.0f}, d_labels, band, vote_max);
}

extern "C" int vh_integrate_labels_map(vh_context *c, const float pose[16], const vh_float4 *d_verts, const uint16_t *d_labels,
                                       float band, int32_t vote_max)
{
    VH_TRACE("vh_integrate_labels_map");
    if (!c || !pose || !d_verts || !d_labels) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return integrate_labels_impl(c, pose, vertex_depth(reinterpret_cast<const float4 *>(d_verts)), d_labels, band, vote_max);
}

extern "C" int vh_has_labels(vh_context *c) { return c && c->labels ? 1 : 0; }

extern "C" int vh_clear_labels(vh_context *c)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    DeviceGuard guard(c->device);
    VH_HIP(reset_labels(c));
    return VH_OK;
}

extern "C" int vh_download_labels(vh_context *c, size_t first_voxel, uint32_t *host_dst, size_t count)
{
    if (!c || !host_dst) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->labels) return fail(VH_ERR_INVALID_ARGUMENT, "the context has no label volume");
    if (first_voxel > label_words(c) || count > label_words(c) - first_voxel)
        return fail(VH_ERR_INVALID_ARGUMENT, "download past the end of the label volume");
    DeviceGuard guard(c->device);
    if (count) VH_HIP(hipMemcpyAsync(host_dst, c->labels.get() + first_voxel, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    return VH_OK;
}

static uint32_t label_min_votes(int32_t min_votes) { return (uint32_t)std::max<int32_t>(min_votes, 1); }

// ---------------------------------------------------------------------------
// reading labels
// ---------------------------------------------------------------------------
static int sample_labels_impl(vh_context *c, uint64_t n, ColorPoints in, int32_t min_votes, uint32_t *d_words_out)
{
    if (n > (uint64_t)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 points: sample in parts");
    if (n == 0) return VH_OK;
    if (!in.points || !d_words_out) return fail(VH_ERR_INVALID_ARGUMENT, "points need a point and a word buffer");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // behind every queued frame
    if (!c->labels || c->viewBlocks) {               // no volume (a view table's ptrs address records, which carry no labels)
        VH_HIP(hipMemsetAsync(d_words_out, 0, sizeof(uint32_t) * n, c->stream));
        return VH_OK;
    }
    const unsigned grid = (unsigned)grid_for((size_t)n, 256);
    hipLaunchKernelGGL(label_points_kernel, dim3(grid), dim3(256), 0, c->stream, c->fp, c->dp, (const uint32_t *)c->labels.get(),
                       label_min_votes(min_votes), (uint32_t)n, in, d_words_out);
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_sample_labels(vh_context *c, uint64_t n, const float *d_points, int32_t min_votes, uint32_t *d_words_out)
{
    VH_TRACE("vh_sample_labels");
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    ColorPoints in{};
    in.points = d_points;
    return sample_labels_impl(c, n, in, min_votes, d_words_out);
}

extern "C" int vh_sample_labels_map(vh_context *c, const float pose[16], uint64_t n, const vh_float4 *d_points, int32_t min_votes,
                                    uint32_t *d_words_out)
{
    VH_TRACE("vh_sample_labels_map");
    if (!c || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    ColorPoints in{};
    in.points = reinterpret_cast<const float *>(d_points);
    std::memcpy(in.T, pose, sizeof in.T);
    in.toWorld = 1;
    return sample_labels_impl(c, n, in, min_votes, d_words_out);
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade): device buffers for the call's
// lifetime, one copy each way.  Not a hot path.
extern "C" int vh_sample_labels_host(vh_context *c, uint64_t n, const float *h_points, int32_t min_votes, uint32_t *h_words_out)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (n == 0 || n > (uint64_t)INT32_MAX || !h_points || !h_words_out)
        return vh_sample_labels(c, n, h_points, min_votes, h_words_out);      // nothing to copy: its answer
    DeviceGuard guard(c->device);
    DevBuf<float> pts;
    DevBuf<uint32_t> words;
    int rc = pts.alloc(n * 3, "sample points");
    if (rc == VH_OK) rc = words.alloc(n, "sample labels");
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemcpyAsync(pts, h_points, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    rc = vh_sample_labels(c, n, pts, min_votes, words);
    if (rc != VH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    VH_HIP(hipMemcpyAsync(h_words_out, words, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));           // (before the device buffers go)
    return VH_OK;
}

// A composition, not a new traversal: vh_raycast_maps, then vh_sample_labels_map over its vertex map.
extern "C" int vh_raycast_labels(vh_context *c, const float pose[16], float t_min, float t_max, float *d_depth_out,
                                 vh_float4 *d_vertices_out, vh_float4 *d_normals_out, int32_t min_votes, uint32_t *d_words_out)
{
    VH_TRACE("vh_raycast_labels");
    if (!c || !pose || !d_depth_out || !d_vertices_out || !d_normals_out || !d_words_out)
        return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    const int rc = vh_raycast_maps(c, pose, t_min, t_max, d_depth_out, d_vertices_out, d_normals_out);
    if (rc != VH_OK) return rc;
    return vh_sample_labels_map(c, pose, (uint64_t)c->fp.width * (uint64_t)c->fp.height, d_vertices_out, min_votes, d_words_out);
}

// ---------------------------------------------------------------------------
// counting and removing
// ---------------------------------------------------------------------------
static bool label_region_empty(const BlockBox &rg)
{
    bool empty = false;
    for (int a = 0; a < 3; ++a) empty = empty || rg.lo[a] >= rg.hi[a];
    return empty;
}

// The ordered block list with the region as predicate, then one launch over it.  Launches only.
extern "C" int vh_label_counts(vh_context *c, const vh_mesh_region *region, int32_t min_votes, int32_t n_bins, uint32_t *d_counts)
{
    VH_TRACE("vh_label_counts");
    if (!c || !d_counts) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (n_bins < 1 || n_bins > 65536) return fail(VH_ERR_INVALID_ARGUMENT, "n_bins must be 1..65536");
    DeviceGuard guard(c->device);
    int rc = settle(c);                                 // the frames queued so far are part of the model
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)n_bins, c->stream));
    const BlockBox rg = block_box(region);
    if (label_region_empty(rg)) return VH_OK;
    BlockListScratch sc;
    if ((rc = block_list_reserve(c, sc)) != VH_OK) return rc;
    const FrameParams fp = c->fp;
    const DevPtrs dp = model_ptrs(c);
    if ((rc = list_blocks(c, fp, dp, rg, true, sc)) != VH_OK) return rc;
    const uint32_t *labels = c->viewBlocks ? nullptr : c->labels.get();      // (a view table's records carry no labels)
    const unsigned grid = (unsigned)std::min<size_t>(sc.listCapacity, 256);      // (few workgroups: each sums many blocks in LDS)
    hipLaunchKernelGGL(label_counts_kernel, dim3(grid), dim3(256), 0, c->stream, dp, labels, (const int4 *)sc.items,
                       (const unsigned long long *)sc.result, sc.listCapacity, label_min_votes(min_votes), (uint32_t)n_bins, d_counts);
    VH_HIP(hipGetLastError());
    return VH_OK;
}

// The same with a HOST buffer, for callers without a HIP runtime of their own (the C++ facade).  Not a hot path.
extern "C" int vh_label_counts_host(vh_context *c, const vh_mesh_region *region, int32_t min_votes, int32_t n_bins, uint32_t *h_counts)
{
    if (!c || !h_counts) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (n_bins < 1 || n_bins > 65536) return fail(VH_ERR_INVALID_ARGUMENT, "n_bins must be 1..65536");
    DeviceGuard guard(c->device);
    DevBuf<uint32_t> counts;
    int rc = counts.alloc((size_t)n_bins, "label counts");
    if (rc != VH_OK) return rc;
    rc = vh_label_counts(c, region, min_votes, n_bins, counts);
    if (rc != VH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    VH_HIP(hipMemcpyAsync(h_counts, counts, sizeof(uint32_t) * (size_t)n_bins, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));           // (before the device buffer goes)
    return VH_OK;
}

// The list, the clearing pass, one read-back; then the blocks that emptied go through vh_delete_blocks' path on their keys, in
// a lock epoch of its own (vh_remove_components' tail).
extern "C" int vh_remove_label(vh_context *c, const vh_mesh_region *region, int32_t label, int32_t min_votes, vh_label_stats *stats)
{
    VH_TRACE("vh_remove_label");
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    vh_label_stats st{};
    if (stats) *stats = st;
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    if (!c->labels) return fail(VH_ERR_INVALID_ARGUMENT, "the context has no label volume: there is no label to take out");
    if (label < 1 || label > 65535) return fail(VH_ERR_INVALID_ARGUMENT, "label must be 1..65535");
    DeviceGuard guard(c->device);
    int rc = settle(c);                                 // the frames queued so far are part of the model
    if (rc != VH_OK) return rc;
    const BlockBox rg = block_box(region);
    if (label_region_empty(rg)) return VH_OK;           // no block is listed
    BlockListScratch sc;
    if ((rc = block_list_reserve(c, sc)) != VH_OK) return rc;
    LabelScratch &ls = c->labelScratch;
    if ((rc = reserve_scratch(c, ls.keys, sc.listCapacity, "label key list")) != VH_OK) return rc;
    if ((rc = reserve_scratch(c, ls.words, (size_t)kLabelWords, "label counts")) != VH_OK) return rc;
    hipStream_t s = c->stream;
    VH_HIP(hipMemsetAsync(ls.words, 0, sizeof(unsigned long long) * kLabelWords, s));
    if ((rc = list_blocks(c, c->fp, c->dp, rg, true, sc)) != VH_OK) return rc;
    const unsigned grid = (unsigned)std::min<size_t>(sc.listCapacity, 8192);
    hipLaunchKernelGGL(label_remove_kernel, dim3(grid), dim3(256), 0, s, c->dp, c->color.get(), c->labels.get(), (const int4 *)sc.items,
                       (const unsigned long long *)sc.result, sc.listCapacity, (uint32_t)label, label_min_votes(min_votes),
                       ls.keys.get(), ls.words.get());
    VH_HIP(hipGetLastError());
    unsigned long long listed = 0, w[kLabelWords] = {};
    VH_HIP(hipMemcpyAsync(&listed, sc.result, sizeof listed, hipMemcpyDeviceToHost, s));
    VH_HIP(hipMemcpyAsync(w, ls.words, sizeof w, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    if ((rc = check_spin_timeouts(c)) != VH_OK) return rc;
    st.blocks = listed;
    st.removed_voxels = w[kLabelRemovedVoxels];
    st.freed_blocks = w[kLabelFreedBlocks];
    if (stats) *stats = st;
    if ((rc = vh_reset_mutexes(c)) != VH_OK) return rc;
    if (st.freed_blocks > 0) {
        rc = launch(c, kPhaseGc, gc_mark_keys_kernel, dim3((unsigned)grid_for((size_t)st.freed_blocks, 256)), dim3(256), c->fp, c->dp,
                    (const int4 *)ls.keys.get(), (int32_t)st.freed_blocks);
        if (rc != VH_OK) return rc;
    }
    if ((rc = sweep_and_release(c)) != VH_OK) return rc;
    VH_HIP(hipStreamSynchronize(c->stream));
    VH_HIP(hipGetLastError());
    return VH_OK;
}
