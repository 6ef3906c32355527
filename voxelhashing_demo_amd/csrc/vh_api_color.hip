// vh_api_color.hip -- C-ABI, the model in colour: vh_integrate_color*, vh_deintegrate_color and its compositions,
// vh_sample_color*, vh_raycast_color, vh_save_color / vh_load_color, the colour volume's housekeeping (kernels: vh_color.hip).  Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard,
// launch(), flush_pending(), vh_set_pose(), vh_flatten(), vh_raycast_maps()).
// The device calls only enqueue: no read-back, no synchronisation (the two file calls are host code and synchronise).  The one allocation is the colour volume itself, made and
// zeroed by the first colour-fusing call into a context and kept.

static size_t color_words(const vh_context *c) { return (size_t)c->params.numVoxelBlocks * kBlockVoxels; }

// The volume of the first colour-fusing call: all or nothing.
static int ensure_color(vh_context *c)
{
    if (c->color) return VH_OK;
    DevBuf<uint32_t> fresh;
    const int rc = fresh.alloc(color_words(c), "colour volume");
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemsetAsync(fresh, 0, sizeof(uint32_t) * color_words(c), c->stream));
    c->color = std::move(fresh);
    return VH_OK;
}

// vh_delete_blocks / vh_garbage_collect, ahead of gc_release_kernel: the freed blocks' colour words go back to zero
static int release_color(vh_context *c)
{
    if (!c->color) return VH_OK;
    return launch(c, kPhaseGc, color_release_kernel, dim3(1024), dim3(256), c->dp, c->color.get());
}

// vh_load_snapshot re-deals the ptrs and snapshots carry no colour: the volume, if there is one, starts over
static hipError_t reset_color(vh_context *c)
{
    if (!c->color) return hipSuccess;
    return hipMemsetAsync(c->color, 0, sizeof(uint32_t) * color_words(c), c->stream);
}

static int check_color_frame(const vh_context *c, float band, int32_t weight_max)
{
    if (!std::isfinite(band) || !(band > 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "band must be finite and positive");
    if (weight_max < 0 || weight_max > 255) return fail(VH_ERR_INVALID_ARGUMENT, "weight_max must be 0..255");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks: its voxels live in the caller's records");
    return VH_OK;
}

// pose -> the step-level flatten, called as it is -> one launch over the list it left (vh_api_deintegrate.hip's shape)
template <class Depth>
static int integrate_color_impl(vh_context *c, const float pose[16], const Depth &depth, const uint32_t *d_rgba, float band,
                                int32_t weight_max)
{
    int rc = check_color_frame(c, band, weight_max);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = ensure_color(c)) != VH_OK) return rc;  // (before anything changes)
    rc = flush_pending(c);                           // the frames queued so far are part of the model
    if (rc == VH_OK) rc = vh_set_pose(c, pose);
    if (rc == VH_OK) rc = vh_flatten(c, nullptr);    // (no occupied_out: the count stays on the device)
    if (rc != VH_OK) return rc;
    rc = launch(c, kPhaseIntegrate, color_integrate_kernel<Depth>, dim3((unsigned)c->integrateGrid), dim3(256), c->fp, c->dp, depth,
                c->color.get(), d_rgba, band, (uint32_t)weight_max);
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_integrate_color(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                                  const uint32_t *d_rgba, float band, int32_t weight_max)
{
    VH_TRACE("vh_integrate_color");
    if (!c || !pose || !d_depth || !k_inv || !d_rgba) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return integrate_color_impl(c, pose, DepthSensor{d_depth, k_inv[6], k_inv[7], k_inv[8], 5000.0f}, d_rgba, band, weight_max);
}

extern "C" int vh_integrate_color_map(vh_context *c, const float pose[16], const vh_float4 *d_verts, const uint32_t *d_rgba,
                                      float band, int32_t weight_max)
{
    VH_TRACE("vh_integrate_color_map");
    if (!c || !pose || !d_verts || !d_rgba) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return integrate_color_impl(c, pose, vertex_depth(reinterpret_cast<const float4 *>(d_verts)), d_rgba, band, weight_max);
}

// A composition: every refusal of the second half is met before the first half runs.
extern "C" int vh_integrate_depth_color(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                                        const uint32_t *d_rgba, float band, int32_t weight_max)
{
    VH_TRACE("vh_integrate_depth_color");
    if (!c || !pose || !d_depth || !k_inv || !d_rgba) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_color_frame(c, band, weight_max);
    if (rc != VH_OK) return rc;
    { DeviceGuard guard(c->device); if ((rc = ensure_color(c)) != VH_OK) return rc; }
    rc = vh_integrate_depth(c, pose, d_depth, k_inv);
    return rc != VH_OK ? rc : vh_integrate_color(c, pose, d_depth, k_inv, d_rgba, band, weight_max);
}

// ---------------------------------------------------------------------------
// taking a frame's colour back out
// ---------------------------------------------------------------------------
// integrate_color_impl's shape with the removal kernel; a context without a volume has nothing to remove
static int check_color_removal(const vh_context *c, float band, int32_t weight_max)
{
    const int rc = check_color_frame(c, band, weight_max);
    if (rc != VH_OK) return rc;
    if (!c->color) return fail(VH_ERR_INVALID_ARGUMENT, "the context has no colour volume: there is no colour to take out");
    return VH_OK;
}

extern "C" int vh_deintegrate_color(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                                    const uint32_t *d_rgba, float band)
{
    VH_TRACE("vh_deintegrate_color");
    if (!c || !pose || !d_depth || !k_inv || !d_rgba) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_color_removal(c, band, 0);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    rc = flush_pending(c);                           // the frames queued so far are part of the model
    if (rc == VH_OK) rc = vh_set_pose(c, pose);
    if (rc == VH_OK) rc = vh_flatten(c, nullptr);    // (no occupied_out: the count stays on the device)
    if (rc != VH_OK) return rc;
    rc = launch(c, kPhaseIntegrate, color_deintegrate_kernel<DepthSensor>, dim3((unsigned)c->integrateGrid), dim3(256), c->fp, c->dp,
                DepthSensor{d_depth, k_inv[6], k_inv[7], k_inv[8], 5000.0f}, c->color.get(), d_rgba, band);
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

// Compositions: every refusal of a later part is met before the first part runs.  Colour goes first -- it reads the TSDF
// weights and the band as the frame left them -- and the sweep of what the TSDF removal emptied goes last.
extern "C" int vh_deintegrate_depth_color(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                                          const uint32_t *d_rgba, float band)
{
    VH_TRACE("vh_deintegrate_depth_color");
    if (!c || !pose || !d_depth || !k_inv || !d_rgba) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_color_removal(c, band, 0);
    if (rc != VH_OK) return rc;
    rc = vh_deintegrate_color(c, pose, d_depth, k_inv, d_rgba, band);
    if (rc == VH_OK) rc = vh_deintegrate_depth(c, pose, d_depth, k_inv);
    return rc != VH_OK ? rc : vh_integrate_color(c, pose, d_depth, k_inv, d_rgba, band, 0);
}

extern "C" int vh_reintegrate_depth_color(vh_context *c, const float old_pose[16], const float new_pose[16], const uint16_t *d_depth,
                                          const float k_inv[9], const uint32_t *d_rgba, float band, int32_t weight_max)
{
    VH_TRACE("vh_reintegrate_depth_color");
    if (!c || !old_pose || !new_pose || !d_depth || !k_inv || !d_rgba) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_color_removal(c, band, weight_max);
    if (rc != VH_OK) return rc;
    rc = vh_deintegrate_depth_color(c, old_pose, d_depth, k_inv, d_rgba, band);
    return rc != VH_OK ? rc : vh_integrate_depth_color(c, new_pose, d_depth, k_inv, d_rgba, band, weight_max);
}

// ---------------------------------------------------------------------------
// colour beside a snapshot
// ---------------------------------------------------------------------------
// A file of its own: header, then {pos[3], 512 words} per allocated entry in table order.  The snapshot format stays as it is;
// the pairing is vh_load_snapshot (which clears the volume) followed by vh_load_color.
struct ColorFileHeader {
    char magic[8];                 // "VHCOLR01"
    uint64_t numEntries, numAllocated;
    uint32_t numVoxelBlocks, reserved;
};
struct ColorFileRecord {
    int32_t pos[3];
    uint32_t words[kBlockVoxels];
};

extern "C" int vh_save_color(vh_context *c, const char *path)
{
    if (!c || !path) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    if (!c->color) return fail(VH_ERR_INVALID_ARGUMENT, "the context has no colour volume");
    std::vector<VoxelEntry> table(c->numEntries);
    int rc = vh_download(c, VH_BUF_HASH_TABLE, table.data(), table.size() * sizeof(VoxelEntry));     // (synchronises)
    if (rc != VH_OK) return rc;
    ColorFileHeader h{};
    std::memcpy(h.magic, "VHCOLR01", 8);
    h.numEntries = c->numEntries;
    h.numVoxelBlocks = c->params.numVoxelBlocks;
    for (const VoxelEntry &e : table) h.numAllocated += e.ptr != VH_FREE_BLOCK;
    const std::string tmp = std::string(path) + ".partial";       // (renamed over the target at the end, as the snapshot is)
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(VH_ERR_INVALID_ARGUMENT, "cannot open the colour file");
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
    DeviceGuard guard(c->device);
    ColorFileRecord rec;
    for (const VoxelEntry &e : table) {
        if (e.ptr == VH_FREE_BLOCK || !ok) continue;
        std::memcpy(rec.pos, e.pos, sizeof rec.pos);
        if (hipMemcpy(rec.words, c->color.get() + e.ptr, sizeof rec.words, hipMemcpyDeviceToHost) != hipSuccess) { ok = false; break; }
        ok = std::fwrite(&rec, sizeof rec, 1, f) == 1;
    }
    ok = (std::fflush(f) == 0) && ok;
    ok = (std::fclose(f) == 0) && ok;
    if (ok) ok = std::rename(tmp.c_str(), path) == 0;
    if (!ok) {
        (void)std::remove(tmp.c_str());
        return fail(VH_ERR_HIP, "colour file write failed");
    }
    return VH_OK;
}

// Everything is validated on the host before a device byte changes: the header against this context, the file size, and the
// file's sequence of keys against the entries the context holds now, in table order.  Only the words are streamed afterwards;
// should reading them fail then (an I/O error after the size check), the volume is left cleared rather than half-loaded.
extern "C" int vh_load_color(vh_context *c, const char *path)
{
    if (!c || !path) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(VH_ERR_INVALID_ARGUMENT, "cannot open the colour file");
    struct Closer { FILE *f; ~Closer() { std::fclose(f); } } closer{f};
    ColorFileHeader h;
    if (std::fread(&h, sizeof h, 1, f) != 1 || std::memcmp(h.magic, "VHCOLR01", 8) != 0)
        return fail(VH_ERR_INVALID_ARGUMENT, "not a colour file");
    if (h.numEntries != c->numEntries || h.numVoxelBlocks != c->params.numVoxelBlocks)
        return fail(VH_ERR_INVALID_ARGUMENT, "colour file does not match this context");
    std::vector<VoxelEntry> table(c->numEntries);
    int rc = vh_download(c, VH_BUF_HASH_TABLE, table.data(), table.size() * sizeof(VoxelEntry));     // (synchronises)
    if (rc != VH_OK) return rc;
    std::vector<int32_t> ptrs;
    for (const VoxelEntry &e : table)
        if (e.ptr != VH_FREE_BLOCK) ptrs.push_back(e.ptr);
    if (h.numAllocated != ptrs.size()) return fail(VH_ERR_INVALID_ARGUMENT, "colour file belongs to another model: the block counts differ");
    if (std::fseek(f, 0, SEEK_END) != 0) return fail(VH_ERR_INVALID_ARGUMENT, "colour file is unreadable");
    const long file_end = std::ftell(f);
    if (file_end < 0 || (uint64_t)file_end != sizeof h + h.numAllocated * sizeof(ColorFileRecord))
        return fail(VH_ERR_INVALID_ARGUMENT, "colour file is truncated or has trailing bytes");
    size_t at = 0;
    for (const VoxelEntry &e : table) {
        if (e.ptr == VH_FREE_BLOCK) continue;
        int32_t pos[3];
        if (std::fseek(f, (long)(sizeof h + at * sizeof(ColorFileRecord)), SEEK_SET) != 0 || std::fread(pos, sizeof pos, 1, f) != 1)
            return fail(VH_ERR_INVALID_ARGUMENT, "colour file is unreadable");
        if (std::memcmp(pos, e.pos, sizeof pos) != 0)
            return fail(VH_ERR_INVALID_ARGUMENT, "colour file belongs to another model: its keys are not this table's");
        ++at;
    }
    if (std::fseek(f, (long)sizeof h, SEEK_SET) != 0) return fail(VH_ERR_INVALID_ARGUMENT, "colour file is unreadable");

    // ---- from here on the device state changes ----
    DeviceGuard guard(c->device);
    if ((rc = ensure_color(c)) != VH_OK) return rc;
    hipError_t e = reset_color(c);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    ColorFileRecord rec;
    bool ok = true;
    for (size_t i = 0; ok && e == hipSuccess && i < ptrs.size(); ++i) {
        ok = std::fread(&rec, sizeof rec, 1, f) == 1;
        if (ok) e = hipMemcpy(c->color.get() + ptrs[i], rec.words, sizeof rec.words, hipMemcpyHostToDevice);
    }
    if (!ok || e != hipSuccess) {
        (void)reset_color(c);                        // never leave a half-loaded volume behind
        (void)hipStreamSynchronize(c->stream);
        return !ok ? fail(VH_ERR_INVALID_ARGUMENT, "colour file could not be read; the colour volume was cleared")
                   : fail(VH_ERR_HIP, "colour upload failed; the colour volume was cleared", e);
    }
    return VH_OK;
}

extern "C" int vh_has_color(vh_context *c) { return c && c->color ? 1 : 0; }

extern "C" int vh_clear_color(vh_context *c)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    DeviceGuard guard(c->device);
    VH_HIP(reset_color(c));
    return VH_OK;
}

extern "C" int vh_download_color(vh_context *c, size_t first_voxel, uint32_t *host_dst, size_t count)
{
    if (!c || !host_dst) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->color) return fail(VH_ERR_INVALID_ARGUMENT, "the context has no colour volume");
    if (first_voxel > color_words(c) || count > color_words(c) - first_voxel)
        return fail(VH_ERR_INVALID_ARGUMENT, "download past the end of the colour volume");
    DeviceGuard guard(c->device);
    if (count) VH_HIP(hipMemcpyAsync(host_dst, c->color.get() + first_voxel, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    return VH_OK;
}

// ---------------------------------------------------------------------------
// reading colour
// ---------------------------------------------------------------------------
static int sample_color_impl(vh_context *c, int32_t mode, uint64_t n, ColorPoints in, uint32_t *d_rgba_out)
{
    if (mode != VH_SAMPLE_NEAREST && mode != VH_SAMPLE_TRILINEAR) return fail(VH_ERR_INVALID_ARGUMENT, "unknown sample mode");
    if (n > (uint64_t)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 points: sample in parts");
    if (n == 0) return VH_OK;
    if (!in.points || !d_rgba_out) return fail(VH_ERR_INVALID_ARGUMENT, "points need a point and a colour buffer");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // behind every queued frame
    if (!c->color || c->viewBlocks) {                // no volume (a view table's ptrs address records, which carry no colour)
        VH_HIP(hipMemsetAsync(d_rgba_out, 0, sizeof(uint32_t) * n, c->stream));
        return VH_OK;
    }
    const unsigned grid = (unsigned)grid_for((size_t)n, 256);
    hipLaunchKernelGGL(color_points_kernel, dim3(grid), dim3(256), 0, c->stream, c->fp, c->dp, (const uint32_t *)c->color.get(),
                       (int)mode, (uint32_t)n, in, d_rgba_out);
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_sample_color(vh_context *c, int32_t mode, uint64_t n, const float *d_points, uint32_t *d_rgba_out)
{
    VH_TRACE("vh_sample_color");
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    ColorPoints in{};
    in.points = d_points;
    return sample_color_impl(c, mode, n, in, d_rgba_out);
}

extern "C" int vh_sample_color_map(vh_context *c, int32_t mode, const float pose[16], uint64_t n, const vh_float4 *d_points,
                                   uint32_t *d_rgba_out)
{
    VH_TRACE("vh_sample_color_map");
    if (!c || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    ColorPoints in{};
    in.points = reinterpret_cast<const float *>(d_points);
    std::memcpy(in.T, pose, sizeof in.T);
    in.toWorld = 1;
    return sample_color_impl(c, mode, n, in, d_rgba_out);
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade): device buffers for the call's
// lifetime, one copy each way.  Not a hot path.
extern "C" int vh_sample_color_host(vh_context *c, int32_t mode, uint64_t n, const float *h_points, uint32_t *h_rgba_out)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (n == 0 || n > (uint64_t)INT32_MAX || !h_points || !h_rgba_out)
        return vh_sample_color(c, mode, n, h_points, h_rgba_out);             // nothing to copy: its answer
    DeviceGuard guard(c->device);
    DevBuf<float> pts;
    DevBuf<uint32_t> rgba;
    int rc = pts.alloc(n * 3, "sample points");
    if (rc == VH_OK) rc = rgba.alloc(n, "sample colours");
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemcpyAsync(pts, h_points, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    rc = vh_sample_color(c, mode, n, pts, rgba);
    if (rc != VH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    VH_HIP(hipMemcpyAsync(h_rgba_out, rgba, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));           // (before the device buffers go)
    return VH_OK;
}

// A composition, not a new traversal: vh_raycast_maps, then vh_sample_color_map over its vertex map.
extern "C" int vh_raycast_color(vh_context *c, const float pose[16], float t_min, float t_max, float *d_depth_out,
                                vh_float4 *d_vertices_out, vh_float4 *d_normals_out, int32_t mode, uint32_t *d_rgba_out)
{
    VH_TRACE("vh_raycast_color");
    if (!c || !pose || !d_depth_out || !d_vertices_out || !d_normals_out || !d_rgba_out)
        return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (mode != VH_SAMPLE_NEAREST && mode != VH_SAMPLE_TRILINEAR) return fail(VH_ERR_INVALID_ARGUMENT, "unknown sample mode");
    const int rc = vh_raycast_maps(c, pose, t_min, t_max, d_depth_out, d_vertices_out, d_normals_out);
    if (rc != VH_OK) return rc;
    return vh_sample_color_map(c, mode, pose, (uint64_t)c->fp.width * (uint64_t)c->fp.height, d_vertices_out, d_rgba_out);
}
