// vh_api_stream.hip -- C-ABI, block streaming: vh_stream_out, vh_stream_in and their _host forms (kernels: vh_stream.hip).
// Included by vh_api.hip after everything else (same translation unit: shares fail(), VH_HIP, DeviceGuard, launch(), settle(),
// the block list and its scans, reserve_scratch(), sweep_and_release(), ensure_candidates(), bin_alloc_rounds(), ensure_color()).
// Both calls read counts back: they synchronise the context's stream.

// The records one vh_stream_in takes: 2^24 (64 GiB of voxels); beyond it the call is refused before anything changes.
constexpr unsigned long long kStreamMaxRecords = 1ull << 24;

static int stream_region(const vh_stream_region *region, float voxelSize, StreamSelect &rg)
{
    if (region->kind != VH_STREAM_BOX && region->kind != VH_STREAM_SPHERE) return fail(VH_ERR_INVALID_ARGUMENT, "unknown region kind");
    if (!std::isfinite(region->radius) || !(region->radius >= 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "radius must be finite and >= 0");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(region->centre[a])) return fail(VH_ERR_INVALID_ARGUMENT, "centre must be finite");
    rg.kind = region->kind;
    rg.invert = region->invert != 0;
    for (int a = 0; a < 3; ++a) {
        rg.box.lo[a] = region->block_lo[a];
        rg.box.hi[a] = region->block_hi[a];
        rg.centre[a] = region->centre[a];
    }
    rg.radius2 = region->radius * region->radius;        // (float32, rounded once: the rule's right-hand side)
    rg.voxelSize = voxelSize;
    return VH_OK;
}

extern "C" int vh_stream_out(vh_context *c, const vh_stream_region *region, uint64_t capacity, vh_view_record *d_records,
                             uint32_t *d_colors, uint64_t *selected_out, uint64_t *written_out)
{
    VH_TRACE("vh_stream_out");
    if (!c || !region || !selected_out || !written_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity > 0 && !d_records) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a record buffer");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    StreamSelect rg;
    int rc = stream_region(region, c->fp.voxelSize, rg);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = settle(c)) != VH_OK) return rc;          // the frames queued so far are part of the model

    // 1. the ordered block list with the region as predicate; the count-only call stops at its length
    hipStream_t s = c->stream;
    BlockListScratch sc;
    if ((rc = list_blocks(c, c->fp, c->dp, rg, capacity > 0, sc)) != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    unsigned long long selected = 0;
    VH_HIP(hipMemcpyAsync(&selected, sc.result, sizeof selected, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    if ((rc = check_spin_timeouts(c)) != VH_OK) return rc;
    const uint64_t written = std::min<uint64_t>(selected, capacity);       // (at most the list's capacity: the scan's total is capped)
    *selected_out = selected;
    *written_out = written;
    if (written == 0) return VH_OK;                    // the count-only call, or nothing to move: nothing changes

    // 2. the records, then 3. the removal: vh_delete_blocks on the listed keys (the list's records begin with the key)
    // (timed as view_export_ms when profiling is on: the record packing of this call)
    rc = launch(c, kPhaseViewExport, stream_pack_kernel, dim3((unsigned)std::min<uint64_t>(written, 2048)), dim3(256), c->dp,
                (const uint32_t *)c->color.get(), (const int4 *)sc.items, (uint32_t)written,
                reinterpret_cast<uint8_t *>(d_records), d_colors);
    if (rc != VH_OK) return rc;
    if ((rc = vh_reset_mutexes(c)) != VH_OK) return rc;
    rc = launch(c, kPhaseGc, gc_mark_keys_kernel, dim3((unsigned)grid_for((size_t)written, 256)), dim3(256), c->fp, c->dp,
                (const int4 *)sc.items, (int32_t)written);
    if (rc == VH_OK) rc = sweep_and_release(c);
    if (rc != VH_OK) return rc;
    VH_HIP(hipStreamSynchronize(s));
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_stream_in(vh_context *c, uint64_t n, const vh_view_record *d_records, const uint32_t *d_colors, int32_t *d_status,
                            vh_stream_stats *stats)
{
    VH_TRACE("vh_stream_in");
    if (!c || (n > 0 && !d_records)) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (n > kStreamMaxRecords) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^24 records: stream them in in parts");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    vh_stream_stats st{};
    if (stats) *stats = st;
    if (n == 0) return VH_OK;
    DeviceGuard guard(c->device);
    int rc = d_colors ? ensure_color(c) : VH_OK;      // (before anything else changes)
    if (rc == VH_OK) rc = settle(c);
    if (rc != VH_OK) return rc;
    StreamScratch &ss = c->streaming;
    MergeScratch &ms = c->merge;                       // the bin and the rounds' counts are vh_merge's
    if ((rc = reserve_scratch(c, ss.totals, 4, "stream totals")) != VH_OK) return rc;
    if (!d_status && (rc = reserve_scratch(c, ss.status, (size_t)n, "stream statuses")) != VH_OK) return rc;
    if ((rc = reserve_scratch(c, ms.words, kMergeWords, "merge counts")) != VH_OK) return rc;
    if ((rc = reserve_scratch(c, ms.bin, (size_t)n + 1, "stream key bin")) != VH_OK) return rc;
    int32_t *status = d_status ? d_status : ss.status.get();
    int4 *bin = ms.bin;
    const uint8_t *records = reinterpret_cast<const uint8_t *>(d_records);
    hipStream_t s = c->stream;

    // 1. classification: FOREIGN, PRESENT, or a record of the bin
    VH_HIP(hipMemsetAsync(ss.totals, 0, sizeof(unsigned long long) * 4, s));
    VH_HIP(hipMemsetAsync(bin, 0, sizeof(int4), s));
    hipLaunchKernelGGL(stream_classify_kernel, dim3((unsigned)grid_for((size_t)n, 256)), dim3(256), 0, s, c->fp, c->dp, records,
                       (uint32_t)n, status, bin);
    VH_HIP(hipGetLastError());
    int32_t pending = 0, allocatedBefore = 0, allocatedNow = 0;
    VH_HIP(hipMemcpyAsync(&pending, bin, sizeof pending, hipMemcpyDeviceToHost, s));
    VH_HIP(hipMemcpyAsync(&allocatedBefore, c->dp.counters + kAllocatedTotal, sizeof allocatedBefore, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    if ((rc = check_spin_timeouts(c)) != VH_OK) return rc;

    // 2. allocation: vh_merge's rounds over the bin
    if (pending > 0) {
        unsigned long long words[kMergeWords];
        if ((rc = ensure_candidates(c, (size_t)pending)) != VH_OK) return rc;
        if ((rc = bin_alloc_rounds(c, bin, pending, allocatedBefore, words, &allocatedNow, &st.rounds)) != VH_OK) return rc;
    }

    // 3. placement: one record per key takes the entry's mark bit and copies its block; the marks go back to zero, the compact
    // list is left empty (alloc_commit_kernel has zeroed the count when a round ran)
    // (timed as view_import_ms when profiling is on)
    rc = launch(c, kPhaseViewImport, stream_place_kernel, dim3((unsigned)std::min<uint64_t>(n, 2048)), dim3(256), c->fp, c->dp,
                c->color.get(), records, d_colors, (uint32_t)n, status, ss.totals.get());
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemsetAsync(c->dp.gcMarks, 0, sizeof(uint32_t) * ((c->numEntries + 31) / 32), s));
    VH_HIP(hipMemsetAsync(c->dp.counters + kCompactCount, 0, sizeof(int32_t), s));
    c->compactArmed = false;
    c->occupiedCounter = kCompactCount;
    c->foldA = -1;
    c->params.numOccupiedBlocks = 0;
    unsigned long long totals[4] = {0, 0, 0, 0};
    VH_HIP(hipMemcpyAsync(totals, ss.totals, sizeof totals, hipMemcpyDeviceToHost, s));
    VH_HIP(hipStreamSynchronize(s));
    VH_HIP(hipGetLastError());
    st.placed = totals[VH_STREAM_PLACED];
    st.present = totals[VH_STREAM_PRESENT];
    st.unplaced = totals[VH_STREAM_UNPLACED];
    st.foreign = totals[VH_STREAM_FOREIGN];
    if (stats) *stats = st;
    return VH_OK;
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade, a numpy store): device scratch the
// context keeps, one copy each way.
extern "C" int vh_stream_out_host(vh_context *c, const vh_stream_region *region, uint64_t capacity, vh_view_record *h_records,
                                  uint32_t *h_colors, uint64_t *selected_out, uint64_t *written_out)
{
    if (!c || !region || !selected_out || !written_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (capacity > 0 && !h_records) return fail(VH_ERR_INVALID_ARGUMENT, "a capacity needs a record buffer");
    int rc = vh_stream_out(c, region, 0, nullptr, nullptr, selected_out, written_out);       // the count sizes the scratch
    if (rc != VH_OK) return rc;
    const uint64_t want = std::min<uint64_t>(*selected_out, capacity);
    if (want == 0) return VH_OK;
    DeviceGuard guard(c->device);
    StreamScratch &ss = c->streaming;
    if ((rc = reserve_scratch(c, ss.records, (size_t)want * sizeof(vh_view_record), "stream records")) != VH_OK) return rc;
    if (h_colors && (rc = reserve_scratch(c, ss.colors, (size_t)want * kBlockVoxels, "stream colours")) != VH_OK) return rc;
    rc = vh_stream_out(c, region, want, reinterpret_cast<vh_view_record *>(ss.records.get()), h_colors ? ss.colors.get() : nullptr,
                       selected_out, written_out);
    if (rc != VH_OK) return rc;
    const size_t got = (size_t)*written_out;
    if (got) {
        VH_HIP(hipMemcpy(h_records, ss.records, got * sizeof(vh_view_record), hipMemcpyDeviceToHost));
        if (h_colors) VH_HIP(hipMemcpy(h_colors, ss.colors, got * kBlockVoxels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return VH_OK;
}

extern "C" int vh_stream_in_host(vh_context *c, uint64_t n, const vh_view_record *h_records, const uint32_t *h_colors,
                                 int32_t *h_status, vh_stream_stats *stats)
{
    if (!c || (n > 0 && !h_records)) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (n > kStreamMaxRecords) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^24 records: stream them in in parts");
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks");
    if (n == 0) return vh_stream_in(c, 0, nullptr, nullptr, nullptr, stats);
    DeviceGuard guard(c->device);
    StreamScratch &ss = c->streaming;
    int rc;
    if ((rc = reserve_scratch(c, ss.records, (size_t)n * sizeof(vh_view_record), "stream records")) != VH_OK) return rc;
    if (h_colors && (rc = reserve_scratch(c, ss.colors, (size_t)n * kBlockVoxels, "stream colours")) != VH_OK) return rc;
    if (h_status && (rc = reserve_scratch(c, ss.hostStatus, (size_t)n, "stream statuses")) != VH_OK) return rc;
    VH_HIP(hipMemcpyAsync(ss.records, h_records, (size_t)n * sizeof(vh_view_record), hipMemcpyHostToDevice, c->stream));
    if (h_colors) VH_HIP(hipMemcpyAsync(ss.colors, h_colors, (size_t)n * kBlockVoxels * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    rc = vh_stream_in(c, n, reinterpret_cast<const vh_view_record *>(ss.records.get()), h_colors ? ss.colors.get() : nullptr,
                      h_status ? ss.hostStatus.get() : nullptr, stats);
    if (rc != VH_OK) return rc;
    if (h_status) VH_HIP(hipMemcpy(h_status, ss.hostStatus, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VH_OK;
}
