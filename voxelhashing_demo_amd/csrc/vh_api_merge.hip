// vh_api_merge.hip -- C-ABI, one model fused into another under a rigid transform: vh_merge, vh_merge_color (kernels:
// vh_merge.hip).  Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, launch(), flush_pending(),
// settle(), ensure_candidates(), invert4x4(), bin_parts(), ensure_color()).
// The call reads counters back between its allocation rounds and for its stats: it synchronises dst's stream.

// The candidate records a call is willing to hold: 2^24 of 16 bytes, 256 MiB of scratch.  A source block gives (about) 8 to 27
// records at equal voxel sizes, so this is a source model of some 600 k blocks; beyond it the call is refused before dst changes.
constexpr unsigned long long kMergeMaxRecords = 1ull << 24;

static int merge_read(vh_context *c, unsigned long long words[kMergeWords], int32_t *allocatedTotal)
{
    VH_HIP(hipMemcpyAsync(words, c->merge.words, sizeof(unsigned long long) * kMergeWords, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipMemcpyAsync(allocatedTotal, c->dp.counters + kAllocatedTotal, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    return VH_OK;
}

// The allocation rounds of one key bin of `records` records (vh_merge, vh_stream_in): the bin goes through the claim + commit path,
// one lock epoch per round, until nothing is missing or a round allocates nothing (buckets full, heap empty).  Every round that
// goes on has allocated a block, so the heap bounds the loop.  words[kMergeMissing]: the records still missing at the end.
static int bin_alloc_rounds(vh_context *dst, const int4 *bin, int32_t records, int32_t allocatedBefore,
                            unsigned long long words[kMergeWords], int32_t *allocatedNow, uint32_t *rounds)
{
    MergeScratch &ms = dst->merge;
    const int32_t capacity = records + 1;
    const unsigned scanGrid = (unsigned)std::min(grid_for((size_t)records, 256), 4096);
    int rc;
    for (;;) {
        if ((rc = vh_reset_mutexes(dst)) != VH_OK) return rc;
        rc = launch(dst, kPhaseClaim, claim_bins_kernel, dim3(bin_parts(capacity), 1), dim3(256), dst->fp, dst->dp,
                    (const int4 *)bin, capacity, capacity);
        if (rc == VH_OK) rc = launch(dst, kPhaseCommit, alloc_commit_kernel, dim3(32), dim3(256), dst->fp, dst->dp);
        if (rc != VH_OK) return rc;
        VH_HIP(hipMemsetAsync(ms.words.get() + kMergeMissing, 0, sizeof(unsigned long long), dst->stream));
        rc = launch(dst, kPhaseCommit, merge_missing_kernel, dim3(scanGrid), dim3(256), dst->fp, dst->dp, (const int4 *)bin, records,
                    ms.words.get());
        const int32_t allocatedLast = *rounds ? *allocatedNow : allocatedBefore;
        if (rc == VH_OK) rc = merge_read(dst, words, allocatedNow);
        if (rc != VH_OK) return rc;
        *rounds += 1;
        if (words[kMergeMissing] == 0 || *allocatedNow == allocatedLast) break;
    }
    return VH_OK;
}

// colorWeightMax == 0: vh_merge.  1..255: vh_merge_color -- the same call with the colour step in its update launch, where src
// has colour to give.
static int merge_impl(vh_context *dst, vh_context *src, const float src_to_dst[16], int32_t mode, int32_t colorWeightMax,
                      vh_merge_stats *stats)
{
    if (!dst || !src || !src_to_dst) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (src == dst) return fail(VH_ERR_INVALID_ARGUMENT, "a model cannot be merged into itself");
    if (src->device != dst->device) return fail(VH_ERR_INVALID_ARGUMENT, "the two contexts live on different devices");
    if (dst->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks: its voxels live in the caller's records");
    if (mode != VH_SAMPLE_NEAREST && mode != VH_SAMPLE_TRILINEAR) return fail(VH_ERR_INVALID_ARGUMENT, "unknown sample mode");
    float inverse[16];
    invert4x4(src_to_dst, inverse);                  // (vh_set_pose's routine)
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(src_to_dst[i]) || !std::isfinite(inverse[i]))
            return fail(VH_ERR_INVALID_ARGUMENT, "an entry of src_to_dst or of its inverse is not finite");
    MergeTransform T, Tinv;
    std::memcpy(T.m, src_to_dst, sizeof T.m);
    std::memcpy(Tinv.m, inverse, sizeof Tinv.m);
    vh_merge_stats st{};
    if (stats) *stats = st;

    DeviceGuard guard(dst->device);
    // a src without colour (a view table's records carry none) has none to give: the call is vh_merge
    const bool colored = colorWeightMax > 0 && src->color && !src->viewBlocks;
    int rc = colored ? ensure_color(dst) : VH_OK;    // (before anything else changes)
    if (rc != VH_OK) return rc;
    rc = flush_pending(src);                         // a pending pipelined frame of either context is part of its model
    if (rc == VH_OK) rc = settle(dst);
    if (rc != VH_OK) return rc;
    MergeScratch &ms = dst->merge;
    if (!ms.ordered) VH_HIP(hipEventCreateWithFlags(&ms.ordered, hipEventDisableTiming));
    if ((rc = ms.words.reserve(kMergeWords, "merge counts")) != VH_OK) return rc;
    // behind everything queued on src's stream; from here on everything runs on dst's
    VH_HIP(hipEventRecord(ms.ordered, src->stream));
    VH_HIP(hipStreamWaitEvent(dst->stream, ms.ordered, 0));

    // 1. candidates: counted, then written as one key bin
    const unsigned srcGrid = (unsigned)grid_for(src->numEntries, 256);
    const float vsSrc = src->fp.voxelSize, vsDst = dst->fp.voxelSize;
    unsigned long long words[kMergeWords];
    int32_t allocatedBefore = 0, allocatedNow = 0;
    VH_HIP(hipMemsetAsync(ms.words, 0, sizeof(unsigned long long) * kMergeWords, dst->stream));
    rc = launch(dst, kPhaseClaim, merge_keys_kernel, dim3(srcGrid), dim3(256), (const VoxelEntry *)src->dp.table,
                (uint32_t)src->numEntries, T, vsSrc, vsDst, ms.words.get(), (int4 *)nullptr, 0);
    if (rc == VH_OK) rc = merge_read(dst, words, &allocatedBefore);
    if (rc == VH_OK) rc = check_spin_timeouts(dst);
    if (rc != VH_OK) return rc;
    st.source_blocks = (uint32_t)words[kMergeSource];
    st.skipped_blocks = (uint32_t)words[kMergeSkipped];
    st.candidates = words[kMergeRecords];
    if (st.candidates == 0) {                        // an empty src, or one wholly outside the domain: nothing to do, nothing changed
        if (stats) *stats = st;
        return VH_OK;
    }
    if (st.candidates > kMergeMaxRecords)
        return fail(VH_ERR_OUT_OF_MEMORY, "more than 2^24 candidate block records: merge the source in parts (or at a coarser dst voxel size)");
    const int32_t records = (int32_t)st.candidates, capacity = records + 1;
    if ((rc = ms.bin.reserve((size_t)capacity, "merge candidate records")) != VH_OK) return rc;
    if ((rc = ensure_candidates(dst, (size_t)records)) != VH_OK) return rc;
    int4 *bin = ms.bin;
    VH_HIP(hipMemsetAsync(bin, 0, sizeof(int4), dst->stream));
    rc = launch(dst, kPhaseClaim, merge_keys_kernel, dim3(srcGrid), dim3(256), (const VoxelEntry *)src->dp.table,
                (uint32_t)src->numEntries, T, vsSrc, vsDst, ms.words.get(), bin, capacity);
    if (rc != VH_OK) return rc;

    // 2. allocation
    if ((rc = bin_alloc_rounds(dst, bin, records, allocatedBefore, words, &allocatedNow, &st.rounds)) != VH_OK) return rc;
    st.allocated = (uint32_t)(allocatedNow - allocatedBefore);
    st.unplaced = words[kMergeMissing];

    // 3. update: the distinct candidate blocks dst holds become its compact list (alloc_commit_kernel has zeroed the count), and
    // one launch in the TSDF update's shape runs over it
    const unsigned scanGrid = (unsigned)std::min(grid_for((size_t)records, 256), 4096);
    rc = launch(dst, kPhaseFlatten, merge_list_kernel, dim3(scanGrid), dim3(256), dst->fp, dst->dp, (const int4 *)bin, records);
    if (rc != VH_OK) return rc;
    dst->compactArmed = false;
    dst->occupiedCounter = kCompactCount;
    dst->foldA = -1;
    DevPtrs srcDp = model_ptrs(src);
    const dim3 grid((unsigned)dst->integrateGrid);
    if (colored) {
        uint32_t *dstColor = dst->color.get();
        const uint32_t *srcColor = src->color.get();
        const uint32_t cap = (uint32_t)colorWeightMax;
        rc = mode == VH_SAMPLE_NEAREST
                 ? launch(dst, kPhaseIntegrate, merge_color_update_kernel<kSampleNearest>, grid, dim3(256), dst->fp, dst->dp, dstColor,
                          src->fp, srcDp, srcColor, Tinv, cap)
                 : launch(dst, kPhaseIntegrate, merge_color_update_kernel<kSampleTrilinear>, grid, dim3(256), dst->fp, dst->dp, dstColor,
                          src->fp, srcDp, srcColor, Tinv, cap);
    } else {
        rc = mode == VH_SAMPLE_NEAREST
                 ? launch(dst, kPhaseIntegrate, merge_update_kernel<kSampleNearest>, grid, dim3(256), dst->fp, dst->dp, src->fp, srcDp, Tinv)
                 : launch(dst, kPhaseIntegrate, merge_update_kernel<kSampleTrilinear>, grid, dim3(256), dst->fp, dst->dp, src->fp, srcDp, Tinv);
    }
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemsetAsync(dst->dp.gcMarks, 0, sizeof(uint32_t) * ((dst->numEntries + 31) / 32), dst->stream));
    int32_t occupied = 0;
    VH_HIP(hipMemcpyAsync(&occupied, dst->dp.counters + kCompactCount, sizeof occupied, hipMemcpyDeviceToHost, dst->stream));
    VH_HIP(hipStreamSynchronize(dst->stream));
    VH_HIP(hipGetLastError());
    st.blocks = (uint32_t)occupied;
    dst->params.numOccupiedBlocks = (uint32_t)occupied;
    if (stats) *stats = st;
    return VH_OK;
}

extern "C" int vh_merge(vh_context *dst, vh_context *src, const float src_to_dst[16], int32_t mode, vh_merge_stats *stats)
{
    VH_TRACE("vh_merge");
    return merge_impl(dst, src, src_to_dst, mode, 0, stats);
}

extern "C" int vh_merge_color(vh_context *dst, vh_context *src, const float src_to_dst[16], int32_t mode, int32_t weight_max,
                              vh_merge_stats *stats)
{
    VH_TRACE("vh_merge_color");
    if (weight_max < 1 || weight_max > 255) return fail(VH_ERR_INVALID_ARGUMENT, "weight_max must be 1..255");
    return merge_impl(dst, src, src_to_dst, mode, weight_max, stats);
}
