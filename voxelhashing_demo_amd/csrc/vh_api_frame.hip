// vh_api_frame.hip -- C-ABI, the frame: step-level entry points, the fused frame, raycast, block silhouettes.
// Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, launch()).

// ---------------------------------------------------------------------------
// per-frame steps
// ---------------------------------------------------------------------------
extern "C" int vh_reset_mutexes(vh_context *c)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    // The reference memsets 4*numBuckets bytes every frame (VoxelUtils.cu:146-149).  Claim words carry
    // the epoch in their top 10 bits, so starting a new epoch invalidates every lock at once.  After
    // kMaxClaimEpoch epochs the words are cleared for real and the epoch restarts at 1.
    if (c->fp.epoch >= kMaxClaimEpoch) {
        DeviceGuard guard(c->device);
        const int rc = flush_pending(c);
        if (rc != VH_OK) return rc;
        const size_t bytes = sizeof(unsigned long long) * (size_t)c->ownedBuckets;
        if (c->claimBuf[0]) {
            VH_HIP(hipMemsetAsync(c->claimBuf[0], 0, bytes, c->stream));
            VH_HIP(hipMemsetAsync(c->claimBuf[1], 0, bytes, c->stream));
        } else {
            VH_HIP(hipMemsetAsync(c->dp.claim, 0, bytes, c->stream));
        }
        c->fp.epoch = 0;
    }
    c->fp.epoch += 1;
    c->epochTotal += 1;
    return VH_OK;
}

static inline int grid_for(size_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }
// 16x16 launch tiles of the depth image (one claim workgroup each, vh_alloc.hip)
static inline uint32_t host_num_tiles(const vh_context *c)
{
    return (uint32_t)((c->fp.width + 15) / 16) * (uint32_t)((c->fp.height + 15) / 16);
}

// Profiling: a start/stop event pair per dispatch, taken from a pool that vh_get_kernel_times (and
// accumulate_times below) refill; a profiled run of any length keeps at most kMaxTimedLaunches
// pairs alive (at that point the stream is synchronised once and the pending pairs are folded
// into the totals).
constexpr size_t kMaxTimedLaunches = 8192;
static int accumulate_times(vh_context *c);

// (-Wpsabi: the pipelined launch hands on a 64-byte vector by value, vh_frame.hip: PipeLeadWords)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpsabi"
template <typename K, typename... Args>
static int launch(vh_context *c, int phase, K kernel, dim3 grid, dim3 block, Args... args)
{
    if (!c->profiling) {
        hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, args...);
        return VH_OK;
    }
    if (c->timed.size() >= kMaxTimedLaunches) {
        const int rc = accumulate_times(c);
        if (rc != VH_OK) return rc;
    }
    TimedLaunch t{phase, nullptr, nullptr};
    if (!c->eventPool.empty()) {
        t.start = c->eventPool.back().first;
        t.stop = c->eventPool.back().second;
        c->eventPool.pop_back();
    } else {
        VH_HIP(hipEventCreate(&t.start));
        const hipError_t e = hipEventCreate(&t.stop);
        if (e != hipSuccess) {
            (void)hipEventDestroy(t.start);
            return fail(VH_ERR_HIP, "hipEventCreate", e);
        }
    }
    hipExtLaunchKernelGGL(kernel, grid, block, 0, c->stream, t.start, t.stop, 0, args...);
    c->timed.push_back(t);
    return VH_OK;
}
#pragma clang diagnostic pop

template <class In>
static int launch_alloc(vh_context *c, const In &in)
{
    int rc = launch(c, kPhaseClaim, alloc_claim_kernel<In>, dim3(host_num_tiles(c)), dim3(256), c->fp, c->dp, in);
    if (rc != VH_OK) return rc;
    rc = launch(c, kPhaseCommit, alloc_commit_kernel, dim3(32), dim3(256), c->fp, c->dp);
    c->compactArmed = (rc == VH_OK);
    return rc;
}

// workgroups of the table walk: 2048 entries each
static uint32_t walk_blocks(const vh_context *c)
{
    if (c->flattenVariant == kWalkIndexed)       // one lane per 32-bucket word of the occupancy bitmap
        return (uint32_t)grid_for(((size_t)c->ownedBuckets + 31) / 32, kFlattenThreads * kIndexWords);
    return (uint32_t)grid_for(c->numEntries, kFlattenThreads * ((c->fp.flags & kFlagWalkShort) ? kEntriesPerLaneShort : kEntriesPerLane));
}

// The reference's walk in the single-camera launches: its ordinals run over groups of 8 workgroups (the tiles rounded up to a
// multiple of 8; vh_walk.hip: walk_tile), and its direction alternates from one launch that carries it to the next, in every
// context (option "walk_reverse" 1, the default; 0: always forward).
static inline uint32_t groups_of_8(uint32_t n) { return (n + 7u) / 8u; }
static uint32_t take_walk_direction(vh_context *c)
{
    const uint32_t reverse = c->walkReverse ? c->walkBackward : 0u;
    c->walkBackward ^= 1u;
    return reverse;
}

// ... of the multi-camera walk: the reference's walk with 4 entries per lane from 32 MB of entries on, else 8; the index walk
// for flatten_variant 4 without the overflow list (holes and chains take the reference's walk)
static bool multi_walk_indexed(const vh_context *c) { return c->flattenVariant == kWalkIndexed && !(c->fp.flags & kFlagOverflow); }
static bool multi_walk_short(const vh_context *c) { return c->numEntries * sizeof(VoxelEntry) >= ((size_t)32 << 20); }
static uint32_t multi_walk_blocks(const vh_context *c)
{
    return multi_walk_indexed(c) ? (uint32_t)grid_for(((size_t)c->ownedBuckets + 31) / 32, kFlattenThreads * kIndexWords)
                                 : (uint32_t)grid_for(c->numEntries, kFlattenThreads * (multi_walk_short(c) ? kEntriesPerLaneShort : kEntriesPerLane));
}

// 1024-record slices of a key bin of `capacity` records (one claim workgroup each, vh_shard.hip: claim_bin_slice)
static uint32_t bin_parts(int32_t capacity) { return (uint32_t)std::max(1, grid_for((size_t)capacity, 256 * 4)); }

// a run-time bool as a template argument: f(std::true_type / std::false_type)
template <class F>
static int with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

static int launch_flatten(vh_context *c)
{
    if (c->flattenVariant == kWalkIndexed)
        return launch(c, kPhaseFlatten, flatten_kernel<kWalkIndexed>, dim3(walk_blocks(c)), dim3(kFlattenThreads), c->fp, c->dp,
                      (uint32_t)c->numEntries, 0u);
    return launch(c, kPhaseFlatten, flatten_kernel<kWalkStridedBallot>, dim3(8u * groups_of_8(walk_blocks(c))), dim3(kFlattenThreads),
                  c->fp, c->dp, (uint32_t)c->numEntries, take_walk_direction(c));
}

template <class Depth>
static int launch_integrate(vh_context *c, const Depth &depth)
{
    return launch(c, kPhaseIntegrate, integrate_kernel<Depth>, dim3(c->integrateGrid), dim3(256), c->fp, c->dp, depth);
}

extern "C" int vh_alloc_blocks(vh_context *c, const vh_float4 *verts, const vh_float4 *normals)
{
    // normals: loaded into a dead variable by the reference (VoxelUtils.cu:631); read only by the DDA band
    if (!c || !verts) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (c->epochTotal == 0) return fail(VH_ERR_INVALID_ARGUMENT, "vh_reset_mutexes must start the frame");
    if ((c->fp.flags & kFlagOverflow) && c->allocEpoch == c->epochTotal)
        return fail(VH_ERR_INVALID_ARGUMENT, "with the overflow list on, allocBlocks runs once per lock epoch "
                                             "(several cameras: vh_insert_bins / vh_apply_frames_batch)");
    c->allocEpoch = c->epochTotal;
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }
    { const int brc = ensure_band_candidates(c); if (brc != VH_OK) return brc; }
    int rc = launch_alloc(c, VertexMap{reinterpret_cast<const float4 *>(verts), reinterpret_cast<const float4 *>(normals)});
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_flatten(vh_context *c, int32_t *occupied_out)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }
    if (!c->compactArmed)
        VH_HIP(hipMemsetAsync(c->dp.counters + kCompactCount, 0, sizeof(int32_t), c->stream));   // :760
    c->compactArmed = false;
    c->occupiedCounter = kCompactCount;
    c->foldA = -1;                                   // (the step kernel writes one dense list)
    int rc = launch_flatten(c);
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    if (occupied_out) {
        int32_t n = 0;
        VH_HIP(hipMemcpyAsync(&n, c->dp.counters + kCompactCount, sizeof n, hipMemcpyDeviceToHost, c->stream));
        VH_HIP(hipStreamSynchronize(c->stream));                                               // :765
        *occupied_out = n;
        c->params.numOccupiedBlocks = (uint32_t)n;
    }
    return VH_OK;
}

extern "C" int vh_integrate_depth_map(vh_context *c, const vh_float4 *verts)
{
    if (!c || !verts) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    DeviceGuard guard(c->device);
    { const int frc = settle(c); if (frc != VH_OK) return frc; }
    int rc = launch_integrate(c, vertex_depth(reinterpret_cast<const float4 *>(verts)));
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

// How many of the claim + walk workgroups of a launch the claim tiles are spread over.  A claim workgroup is
// a chain of dependent reads (vertex -> bucket -> claim word) of about 4 us; interleaved uniformly over the
// whole grid, the ones dispatched last are the tail of the launch.  Ending them early by the share that
// chain has of the launch (estimated from the table bytes the walk streams at ~6 TB/s) removes the tail;
// squeezing them further starves the stream.  In-process A/B of the pipelined launch (4 entries per lane in
// the walk): C2 19.5 us uniform, 18.6 by this rule (77 %), 18.9 at 65 % or 85 %; C2 with band allocation (a
// claim tile then runs ~12 us) 29.0 uniform, 26.2 at 70 %, 24.3 at 50 %, 24.6 at 40 %, 26.6 at 30 %; C3, a
// 72 us launch: 72.5 uniform, 72.2 by the rule (94 %).
static uint32_t claim_span(const vh_context *c, uint32_t claimBlocks, uint32_t walkBlocks)
{
    const uint32_t total = claimBlocks + walkBlocks;
    const double walk_us = (double)c->numEntries * sizeof(VoxelEntry) / 6.0e6;     // bytes / (6 TB/s) in us
    // with band allocation a pixel demands several keys: ~2 us more per sample
    double chain_us = 4.0;
    if (c->fp.allocBand > 0.0f)
        chain_us += 2.0 * std::min(8.0, 2.0 * std::ceil((double)c->fp.allocBand / (4.0 * c->fp.voxelSize)));
    const double share = std::min(1.0, std::max(0.5, 1.0 - chain_us / std::max(walk_us, 1.0)));
    // (strictly more workgroups than claim tiles whenever there is a walk: claim_ratio below must stay < 2^32)
    return std::min(total, std::max<uint32_t>(claimBlocks + (walkBlocks ? 1u : 0u), (uint32_t)(share * total)));
}

// How many groups of walk workgroups run ahead of the claim window (vh_frame.hip: grouped_role).  With the alternating sweep
// the first walk groups of a launch read what their XCD's 4 MiB L2 still holds of the previous sweep, and the claim tiles'
// traffic among them takes part of that away: in process the reversal is worth 2.6 us to C2's walk alone and 1.5 us to the
// whole launch (profiles/pipelined_roles_reverse_C2.txt).  So the claim window starts behind the groups whose tiles fill
// the eight L2s once (4 MiB / 20 bytes / 1024 or 2048 entries a tile: 204 or 102 groups), at most a quarter of the walk, and
// keeps its end.  Same process, launch us by lead in groups -- C2 (640 walk groups): 0 17.94, 64 17.11, 128 16.67, 192 16.65,
// 256 16.93, 320 17.33, 400 17.64; C3 (2 560): 0 67.92, 128 67.76, 256 67.53, 512 67.86, 768 68.35, 1 024 69.26.  The rule
// itself, another session (profiles/claim_lead_ab.txt): C2 17.52 -> 16.33 (160 groups; 128, 160 and 192 within one spread of
// each other), C3 68.14 -> 67.81 (204 groups: twice the spread of its rounds).  The quarter is a cap for small tables, not a
// measured optimum: C2 is the one workload it binds on.  The window's END moving out with the lead loses most of the gain
// (an earlier session, C2, lead 128: 17.40 -> 16.88, against 16.22 with the end kept).
// Option "claim_lead" >= 0: that many groups; -1 (default): this rule in the pipelined launch without band allocation, else
// none (the two-launch frame and the loaded frame are not measured with a lead).
static uint32_t claim_lead(const vh_context *c, uint32_t claimGroups, uint32_t walkGroups, uint32_t &span, bool pipelined)
{
    uint32_t want = 0u;
    if (c->claimLead >= 0) want = (uint32_t)c->claimLead;
    else if (pipelined && !(c->fp.allocBand > 0.0f)) {
        const size_t tileBytes = sizeof(VoxelEntry) * kFlattenThreads * ((c->fp.flags & kFlagWalkShort) ? kEntriesPerLaneShort : kEntriesPerLane);
        want = std::min<uint32_t>((uint32_t)(((size_t)4 << 20) / tileBytes), walkGroups / 4u);
    }
    // the window keeps the end claim_span gave it and starts `lead` groups in: span shrinks by the lead, and strictly more
    // groups than claim groups stay in it (claim_ratio < 2^32)
    const uint32_t least = claimGroups + (walkGroups ? 1u : 0u);
    const uint32_t lead = span > least ? std::min(want, span - least) : 0u;
    span -= lead;
    return lead;
}

// ceil(claimBlocks * 2^32 / span): floor(r * ratio / 2^32) steps from 0 to claimBlocks in unit steps over r = 0 .. span
static uint32_t claim_ratio(uint32_t claimBlocks, uint32_t span)
{
    if (span == 0 || claimBlocks >= span) return 0xffffffffu;       // (no walk workgroups: every workgroup claims; see callers)
    return (uint32_t)((((uint64_t)claimBlocks << 32) + span - 1) / span);
}

// ---------------------------------------------------------------------------
// pipelined frames (vh_frame.hip: frame_pipelined_kernel)
// ---------------------------------------------------------------------------
// second claim array / candidate list / compact list and the private depth copies, on first use
static int ensure_pipeline_buffers(vh_context *c)
{
    if (c->claimBuf[1]) return VH_OK;
    const size_t npix = (size_t)c->fp.width * c->fp.height;
    const size_t claimBytes = sizeof(unsigned long long) * (size_t)c->ownedBuckets;
    // all or nothing: allocated into locals, which free themselves on any early return; the context is written from the commit on
    DevBuf<unsigned long long> claim2;
    DevBuf<int4> cand2;
    DevBuf<VoxelEntry> compact2;
    DevBuf<uint32_t> filter;
    DevBuf<float> plane[2];
    DevBuf<uint16_t> raw[2];
    int rc;
    if ((rc = claim2.alloc(c->ownedBuckets, "pipeline buffers")) || (rc = cand2.alloc(c->candAllocated, "pipeline buffers")) ||
        (rc = compact2.alloc(c->numEntries, "pipeline buffers")) ||
        (rc = plane[0].alloc(npix, "pipeline buffers")) || (rc = raw[0].alloc(npix, "pipeline buffers")) ||
        (rc = plane[1].alloc(npix, "pipeline buffers")) || (rc = raw[1].alloc(npix, "pipeline buffers")))
        return rc;
    VH_HIP(hipMemsetAsync(claim2, 0, claimBytes, c->stream));
    if ((rc = filter.alloc(3 * kPendFilterWords, "pipeline buffers")) != VH_OK) return rc;
    VH_HIP(hipMemsetAsync(filter, 0, sizeof(uint32_t) * 3 * kPendFilterWords, c->stream));
    // commit
    c->claim[1] = std::move(claim2);
    c->candidates[1] = std::move(cand2);
    c->compact[1] = std::move(compact2);
    for (int i = 0; i < 2; ++i) { c->planeBuf[i] = std::move(plane[i]); c->rawBuf[i] = std::move(raw[i]); }
    c->claimFilter = std::move(filter);
    c->claimBuf[0] = c->dp.claim;          c->claimBuf[1] = c->claim[1];
    c->candBuf[0] = c->dp.candidates;      c->candBuf[1] = c->candidates[1];
    c->compactBuf[0] = c->dp.compact;      c->compactBuf[1] = c->compact[1];
    c->pipeParity = 0;                     // dp.* currently alias set 0
    return VH_OK;
}

static DevPtrs pipe_view(const vh_context *c, int parity)
{
    DevPtrs d = c->dp;
    d.claim = c->claimBuf[parity];
    d.candidates = c->candBuf[parity];
    d.compact = c->compactBuf[parity];
    return d;
}

// With the overflow list a one-launch frame is serialised inside the launch: every claim / walk workgroup of frame i+1 waits
// for commit(i) and then ACQUIRES -- a cache invalidate (buffer_inv sc1), which this chip serves one at a time.  Measured in
// round 4 on C2 (6 320 such workgroups per launch, profiles/r04_ab_overflow_serial.txt): 185 us per launch with the
// invalidate in every wave, 53 us with one per workgroup (wait_commit_done), against 16.4 + 4.6 us for the two-launch frame
// -- ~5.5 ns per waiting workgroup against ~3 us for a second launch.  So the serialised form is taken only where it is the
// cheaper one: up to kSerialMaxWaiters waiting workgroups (option "pipeline_overflow" 1, the default; 0 never, 2 always).
constexpr uint32_t kSerialMaxWaiters = 512;
static bool serial_launch_pays(const vh_context *c, uint32_t waiters)
{
    if (!(c->fp.flags & kFlagOverflow)) return true;
    if (c->serialFallback || c->pipelineOverflow == 0) return false;
    return c->pipelineOverflow == 2 || waiters <= kSerialMaxWaiters;
}

// can this context run one-launch frames (single- or multi-camera) whose claim + walk roles have `waiters` workgroups?
static bool can_pipeline(const vh_context *c, uint32_t waiters)
{
    return c->fp.bucketSize <= kMaxPipelinedBucket && !c->viewBlocks && serial_launch_pays(c, waiters);
}

// ... its single-camera frames, right now?
static bool pipeline_applies(const vh_context *c)
{
    return c->pipeline && c->fusedFrame && (c->flattenVariant == kWalkStridedBallot || c->flattenVariant == kWalkIndexed) &&
           can_pipeline(c, host_num_tiles(c) + walk_blocks(c));
}

// What a pipelined launch works on.  Buffers alternate and counter sets rotate from frame to frame -- single- and multi-camera
// frames alike, across flushes too (a flush leaves the two sets it did not consume empty; at creation all three are).
struct PipeRotation {
    int oldParity, newParity;          // buffer sets of the pending frame and of the new one
    int iNew, iOld, iClear;            // counter sets (0..2): filled by the new frame (c->pipeSet once it is pending), consumed, cleared by this launch
    DevPtrs dpOld, dpNew;
};
// ... and its part of the launch's argument block (PipeArgs / MultiPipeArgs); which frames the launch carries goes where the
// kernel reads it: `lead` is the single-camera launch's PipeLead, the multi-camera launch's MultiPipeArgs itself
template <class Args, class Lead>
static PipeRotation pipe_rotation(const vh_context *c, Args &a, Lead &lead, bool hasNew, bool hasOld)
{
    PipeRotation r;
    r.oldParity = c->pipeParity; r.newParity = r.oldParity ^ 1;
    r.iOld = c->pipeSet; r.iNew = (r.iOld + 1) % 3; r.iClear = (r.iNew + 1) % 3;
    r.dpNew = pipe_view(c, r.newParity); r.dpOld = pipe_view(c, r.oldParity);
    a.setNew = kPipeSetStride * r.iNew; a.setOld = kPipeSetStride * r.iOld; a.setClear = kPipeSetStride * r.iClear;
    lead.hasNew = hasNew; lead.hasOld = hasOld;
    a.doneTag = c->pend.doneTag;
    a.spinLimit = c->spinLimit ? c->spinLimit : kSpinLimitDefault;
    return r;
}

// What follows a successful pipelined launch.  kind: of the frame it started (kNone: a flush launch; the caller fills in what that
// kind keeps).  twoEnded: the consumed frame's list has two ends to fold (single-camera; the multi-camera list is dense).
static void pipe_launched(vh_context *c, const PipeRotation &r, bool serial, PendingFrame::Kind kind, bool hasOld, bool twoEnded, bool countFrame)
{
    if (serial && kind != PendingFrame::kNone && hasOld) c->serialQueued = true;       // (its claim / walk workgroups wait: check_spin_timeouts)
    if (!twoEnded) c->foldA = -1;
    else if (hasOld) { const int set = kPipeSetStride * r.iOld; c->foldA = kPipeScan + set; c->foldB = kPipeScanB + set; c->foldNew = kPipeNew + set; }
    c->pend.kind = kind;               // (kNone: pipeSet / pipeParity stay, the next run starts on the following set)
    if (kind != PendingFrame::kNone) {
        c->pend.doneTag = (int32_t)(c->epochTotal & 0x7fffffffu) | 0x40000000;      // (never 0, the counter's initial value)
        c->pipeSet = r.iNew;
        c->pipeParity = r.newParity;
        c->dp.claim = r.dpNew.claim;             // the "current" buffers of everything that is not pipelined
        c->dp.candidates = r.dpNew.candidates;
        c->dp.compact = r.dpNew.compact;
    }
    c->occupiedCounter = kCompactCount;
    c->compactArmed = false;
    if (countFrame && c->profiling) c->profiledFrames += 1;
}

// The build of frame_pipelined_kernel for this context's state (vh_frame.hip: kLean*): a lean one when there is no overflow list
// and both frames' option flags, the walk and the claim form are exactly what that build has folded in.
static int lean_for(const vh_context *c, uint32_t flagsOld, bool band, bool indexed, bool claimPerWave)
{
    if (c->fp.flags & kFlagOverflow) return kLeanNone;
    for (int k = kLeanShort; k < kLeanBuilds; ++k) {
        const LeanBuild lb = lean_build(k);
        const bool rayDda = (lb.flags & kFlagBandRayDda) != 0u;
        if (lb.flags == c->fp.flags && lb.flags == flagsOld && lb.indexed == indexed && lb.claimPerWave == claimPerWave &&
            (!rayDda || band) && (!lb.indexed || !band))          // (the ray-DDA builds exist with the band only, the walk-free ones without)
            return k;
    }
    return kLeanNone;
}

// run-time (lean, band, serial) -> the instantiation.  Only the builds named here exist.
template <int kLean>
using LeanC = std::integral_constant<int, kLean>;
template <class In, class Depth, class... Args>
static int launch_pipelined_build(vh_context *c, int lean, bool band, bool serial, dim3 grid, Args... args)
{
    using Yes = std::true_type;
    using No = std::false_type;
    auto go = [&](auto leanC, auto bandC, auto serialC) {
        return launch(c, kPhaseFramePipelined, frame_pipelined_kernel<In, Depth, decltype(bandC)::value, decltype(serialC)::value, decltype(leanC)::value>,
                      grid, dim3(256), args...);
    };
    switch (lean) {
    case kLeanShort: return with_bool(band, [&](auto b) { return go(LeanC<kLeanShort>{}, b, No{}); });
    case kLeanShortNt: return with_bool(band, [&](auto b) { return go(LeanC<kLeanShortNt>{}, b, No{}); });
    case kLeanRayDda: return go(LeanC<kLeanRayDda>{}, Yes{}, No{});
    case kLeanRayDdaNt: return go(LeanC<kLeanRayDdaNt>{}, Yes{}, No{});
    case kLeanIndexed: return go(LeanC<kLeanIndexed>{}, No{}, No{});
    case kLeanIndexedNt: return go(LeanC<kLeanIndexedNt>{}, No{}, No{});
    case kLeanIndexedWave: return go(LeanC<kLeanIndexedWave>{}, No{}, No{});
    case kLeanIndexedWaveNt: return go(LeanC<kLeanIndexedWaveNt>{}, No{}, No{});
    default: return with_bool(band, [&](auto b) { return with_bool(serial, [&](auto q) { return go(LeanC<kLeanNone>{}, b, q); }); });
    }
}

// One launch: {claim || walk} of the new frame (in != nullptr) and {commit + integrate} of the pending one.
template <class In>
static int launch_pipelined(vh_context *c, const In *in, int newSensor, const float newK[4])
{
    const bool hasNew = in != nullptr, hasOld = c->pend.kind == PendingFrame::kSingle;
    if (!hasNew && !hasOld) return VH_OK;
    int rc;
    if (!hasOld && (rc = ensure_pipeline_buffers(c)) != VH_OK) return rc;
    PipeArgs args;
    PipeLead a{};                                   // the leading piece: role map and the walk's two values (vh_frame.hip)
    const PipeRotation r = pipe_rotation(c, args, a, hasNew, hasOld);
    a.table = r.dpNew.table;
    const bool band = c->fp.allocBand > 0.0f;       // (the new frame's; the pending frame's claims are done)
    a.walkBlocks = hasNew ? walk_blocks(c) : 0u;
    a.walkIndexed = c->flattenVariant == kWalkIndexed ? 1u : 0u;
    const bool serial = (c->fp.flags & kFlagOverflow) != 0u;
    // The walk-free frame of a large image: a claim workgroup takes four launch tiles, one per wave (claim_tile_wave, vh_alloc.hip:
    // a quarter of the waves, each with four pixels per lane).  C3 28.4 -> 26.7 us same box; a 640x480 frame prefers the tile per
    // workgroup (8.9 against 11.1 us: the longer chain per wave is its tail), and so does every frame under the reference's walk
    // (C2 18.9 -> 19.9-22.7 us, C3 72.0 -> 71.5): profiles/r05_claim_wave_tile_ab.txt.  Hence the size rule (builds 7 / 8).
    const uint32_t flagsOld = hasOld ? c->pend.fp.flags : c->fp.flags;
    const bool large = host_num_tiles(c) > 2400u;
    int lean = lean_for(c, flagsOld, band, a.walkIndexed != 0u, false);
    const bool claimPerWave = hasNew && large && (lean == kLeanIndexed || lean == kLeanIndexedNt);
    if (claimPerWave) lean = lean_for(c, flagsOld, band, true, true);
    a.claimBlocks = !hasNew ? 0u : claimPerWave ? (host_num_tiles(c) + 3u) / 4u : host_num_tiles(c);
    a.commitBlocks = hasOld ? (uint32_t)c->commitBlocks : 0u;
    a.integrateBlocks = hasOld ? (uint32_t)c->pipeIntegrateGrid : 0u;
    // (the walk-free frame of a large image: its TSDF update is on the critical path, not under a walk -- twice the workgroups:
    // C3 26.1 -> 25.1 us, while C2 prefers the 512 it has, 8.7 against 9.0)
    if (hasOld && a.walkIndexed && large) a.integrateBlocks *= 2u;
    a.numEntries = (uint32_t)c->numEntries;
    a.walkGroups = 0u; a.walkReverse = 0u; a.claimLead = 0u;
    uint32_t claimWalk = a.claimBlocks + a.walkBlocks;          // workgroups of the two roles
    if (a.walkIndexed) {
        a.claimSpan = claim_span(c, a.claimBlocks, a.walkBlocks);
        a.claimRatio = claim_ratio(a.claimBlocks, a.claimSpan);
    } else {
        // The reference's walk: every role count a multiple of 8, so that the walk workgroup of ordinal w has blockIdx = w
        // (mod 8) in every launch (vh_frame.hip: grouped_role); span and ratio count groups.  The surplus commit and
        // integrate workgroups stride over the candidates and the list like the others; the surplus claim and walk
        // workgroups return.  The direction changes hands with every launch that carries a walk, not with a flush launch.
        a.commitBlocks = 8u * groups_of_8(a.commitBlocks);
        a.integrateBlocks = 8u * groups_of_8(a.integrateBlocks);
        const uint32_t claimGroups = groups_of_8(a.claimBlocks);
        a.walkGroups = groups_of_8(a.walkBlocks);
        a.claimSpan = claim_span(c, claimGroups, a.walkGroups);
        a.claimLead = claim_lead(c, claimGroups, a.walkGroups, a.claimSpan, true);       // (takes the lead off the span)
        a.claimRatio = claim_ratio(claimGroups, a.claimSpan);
        if (hasNew) a.walkReverse = take_walk_direction(c);
        claimWalk = 8u * (claimGroups + a.walkGroups);
    }
    args.planeNew = (hasNew && !newSensor) ? c->planeBuf[r.newParity].get() : nullptr;
    args.rawNew = (hasNew && newSensor) ? c->rawBuf[r.newParity].get() : nullptr;
    args.filter = c->claimFilter;
    args.filtNew = kPendFilterWords * (uint32_t)r.iNew; args.filtOld = kPendFilterWords * (uint32_t)r.iOld;
    args.filtClear = kPendFilterWords * (uint32_t)r.iClear;
#ifdef VH_DEBUG_SKIP_ROLES
    a.skipRoles = (uint32_t)c->debugSkipRoles;
#endif
    const dim3 grid(a.commitBlocks + a.integrateBlocks + claimWalk);
    In inNew{};
    if (hasNew) inNew = *in;
    // A lean build is told that both frames' flags are its own (vh_frame.hip: role_arguments).  lean_for is what makes that
    // true; a first launch, which has no pending frame, hands over the new frame's parameters in its place.  Checked here,
    // where a drift between lean_for and lean_build would otherwise be undefined behaviour on the device.
    const FrameParams &fpOld = hasOld ? c->pend.fp : c->fp;
    if (lean != kLeanNone && (c->fp.flags != lean_build(lean).flags || fpOld.flags != lean_build(lean).flags))
        return fail(VH_ERR_INVALID_ARGUMENT, "launch_pipelined: the lean build does not match the frames' flags");
    // (the two kernel arguments are built as the members of the struct that states the kernel's parameter list)
    if (hasOld && c->pend.sensor) {
        const DepthSensor d{c->rawBuf[r.oldParity], c->pend.k[0], c->pend.k[1], c->pend.k[2], c->pend.k[3]};
        const PipeSignature<In, DepthSensor> sig{__builtin_bit_cast(PipeLeadWords, a), {c->fp, r.dpNew, inNew, fpOld, r.dpOld, d, args}};
        rc = launch_pipelined_build<In, DepthSensor>(c, lean, band, serial, grid, sig.lead, sig.rest);
    } else {
        const DepthPlane d{c->planeBuf[r.oldParity], 1};
        const PipeSignature<In, DepthPlane> sig{__builtin_bit_cast(PipeLeadWords, a), {c->fp, r.dpNew, inNew, fpOld, r.dpOld, d, args}};
        rc = launch_pipelined_build<In, DepthPlane>(c, lean, band, serial, grid, sig.lead, sig.rest);
    }
    if (rc != VH_OK) return rc;
    pipe_launched(c, r, serial, hasNew ? PendingFrame::kSingle : PendingFrame::kNone, hasOld, true, false);     // (run_frame counts the frame)
    if (hasNew) {
        c->pend.fp = c->fp;
        c->pend.sensor = newSensor;
        if (newK) std::memcpy(c->pend.k, newK, sizeof c->pend.k);
    }
    return VH_OK;
}

// the pending frame's deferred half in a launch of its own, if it is of that kind (every observer comes through flush_pending)
static int flush_pending(vh_context *c, PendingFrame::Kind kind)
{
    if (c->pend.kind != kind || kind == PendingFrame::kNone) return VH_OK;
    const int rc = kind == PendingFrame::kSingle ? launch_pipelined<VertexMap>(c, nullptr, 0, nullptr) : launch_multi_pipelined(c, nullptr, 0);
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}
static int flush_pending(vh_context *c) { return flush_pending(c, c->pend.kind); }

// For whoever looks at the compact list from outside a frame (download, device pointers, the step-level TSDF
// update, collection, an explicit flush or synchronisation): the pending half first, then end B of the
// two-ended list (vh_walk.hip: CompactOut) behind end A -- the reference's dense list [0, occupied) -- and
// always in the buffer the context was created with (c->compactHome): pipelined frames alternate between two
// compact buffers, but a PtrContainer fetched once (as the reference does, VoxelUtils.cu:141-148) must stay
// good for the dense list after every later vh_flush / vh_synchronize.  Once no frame is pending the two
// buffers are interchangeable, so the home buffer becomes the current one again.
static int settle(vh_context *c)
{
    int rc = flush_pending(c);
    if (rc != VH_OK) return rc;
    VoxelEntry *home = c->compactHome;
    const bool away = c->dp.compact != home;
    if (c->foldA < 0 && !away) return VH_OK;
    rc = c->foldA >= 0 ? launch(c, kPhaseFlatten, compact_fold_kernel, dim3(64), dim3(256), c->dp, home, (uint32_t)c->numEntries,
                                c->foldA, c->foldB, c->foldNew)
                       : launch(c, kPhaseFlatten, compact_fold_kernel, dim3(64), dim3(256), c->dp, home, (uint32_t)c->numEntries,
                                c->occupiedCounter, -1, -1);
    c->foldA = -1;
    if (rc != VH_OK) return rc;
    if (away) {
        c->compactBuf[c->pipeParity ^ 1] = c->dp.compact;       // (compactBuf[] exist: only pipelined frames move dp.compact)
        c->compactBuf[c->pipeParity] = home;
        c->dp.compact = home;
    }
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_flush(vh_context *c)
{
    VH_TRACE("vh_flush");
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    DeviceGuard guard(c->device);
    return settle(c);
}

// One frame (pose and lock epoch already set): In = where the claim phase reads a pixel's vertex,
// Depth = where the TSDF update reads a pixel's camera z.  Honours "fused_frame" and "flatten_variant".
template <int kKind, class In>
static int launch_scan_claim(vh_context *c, const In &in, uint32_t claimBlocks, uint32_t scanBlocks, float *planeOut)
{
    if (kKind != kWalkIndexed) {
        // the reference's walk: both roles in groups of 8 workgroups (vh_frame.hip: grouped_role), span and ratio in groups
        const uint32_t claimGroups = groups_of_8(claimBlocks), walkGroups = groups_of_8(scanBlocks);
        uint32_t span = claim_span(c, claimGroups, walkGroups);
        const uint32_t lead = claim_lead(c, claimGroups, walkGroups, span, false);         // (takes the lead off the span)
        return launch(c, kPhaseFrameScanClaim, frame_scan_claim_kernel<kKind, In>, dim3(8u * (claimGroups + walkGroups)),
                      dim3(256), c->fp, c->dp, in, (uint32_t)c->numEntries, claimBlocks, c->fusedParity, planeOut,
                      span, claim_ratio(claimGroups, span), walkGroups, take_walk_direction(c), lead);
    }
    return launch(c, kPhaseFrameScanClaim, frame_scan_claim_kernel<kKind, In>, dim3(claimBlocks + scanBlocks),
                  dim3(256), c->fp, c->dp, in, (uint32_t)c->numEntries, claimBlocks, c->fusedParity, planeOut,
                  claim_span(c, claimBlocks, scanBlocks), claim_ratio(claimBlocks, claim_span(c, claimBlocks, scanBlocks)), 0u, 0u, 0u);
}

// the packed camera-z plane launch 1 leaves for launch 2 (vertex-map input only)
static inline float *fused_plane(vh_context *c, const VertexMap &)
{
    // optional: a failed allocation leaves it empty (launch 2 gathers from the vertex map as before) and the next frame tries again
    if (!c->fusedPlane) (void)c->fusedPlane.try_alloc((size_t)c->fp.width * c->fp.height);
    return c->fusedPlane;
}
static inline float *fused_plane(vh_context *, const SensorImage &) { return nullptr; }
static inline DepthPlane plane_depth(const DepthPlane &fromVerts, float *plane) { return plane ? DepthPlane{plane, 1} : fromVerts; }
static inline DepthSensor plane_depth(const DepthSensor &d, float *) { return d; }

static inline int pipe_is_sensor(const VertexMap &) { return 0; }
static inline int pipe_is_sensor(const SensorImage &) { return 1; }
struct PipeK { float v[4]; };
static inline PipeK pipe_k(const VertexMap &) { return PipeK{{0, 0, 0, 0}}; }
static inline PipeK pipe_k(const SensorImage &s) { return PipeK{{s.k[6], s.k[7], s.k[8], s.unit}}; }

template <class In, class Depth>
static int run_frame(vh_context *c, const In &in, const Depth &depth)
{
    int rc;
    if ((rc = ensure_band_candidates(c)) != VH_OK) return rc;
    c->occupiedCounter = kCompactCount;
    if (pipeline_applies(c)) {
        rc = launch_pipelined(c, &in, pipe_is_sensor(in), pipe_k(in).v);
        if (rc != VH_OK) return rc;
        if (c->profiling) c->profiledFrames += 1;
        VH_HIP(hipGetLastError());
        return VH_OK;
    }
    if ((rc = flush_pending(c)) != VH_OK) return rc;
    if (c->fusedFrame) {
        // two launches: {claim || table walk}, then {commit + integrate}; see vh_frame.hip
        const uint32_t claimBlocks = host_num_tiles(c);
        const uint32_t scanBlocks = walk_blocks(c);
        // Large images: launch 1 also leaves the camera z of every pixel in a packed float plane and launch 2
        // gathers from that instead of the 16-byte-strided .z of the vertex map, which drags every line of the
        // map through launch 2 (C3: 72 MB of counter traffic for 40 MB of algorithmic bytes).  In-process A/B:
        // C3 (1.2 M pixels) launch 1 +1.4 us, launch 2 -2.9 us; C2 (0.3 M) +0.7 / -0.1 us: hence the size rule.
        float *plane = (size_t)c->fp.width * c->fp.height >= ((size_t)1 << 20) ? fused_plane(c, in) : nullptr;
        if (c->flattenVariant == kWalkIndexed)
            rc = launch_scan_claim<kWalkIndexed>(c, in, claimBlocks, scanBlocks, plane);
        else
            rc = launch_scan_claim<kWalkStridedBallot>(c, in, claimBlocks, scanBlocks, plane);
        if (rc != VH_OK) return rc;
        const uint32_t commitBlocks = (uint32_t)c->commitBlocks;
        rc = launch(c, kPhaseFrameCommitIntegrate, frame_commit_integrate_kernel<Depth>,
                    dim3(commitBlocks + (uint32_t)c->integrateGrid), dim3(256), c->fp, c->dp, plane_depth(depth, plane),
                    commitBlocks, c->fusedParity);
        if (rc != VH_OK) return rc;
        c->foldA = kScanCount + c->fusedParity; c->foldB = kScanCountB + c->fusedParity; c->foldNew = kNewCount + c->fusedParity;
        c->fusedParity ^= 1;       // this frame cleared the other counter set for the next one
        c->compactArmed = false;
    } else {
        // alloc_commit re-arms the compact counter, so no memset node is needed here
        c->foldA = -1;
        if ((rc = launch_alloc(c, in)) != VH_OK) return rc;
        c->compactArmed = false;
        if ((rc = launch_flatten(c)) != VH_OK) return rc;
        if ((rc = launch_integrate(c, depth)) != VH_OK) return rc;
    }
    if (c->profiling) c->profiledFrames += 1;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_integrate(vh_context *c, const float pose[16], const vh_float4 *verts, const vh_float4 *normals)
{
    VH_TRACE("vh_integrate");
    if (!c || !pose || !verts) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    DeviceGuard guard(c->device);
    // a single-camera frame on a context that still holds a multi-camera frame's deferred half (pipeline_shards 2, e.g. the
    // shard of a vh_dist): that half is served first -- the two pipelines share buffer parity and counter sets
    int rc = flush_pending(c, PendingFrame::kMulti);
    if (rc == VH_OK) rc = vh_set_pose(c, pose);
    if (rc == VH_OK) rc = vh_reset_mutexes(c);
    if (rc != VH_OK) return rc;
    c->allocEpoch = c->epochTotal;
    const float4 *v = reinterpret_cast<const float4 *>(verts);
    return run_frame(c, VertexMap{v, reinterpret_cast<const float4 *>(normals)}, vertex_depth(v));
}

// The frame straight from the uint16 sensor image: preProcess's vertex computation happens inside
// the claim half, the TSDF update reads the image.  Equals vh_preprocess + vh_integrate.
extern "C" int vh_integrate_depth(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9])
{
    VH_TRACE("vh_integrate_depth");
    if (!c || !pose || !d_depth || !k_inv) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    DeviceGuard guard(c->device);
    int rc = flush_pending(c, PendingFrame::kMulti);      // (see vh_integrate)
    if (rc == VH_OK) rc = vh_set_pose(c, pose);
    if (rc == VH_OK) rc = vh_reset_mutexes(c);
    if (rc != VH_OK) return rc;
    SensorImage in;
    in.depth = d_depth;
    std::memcpy(in.k, k_inv, sizeof in.k);
    in.unit = 5000.0f;                                                   // CameraTrackingUtils.cu:64
    c->allocEpoch = c->epochTotal;
    return run_frame(c, in, DepthSensor{in.depth, in.k[6], in.k[7], in.k[8], in.unit});
}

// K frames in K + 1 launches: the pipeline switched on for the call, flushed at its end.  frame(i): frame i's entry point.
template <class Frame>
static int run_batch(vh_context *c, int32_t count, Frame frame)
{
    const int saved = c->pipeline;
    c->pipeline = 1;
    int rc = VH_OK;
    for (int32_t i = 0; i < count && rc == VH_OK; ++i) rc = frame(i);
    c->pipeline = saved;
    if (!saved) {
        const int rc2 = vh_flush(c);
        if (rc == VH_OK) rc = rc2;
    }
    return rc;
}

extern "C" int vh_integrate_batch(vh_context *c, int32_t count, const float *poses, const vh_float4 *const *d_verts,
                                  const vh_float4 *const *d_normals)
{
    if (!c || count < 0 || (count > 0 && (!poses || !d_verts))) return fail(VH_ERR_INVALID_ARGUMENT, "bad argument");
    return run_batch(c, count, [&](int32_t i) { return vh_integrate(c, poses + 16 * (size_t)i, d_verts[i], d_normals ? d_normals[i] : nullptr); });
}

extern "C" int vh_integrate_depth_batch(vh_context *c, int32_t count, const float *poses, const uint16_t *const *d_depth,
                                        const float k_inv[9])
{
    if (!c || count < 0 || (count > 0 && (!poses || !d_depth || !k_inv))) return fail(VH_ERR_INVALID_ARGUMENT, "bad argument");
    return run_batch(c, count, [&](int32_t i) { return vh_integrate_depth(c, poses + 16 * (size_t)i, d_depth[i], k_inv); });
}

// The raycast in the context's mode (option "raycast_mode"): the voxel DDA (default), optionally with the normal
// map of the hits written by the same pass, or the fixed-step march of rounds 1-2.
static int raycast_impl(vh_context *c, const float pose[16], float t_min, float t_max, float *d_depth_out,
                        vh_float4 *d_normals_out)
{
    VH_TRACE("vh_raycast");
    if (!c || !pose || !d_depth_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (!(t_max > t_min)) return fail(VH_ERR_INVALID_ARGUMENT, "t_max must exceed t_min");
    if (c->raycastMode == VH_RAYCAST_FIXED_STEP && d_normals_out)
        return fail(VH_ERR_INVALID_ARGUMENT, "the fixed-step march has no normal output (raycast_mode 0)");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }
    FrameParams fp = c->fp;
    std::memcpy(fp.T, pose, sizeof fp.T);
    dim3 grid((fp.width + 15) / 16, (fp.height + 15) / 16);
    DevPtrs dp = model_ptrs(c);
    int rc;
    if (c->raycastMode == VH_RAYCAST_FIXED_STEP) {
        const float q = (t_max - t_min) / fp.voxelSize;
        int nsteps = (q >= 2147483648.0f) ? 0x7fffffff : (int)q;
        nsteps += 1;
        rc = launch(c, kPhaseRaycast, raycast_kernel, grid, dim3(256), fp, dp, c->rc_fx, c->rc_fy, c->rc_cx, c->rc_cy, t_min, nsteps,
                    d_depth_out);
    } else {
        RaycastArgs ra;
        ra.fx = c->rc_fx; ra.fy = c->rc_fy; ra.cx = c->rc_cx; ra.cy = c->rc_cy;
        ra.tMin = t_min; ra.tMax = t_max;
        float inv[16];
        invert4x4(pose, inv);                      // cofactor inverse (cuda_SimpleMatrixUtil.h:944-1069), as vh_set_pose
        ra.zrow[0] = inv[8] * fp.voxelSize; ra.zrow[1] = inv[9] * fp.voxelSize; ra.zrow[2] = inv[10] * fp.voxelSize;
        ra.zrow[3] = inv[11];
        // Hang guard, never reached by a ray: a ray changes voxel coordinate a at most (t_max - t_min) * |E_a| + 1
        // times, |E_a| <= (|T_a0| max|dx| + |T_a1| max|dy| + |T_a2|) / voxelSize.  A view whose bound is not finite
        // or beyond 2^22 steps is refused (the oracle walks at most that many voxels per ray).
        const double mdx = std::max(std::fabs((0.0 - ra.cx) / ra.fx), std::fabs(((double)fp.width - 1.0 - ra.cx) / ra.fx));
        const double mdy = std::max(std::fabs((0.0 - ra.cy) / ra.fy), std::fabs(((double)fp.height - 1.0 - ra.cy) / ra.fy));
        double bound[3];                           // |T_a0| max|dx| + |T_a1| max|dy| + |T_a2|
        for (int a = 0; a < 3; ++a)
            bound[a] = std::fabs((double)pose[4 * a]) * mdx + std::fabs((double)pose[4 * a + 1]) * mdy + std::fabs((double)pose[4 * a + 2]);
        double steps = 16.0;
        for (int a = 0; a < 3; ++a) steps += 1.01 * ((double)t_max - (double)t_min) * bound[a] / (double)fp.voxelSize + 2.0;
        if (!(steps < 4194304.0)) return fail(VH_ERR_INVALID_ARGUMENT, "view too deep for the voxel size (more than 2^22 voxel steps per ray) or not finite");
        ra.budget = (int)steps;
        // The camera centre in voxel-grid units, and the domain: inside an allocated block the kernel steps the voxel
        // coordinate as a float (exact below 2^24), so a view that can reach |coordinate| >= 2^23 is refused.
        double reach = 0.0;
        for (int a = 0; a < 3; ++a) {
            ra.G[a] = pose[4 * a + 3] / fp.voxelSize + 0.5f;
            reach = std::max(reach, std::fabs((double)ra.G[a]) + std::fabs((double)t_max) * bound[a] / (double)fp.voxelSize +
                                        std::fabs((double)t_min) * bound[a] / (double)fp.voxelSize);
        }
        if (!(reach < 8388608.0)) return fail(VH_ERR_INVALID_ARGUMENT, "view reaches beyond 2^23 voxels from the origin");
        ra.invVs = 1.0f / fp.voxelSize;
        ra.stamps = reinterpret_cast<unsigned long long *>(c->raycastStamps);
        // Which form: the cooperative one where ONE pass of its beam step covers the depth range -- 64 x kCoopSubs half-block slabs
        // (C2's 2 cm voxels: 5 m in one sub-pass; C3's 5 mm voxels: 4.9 m in four).  Round 6, with the lists shared inside the
        // workgroup (1280x960 views of the 5 mm model after 300 / 1 000 / 2 000 poses): 242 / 302 / 312 us against 238 / 319 / 335
        // for the per-lane walk behind the beam front end -- equal on a sparse model, ahead on a dense one (before the sharing the
        // per-lane walk was ahead at 5 mm: 151 against 175 us).  Longer ranges (several windows) keep the per-lane walk.
        int beam = c->raycastBeam;
        if (beam == 3) beam = (t_max - t_min) <= 64.0f * (float)kCoopSubs * 4.0f * fp.voxelSize ? 2 : 1;
        ra.beam = t_min > 0.0f ? beam : 0;
        float4 *nrm = reinterpret_cast<float4 *>(d_normals_out);
        const dim3 block(64 * kDdaBlockWaves);
        ra.patchesX = (fp.width + 7) / 8;
        ra.numPatches = ra.patchesX * ((fp.height + 7) / 8);
        ra.groups = (ra.numPatches + kDdaBlockWaves - 1) / kDdaBlockWaves;
        if (ra.beam == 2)       // the cooperative form: a workgroup per group of four far-apart patches (vh_raycast_coop.hip)
            rc = nrm ? launch(c, kPhaseRaycast, raycast_coop_kernel<true>, dim3((unsigned)ra.groups), block, fp, dp, ra, d_depth_out, nrm)
                     : launch(c, kPhaseRaycast, raycast_coop_kernel<false>, dim3((unsigned)ra.groups), block, fp, dp, ra, d_depth_out, nrm);
        else
            rc = nrm ? launch(c, kPhaseRaycast, raycast_dda_kernel<true>, grid, block, fp, dp, ra, d_depth_out, nrm)
                     : launch(c, kPhaseRaycast, raycast_dda_kernel<false>, grid, block, fp, dp, ra, d_depth_out, nrm);
    }
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_raycast(vh_context *c, const float pose[16], float t_min, float t_max, float *d_depth_out)
{
    return raycast_impl(c, pose, t_min, t_max, d_depth_out, nullptr);
}

extern "C" int vh_raycast_normals(vh_context *c, const float pose[16], float t_min, float t_max, float *d_depth_out,
                                  vh_float4 *d_normals_out)
{
    if (!d_normals_out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return raycast_impl(c, pose, t_min, t_max, d_depth_out, d_normals_out);
}

// Block silhouettes: SDFRenderer::drawToFrontAndBack, SDFRenderer.cpp:165-208.
extern "C" int vh_render_blocks(vh_context *c, const float pose[16], float t_min, float t_max, float *d_front,
                                float *d_back)
{
    VH_TRACE("vh_render_blocks");
    if (!c || !pose || !d_front || !d_back) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (!(t_max > t_min) || !(t_min >= 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "need 0 <= t_min < t_max");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }
    BlockView bv;
    float inv[16];
    invert4x4(pose, inv);
    std::memcpy(bv.T, pose, sizeof bv.T);
    std::memcpy(bv.Tinv, inv, sizeof bv.Tinv);
    bv.fx = c->rc_fx; bv.fy = c->rc_fy; bv.cx = c->rc_cx; bv.cy = c->rc_cy;
    bv.tMin = t_min;
    bv.tMax = t_max;
    // records of the allocated blocks (32 bytes each + their 8-byte screen boxes on their own; a table holds at most
    // numVoxelBlocks of them, a view table one per entry) behind two counter words, allocated on first use (synchronises once)
    const size_t capacity = c->viewBlocks ? c->numEntries : std::min<size_t>(c->numEntries, c->params.numVoxelBlocks);
    if (!c->blockList || c->blockCapacity < capacity) {      // (a view context grows from 1 to numEntries at its first import)
        VH_HIP(hipStreamSynchronize(c->stream));                 // (the caller's stream logic: before the old list is freed)
        const int arc = c->blockList.alloc(4 + (sizeof(BlockRecord) + sizeof(uint2)) / sizeof(int32_t) * capacity, "blockList");
        if (arc != VH_OK) return arc;
        VH_HIP(hipMemsetAsync(c->blockList, 0, 16, c->stream));
        c->blockCapacity = capacity;
        c->blockParity = 0;
    }
    int32_t *counts = c->blockList;
    BlockRecord *records = reinterpret_cast<BlockRecord *>(counts + 4);
    uint2 *bounds = reinterpret_cast<uint2 *>(records + c->blockCapacity);
    const int parity = c->blockParity;
    const uint32_t words = (c->ownedBuckets + 31u) / 32u;
    int rc = launch(c, kPhaseRaycastBounds, blocks_list_kernel, dim3((unsigned)grid_for(words, 256)), dim3(256), c->fp, c->dp,
                    bv, records, bounds, (int32_t)capacity, counts, parity);
    if (rc == VH_OK)
        rc = launch(c, kPhaseRaycastBounds, blocks_tile_kernel, dim3((c->fp.width + 15) / 16, (c->fp.height + 15) / 16),
                    dim3(256), c->fp, bv, (const BlockRecord *)records, (const uint2 *)bounds, (int32_t)capacity, (const int32_t *)counts, parity,
                    d_front, d_back);
    c->blockParity ^= 1;
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}
