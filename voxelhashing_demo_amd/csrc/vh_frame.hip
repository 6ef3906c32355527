// vh_frame.hip -- the fused frame: SDF_Hashtable::integrate in two launches.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_device.h.
#pragma once

namespace vh {

// ---------------------------------------------------------------------------
// the fused frame: SDF_Hashtable::integrate in two launches
// ---------------------------------------------------------------------------
// Launch 1 runs the per-pixel claim phase and the table walk side by side: both only
// READ the hash table (claims go to the claim words, hits to the compact list), so the
// latency-bound pixel work hides under the bandwidth-bound walk.  The walk therefore
// sees the table as it was at the start of the frame; the entries this frame inserts
// are appended to the compact list by launch 2 -- they pass the frustum test by
// construction (allocBlocks tested the same key against the same pose, :673 / :732).
//
// In: where a pixel's vertex comes from -- VertexMap (the float4 map of the reference's
// interface) or SensorImage (vh_integrate_depth: the uint16 image, vertices computed in place).
// planeOut (nullable): the claim half also leaves the camera z of every pixel in a packed float plane
// for launch 2 to gather from -- 4 bytes per pixel written once here instead of a 16-byte-strided
// gather from the vertex map there (C3, launch 2: 72 MB of traffic for 40 MB of algorithmic bytes).
//
// Under the reference's walk the two roles are dealt in GROUPS of 8 consecutive workgroups (grouped_role): r = the
// workgroup's index among the claim + walk workgroups, g = r >> 3 its group, q = r & 7 its class.  Every class takes as
// many claim tiles as there are claim groups, where ITS multiply-high steps -- the classes q / 8 of a step apart, so the
// claim tiles stay spread over the span one by one (whole groups claiming together: 53.9 k frames/s on C2 against 54.1 k)
// -- and a walk workgroup's ordinal w = r - 8 * (claims of its class before it) keeps w = r (mod 8).  With every role
// count ahead of them a multiple of 8 too (the host's to ensure), the tile of ordinal w (vh_walk.hip: walk_tile) is read
// by a workgroup of the same blockIdx % 8 in every launch.  Claim indices 8 * step + q beyond claimBlocks fill up the
// last claim group: those workgroups return.  claimSpan and claimRatio count groups here; at g = claimSpan every class
// has had ceil(claimBlocks / 8) claims (claimRatio * claimSpan exceeds that many steps by less than claimSpan / 2^32).
// Returns true for a claim workgroup (index: its claim tile, to be tested against claimBlocks), false for a walk
// workgroup (index: its ordinal).
// claimLead: the claim window starts that many groups into the grid, [claimLead, claimLead + claimSpan) -- the groups ahead of
// it walk, with no claim before them (g below is the group's index inside the window; ahead of it the subtraction wraps).
__device__ __forceinline__ bool grouped_role(uint32_t r, uint32_t claimBlocks, uint32_t claimSpan, uint32_t claimRatio,
                                             uint32_t claimLead, uint32_t &index)
{
    const uint32_t g = (r >> 3) - claimLead, q = r & 7u;
    uint32_t before = (int32_t)g < 0 ? 0u : (claimBlocks + 7u) >> 3;
    if (g < claimSpan) {
        const unsigned long long phase = (unsigned long long)q << 29;          // q / 8 of a step
        before = (uint32_t)(((unsigned long long)g * claimRatio + phase) >> 32);
        const uint32_t after = (uint32_t)(((unsigned long long)(g + 1u) * claimRatio + phase) >> 32);
        if (after != before) { index = 8u * before + q; return true; }
    }
    index = r - 8u * before;
    return false;
}

// walkGroups, walkReverse: of the reference's walk (walk_tile); the walk-free frame (kKind = kWalkIndexed) keeps the
// single dealing described below and ignores them
template <int kKind, class In>
__global__ __launch_bounds__(256) void frame_scan_claim_kernel(const FrameParams fp, const DevPtrs dp, const In in,
                                                               uint32_t numEntries, uint32_t claimBlocks,
                                                               int parity, float *__restrict__ planeOut, uint32_t claimSpan,
                                                               uint32_t claimRatio, uint32_t walkGroups, uint32_t walkReverse,
                                                               uint32_t claimLead)
{
    if constexpr (kKind != kWalkIndexed) {
        uint32_t index;
        if (grouped_role(blockIdx.x, claimBlocks, claimSpan, claimRatio, claimLead, index)) {
            if (index >= claimBlocks) return;
            __builtin_amdgcn_s_setprio(3);
            claim_tile(fp, dp, in, index, kFusedCand + parity, kNoPending, planeOut);
        } else {
            flatten_tile<kKind>(fp, dp, numEntries, walk_tile(index, walkGroups, walkReverse),
                                CompactOut{kScanCount + parity, kScanCountB + parity, numEntries}, 8u * walkGroups);
        }
        return;
    }
    // The two roles are interleaved over the grid in proportion (block b is a claim block when
    // floor((b+1)*claim/total) steps): workgroups are dispatched roughly in index order, and
    // with all claim blocks in front a large image would fill the chip with latency-bound
    // pixel work before the first byte of the table is streamed.
    // The claim tiles end before the grid does (claimSpan < total; vh_api_frame.hip: claim_span): a claim
    // workgroup is a chain of dependent reads of ~4 us, and one dispatched among the last workgroups of a
    // 20 us launch is its tail.
    // (claim_index: the claim tiles 0 .. claimBlocks-1 spread evenly over workgroups 0 .. claimSpan-1 by a
    // multiply-high with claimRatio = ceil(claimBlocks * 2^32 / claimSpan) -- the host's numbers; a 64-bit
    // division per workgroup here cost the launch 2 us)
    const uint32_t total = gridDim.x;
    const bool inSpan = blockIdx.x < claimSpan;
    const uint32_t claimBefore = inSpan ? __umulhi(blockIdx.x, claimRatio) : claimBlocks;
    const uint32_t claimAfter = inSpan ? __umulhi(blockIdx.x + 1u, claimRatio) : claimBlocks;
    if (claimAfter != claimBefore) {
        // the latency-bound pixel waves issue first when they are ready, so they are off the compute
        // unit sooner (17.9 -> 17.6 us; raising the streaming waves instead cost 0.25 us)
        __builtin_amdgcn_s_setprio(3);
        claim_tile(fp, dp, in, claimBefore, kFusedCand + parity, kNoPending, planeOut);
    } else {
        flatten_tile<kKind>(fp, dp, numEntries, blockIdx.x - claimBefore,
                            CompactOut{kScanCount + parity, kScanCountB + parity, numEntries}, total - claimBlocks);
    }
}

// The words a per-frame counter set consists of: of the two-launch frame (two sets, by parity) ...
__device__ __forceinline__ void clear_fused_set(int32_t *counters, int parity)
{
    counters[kScanCount + parity] = 0;
    counters[kScanCountB + parity] = 0;
    counters[kNewCount + parity] = 0;
    counters[kFusedCand + parity] = 0;
}
// ... and of the pipelined frame (three, rotating; `set` = kPipeSetStride * index)
__device__ __forceinline__ void clear_pipe_set(int32_t *counters, int set)
{
    counters[kPipeScan + set] = 0;
    counters[kPipeScanB + set] = 0;
    counters[kPipeNew + set] = 0;
    counters[kPipeCand + set] = 0;
    counters[kPipeWinners + set] = 0;
}
// The close of a two-launch frame's commit phase.  Only the `workers` commit workgroups that served candidates take a ticket (a
// word that every workgroup of a large grid increments costs tens of microseconds): the last of them publishes the occupied count
// and clears the counter set of the other parity for the next frame.  scanCountB: end B of the single-camera frame's two-ended
// list (vh_walk.hip); the multi-camera frame has none and passes a literal 0.  (The pipelined kernels close in the same way over
// the rotating sets, each in its own lines: DESIGN_LOG.md.)
__device__ __forceinline__ void close_commit_fused(int32_t *counters, int workers, int parity, int scanCount, int scanCountB, int demanded)
{
    if (threadIdx.x == 0) {
        __threadfence();
        const int ticket = atomicAdd(counters + kCommitTicket, 1);
        if (ticket == workers - 1) {
            counters[kCompactCount] = scanCount + scanCountB + atomicAdd(counters + kNewCount + parity, 0);
            counters[kLastCandidates] = demanded;
            clear_fused_set(counters, parity ^ 1);
            counters[kCommitTicket] = 0;
        }
    }
}
// Launch 2: the first commitBlocks workgroups serve the candidates (one candidate per
// workgroup pass: lane 0 inserts, then all 256 lanes integrate the new block and it is
// appended to the compact list); the others stride over the entries the walk found.
// Depth: where the TSDF update reads a pixel's camera z -- DepthPlane on &verts[0].z or DepthSensor.
template <class Depth>
__device__ __forceinline__ void frame_commit_integrate(const FrameParams &fp, const DevPtrs &dp, const Depth &verts,
                                                       uint32_t commitBlocks, int parity)
{
    const int scanCount = dp.counters[kScanCount + parity];          // end A of the list; end B:
    const int scanCountB = dp.counters[kScanCountB + parity];
    if (blockIdx.x >= commitBlocks) {
        integrate_list(fp, dp, dp.compact, scanCount, (int)(blockIdx.x - commitBlocks), (int)(gridDim.x - commitBlocks), verts,
                       scanCountB, owned_entries(fp));
        return;
    }
    __shared__ VoxelEntry newEntry;
    __shared__ int inserted;
    const int demanded = dp.counters[kFusedCand + parity];
    const int n = min(demanded, (int)dp.candCapacity);
    // only the workgroups that have a candidate to serve take part in the ticket (a release fence and
    // a returning atomic on one word per workgroup: 128 of them cost 0.8 us of a steady-state frame
    // that has a few dozen candidates)
    const int workers = max(1, min(n, (int)commitBlocks));
    if ((int)blockIdx.x >= workers) return;
    for (int i = blockIdx.x; i < n; i += commitBlocks) {
        if (threadIdx.x == 0) {
            VoxelEntry e;
            inserted = commit_candidate(fp, dp, dp.candidates[i], e, (uint32_t)i) ? 1 : 0;
            if (inserted) {
                newEntry = e;
                dp.compact[scanCount + atomicAdd(dp.counters + kNewCount + parity, 1)] = e;
            }
        }
        __syncthreads();
        if (inserted) integrate_block(fp, dp, newEntry, verts);
        __syncthreads();
    }
    close_commit_fused(dp.counters, workers, parity, scanCount, scanCountB, demanded);
}

template <class Depth>
__global__ __launch_bounds__(256) void frame_commit_integrate_kernel(const FrameParams fp, const DevPtrs dp,
                                                                     const Depth verts, uint32_t commitBlocks,
                                                                     int parity)
{
    frame_commit_integrate(fp, dp, verts, commitBlocks, parity);
}

// ---------------------------------------------------------------------------
// the pipelined frame: ONE launch per frame (option "pipeline", vh_integrate_batch)
// ---------------------------------------------------------------------------
// The two launches of a frame are ordered by data -- commit(i) needs every claim of frame i -- but the
// second one is a few microseconds of latency (counters -> candidate -> bucket -> heap -> block) that a
// kernel boundary on each side turns into a quarter of the frame.  Here the launch of frame i+1 also
// carries the deferred half of frame i:
//     launch i+1 = { claim(i+1) || walk(i+1) || commit(i) + integrate(i) }
// so the only ordering left is one kernel boundary per frame.  What makes this exact:
//   * claim(i+1) must judge every bucket as it will be AFTER commit(i), which runs concurrently.  It
//     never reads a slot that is being written: frame i's claim words (final, written by the previous
//     launch) say for every bucket who won it and which slot the entry goes to (claim_word: slot -> key,
//     f), so the insertion in flight is substituted from there (probe_and_claim, Pending);
//   * walk(i+1) must list the entries allocated after commit(i) and visible from pose i+1.  An entry
//     that commit(i) is inserting is skipped by the walk whatever it sees of it (same claim words) and
//     appended to frame i+1's list by commit(i) itself after the frustum test with pose i+1;
//   * integrate(i) gathers depth from a private copy of frame i's camera-z plane (float) or sensor
//     image (uint16) that claim(i) wrote, so the caller's buffer is only read by the launch of its own
//     frame: no lifetime requirement beyond vh_integrate's;
//   * claim words, candidate lists and compact lists alternate between two buffers, the per-frame
//     counters between three sets (filled by frame i+1, consumed by frame i, cleared for frame i+2; the
//     rotation simply continues across flushes, a flush clearing the two sets it does not consume);
//   * a frame that would insert more entries than the heap has free blocks is refused as a whole (all its
//     winners count as heap_exhausted and retry next frame): then claim(i+1) knows -- from two numbers
//     that are stable while the launch runs -- that nothing is in flight and reads the table as it is.
//     (vh_integrate without the pipeline serves as many winners as there are blocks.)
// (Round 3 measured the slimmer argument block the round-2 review asked for -- one FrameParams, one DevPtrs, and of the
// pending frame only its inverse pose, lock epoch and three alternating pointers: 0.55 instead of 0.8 KB, scalar spills
// 173-208 -> 129-137 -- side by side with this form on one box (tools/ab_commits.sh): C2 18.6 vs 18.0 us, C3 70.6 vs
// 70.3, C2 with band allocation 24.1 vs 23.9.  Slower, so the two-struct form stays.  That experiment changed the block's
// SIZE; what a workgroup pays is the ORDER in which it reads the block -- see PipeLead.)
//
// The leading 64 bytes of the launch's arguments: what the role map needs and what a walk workgroup's loads need, so that ONE
// wide scalar load and one wait stand between a workgroup's start and its role, and a walk workgroup issues its whole stream
// (walk_load_tile) without reading anything else.  Everything behind it -- the two FrameParams, the two DevPtrs, PipeArgs --
// is read inside the role that uses it, where it is used.  (Until this form the kernel took both FrameParams by value and
// patched their flags for the lean builds: two structs live across every role, so every workgroup loaded and spilled both,
// piece by piece with a full wait each, and read the three counter words behind `live`, before it looked at its role --
// 17 scalar waits, 48 lane spills and a device-memory read ahead of a walk workgroup's first ptr load; DESIGN_LOG.md.)
// The kernel receives it as one 16-dword vector, so the load is one instruction whatever the compiler makes of the rest.
struct PipeLead {
    uint32_t commitBlocks, integrateBlocks, claimBlocks, walkBlocks;
    uint32_t claimSpan, claimRatio;        // claim tiles are interleaved with the first walk tiles: over claimSpan groups of 8 workgroups (grouped_role)
    uint32_t claimLead;                    // ... of which the first is group claimLead of the claim + walk workgroups
    uint32_t walkGroups, walkReverse;      // the reference's walk: its ordinals run over 8 * walkGroups >= walkBlocks, backward if walkReverse (vh_walk.hip: walk_tile)
    uint32_t numEntries;
    uint32_t hasNew, hasOld;               // first launch of a run: no old frame; flush launch: no new frame
    uint32_t walkIndexed;                  // flatten_variant 4: the walk role runs over the bucket-occupancy bitmap
    uint32_t skipRoles;                    // diagnostics build (VH_DEBUG_SKIP_ROLES, option "debug_skip_roles"): bit r set = workgroups of role r
                                           // (0 commit, 1 integrate, 2 claim, 3 walk) return at once: what the launch costs without them; else 0
    const VoxelEntry *table;               // = the new frame's DevPtrs::table
};
// (On the host the vector only travels by value between functions of this one translation unit, all built with the same
// flags, so the x86 note about its calling convention, -Wpsabi, has nothing to say: it is switched off around the two places
// that hand the vector on, the kernel below and vh_api_frame.hip's launch().)
typedef uint32_t PipeLeadWords __attribute__((ext_vector_type(16)));
static_assert(sizeof(PipeLead) == sizeof(PipeLeadWords), "PipeLead is the one 64-byte scalar load at the head of the arguments");

struct PipeArgs {
    int32_t setNew, setOld, setClear;      // counter sets: filled, consumed, cleared by this launch
    float *planeNew;                       // private depth copies written by claim(new) ...
    uint16_t *rawNew;
    uint32_t *filter;                      // claim filters (vh_alloc.hip: pend_maybe), three of kPendFilterWords words
    uint32_t filtNew, filtOld, filtClear;  // word offsets of the filter the new frame fills / the pending frame filled / this launch clears
    int32_t doneTag;                       // overflow list: the pending frame's tag (lock epochs since creation), published when its commit phase ends
    uint32_t spinLimit;                    // ... and how many polls a workgroup waits for it (wait_commit_done)
};

// Serialised pipelined launches (overflow list): the claim and walk workgroups of frame i+1 wait here until the commit phase
// of frame i -- workgroups of the SAME grid, with the lowest indices, hence dispatched first -- has published its tag.
// "Dispatched first" is how the hardware dispatches today, not a guarantee, so the wait is bounded: after `limit` polls
// (~1.5 us each) the workgroup counts itself in kSpinTimeouts and gives up; the host sees the counter in vh_get_counters and
// runs that context's overflow-list frames as two launches from then on (the frame that timed out has lost the work of the
// workgroups that gave up: vh_counters.spin_timeouts > 0 is an error report, not a mode).
constexpr uint32_t kSpinLimitDefault = 1u << 20;
__device__ __forceinline__ bool wait_commit_done(int32_t *counters, int32_t tag, uint32_t limit)
{
    __shared__ int reached;
    if (threadIdx.x == 0) {
        int ok = 0;
        for (uint32_t it = 0; it < limit; ++it) {
            if (__hip_atomic_load(counters + kPipeCommitDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag) { ok = 1; break; }
            __builtin_amdgcn_s_sleep(8);
        }
        if (!ok) atomicAdd(counters + kSpinTimeouts, 1);
        reached = ok;
        // the acquire: ONE cache invalidate per workgroup (its CU's vector cache, the XCD's non-coherent L2 lines), by the
        // wave that saw the tag; the other waves' loads come behind the barrier
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return reached != 0;
}

// The builds of the pipelined launch (kLean).  A lean build has both frames' option flags, the walk and the claim form folded in
// when the kernel is BUILT; the host picks it when the context's state is exactly its lean_build() (vh_api_frame.hip: lean_for).
enum : int {
    kLeanNone = 0,             // the generic build: flags, walk and claim form are read at run time
    kLeanShort = 1,            // the reference's walk, 4 entries per lane (the default of a table inside the Infinity Cache)
    kLeanShortNt = 2,          // ... with non-temporal walk loads (a table beyond it)
    kLeanRayDda = 3,           // 1 / 2 with the ray-DDA band, VH_BAND_RAY_DDA -- builds that exist with kBand only
    kLeanRayDdaNt = 4,
    kLeanIndexed = 5,          // 1 / 2 with the occupancy-index walk in place of the reference's -- the walk-free frame, no band
    kLeanIndexedNt = 6,
    kLeanIndexedWave = 7,      // 5 / 6 with a launch tile per wave in the claim role, claim_tile_wave -- the walk-free frame of a
    kLeanIndexedWaveNt = 8,    // large image (as a run-time switch of builds 5 / 6 it cost the 640x480 frame 8.9 -> 9.45 us)
    kLeanBuilds = 9
};
struct LeanBuild { uint32_t flags; bool indexed, claimPerWave; };
constexpr LeanBuild lean_build(int kLean)
{
    return {kFlagWalkShort | (kLean % 2 == 0 ? kFlagWalkNt : 0u) | (kLean == kLeanRayDda || kLean == kLeanRayDdaNt ? kFlagBandRayDda : 0u),
            kLean >= kLeanIndexed, kLean >= kLeanIndexedWave};
}

// is frame i's commit phase inserting (live) or refusing everything?  Both numbers are stable while the launch runs: the
// count of claimed buckets was final when the previous launch ended, the free-block count was stored by its last commit
// workgroup (or, in a run's first launch, its first workgroup) in a word this launch does not write.  Asked by the roles that
// need the answer, when they need it: commit per candidate pass, claim behind its vertex requests, walk only in a wave that
// found an allocated entry.
template <bool kSerial>
__device__ __forceinline__ bool pending_live(uint32_t hasOld, const int32_t *counters, int32_t setOld)
{
    if (kSerial) return hasOld != 0u;
    return hasOld && counters[kPipeHeapFree + setOld] >= counters[kPipeWinners + setOld];
}

// The launch's argument block behind its leading piece, one struct: the kernel's second and last parameter, so it lies in the
// argument segment right behind the 64 bytes of the first, laid out as below.
template <class In, class Depth>
struct PipeKernargs {
    FrameParams fpNew;
    DevPtrs dpNew;
    In inNew;
    FrameParams fpOld;
    DevPtrs dpOld;
    Depth depthOld;
    PipeArgs a;
};
// The kernel's parameter list as the argument segment lays it out: every parameter at the next offset that suits its
// alignment, in order -- which is a struct of the parameters.  role_arguments reads the second one at the offset this gives;
// launch_pipelined (vh_api_frame.hip) builds its two arguments as the members of one, so host and device agree by type.
template <class In, class Depth>
struct PipeSignature {
    PipeLeadWords lead;
    PipeKernargs<In, Depth> rest;
};

// The argument block as ONE ROLE reads it.  Read through the kernel's parameter, a field that two roles use is loaded once,
// ahead of both -- the compiler places such a load in the block that dominates its uses, which is the role decision: that is
// how the block of loads, waits and spills in front of every role came about, and it comes back with any field that the
// claim role, a listing walk wave and the commit role share (the frustum of the new frame, the counters pointer ...).  So
// each role takes the segment's address through an empty volatile asm at the point where it may start to read it: loads
// behind that point cannot move ahead of it and are not merged with another role's.  (Scalar loads all the same: the asm
// hands back a uniform pointer into the constant address space.)
template <class In, class Depth, int kLean>
__device__ __forceinline__ const PipeKernargs<In, Depth> &role_arguments()
{
    typedef PipeKernargs<In, Depth> K;
    typedef PipeSignature<In, Depth> Signature;
    static_assert(offsetof(Signature, lead) == 0 && offsetof(Signature, rest) == sizeof(PipeLeadWords),
                  "frame_pipelined_kernel(lead, rest): rest lies right behind lead");
    typedef const __attribute__((address_space(4))) char *SegmentBytes;
    typedef const __attribute__((address_space(4))) K *SegmentPtr;
    SegmentPtr p = (SegmentPtr)((SegmentBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(Signature, rest));
    asm volatile("" : "+s"(p));
    const K &k = *(const K *)p;
    // How a lean build's flags reach the device functions: as a fact about the arguments, not as a patched copy of them.
    // The host launches build kLean only when both frames' flags ARE lean_build(kLean).flags (vh_api_frame.hip: lean_for),
    // and this tells the compiler so: every `fp.flags & ...` down the call tree folds as it did when the kernel overwrote the
    // word in by-value copies -- which made both structs live across every role.
    constexpr uint32_t leanFlags = lean_build(kLean).flags;
    if (kLean != kLeanNone) {
        __builtin_assume(k.fpNew.flags == leanFlags);
        __builtin_assume(k.fpOld.flags == leanFlags);
    }
    return k;
}

// l: the leading piece of the arguments, in registers; everything else is still in the argument block and is read by the
// role that uses it (role_arguments).
template <class In, class Depth, bool kBand, bool kSerial, int kLean>
__device__ __forceinline__ void frame_pipelined(const PipeLead &l)
{
    typedef PipeKernargs<In, Depth> K;
    constexpr LeanBuild lean = lean_build(kLean);
    const bool walkIndexed = kLean != kLeanNone ? lean.indexed : l.walkIndexed != 0u;
    // With the overflow list an insertion in flight can change a chain link and a slot behind another bucket, which the
    // claim phase cannot substitute from the claim words alone.  Those frames are serialised INSIDE the launch instead: the
    // claim and walk workgroups of frame i+1 start when commit(i) has published its tag, and then read the table as it
    // is -- one launch per frame still, TSDF update(i) still beside walk(i+1); commit(i) serves as many winners as the heap
    // has blocks, like the unpipelined frame (no whole-frame refusal), and leaves its new entries for walk(i+1) to find.
    // (kSerial = the context has the list on: a build of its own -- the code of this launch is weighed by the microsecond:
    // the run-time form of this switch cost the C2 launch 0.7 us)
    constexpr bool serial = kSerial;
    // Roles by workgroup index: [commit][integrate][claim and walk interleaved as in
    // frame_scan_claim_kernel]: frame i's deferred half runs first, at full width, then the table streams.
    // In-process A/B on C2 / C3 (launch time, us): this order with 512 integrate workgroups 18.8 / 88.9; with
    // 2048 of them (mostly idle, but dispatched before the first walk tile) 19.7 / 91.9; integrate and claim
    // workgroups interleaved among the walk tiles 20.5 / 93.7 (the latency-bound block updates then hold the
    // slots the stream needs); all claim tiles before the walk 20.4 / 93.0; the deferred half at the END of
    // the grid, where the walk drains (or commit first, integrate last) 21.5 / 105.9 against 21.0 / 94.6 for
    // this order on that box.  (Those orders were selectable at run time for a while; the run-time mapping
    // with its 64-bit divisions per workgroup cost every launch 2 us and is gone.)
    // EVERY figure above predates the alternating sweep (vh_walk.hip: walk_tile): the first walk ordinals of a launch were
    // not served from an XCD's L2 then, so it did not matter in that way what was dealt among them.  With the sweep, the
    // role table (profiles/pipelined_roles_reverse_C2.txt) has the reversal win 2.6 us for the walk alone and 1.5 us for the
    // whole launch; the claim role and the deferred half each take about half a microsecond of it back.  Hence the claim
    // window's lead (grouped_role: claimLead); the order of the roles is as it was.
    const uint32_t b = blockIdx.x;
    uint32_t role, index;                          // 0 commit, 1 integrate, 2 claim, 3 walk
    if (b < l.commitBlocks) { role = 0; index = b; }
    else if (walkIndexed) {
        // The walk-free frame streams nothing: every role is a chain of dependent reads plus arithmetic, and a chain that starts
        // late is the launch's tail.  The index walk's workgroups are few and their chain is the longest (bitmap -> buckets ->
        // frustum test -> list), so they come first, then the TSDF update, then the claim tiles; spread among the claim tiles
        // like the streaming walk they cost C2 10.8-11.2 us against 9.0-9.2, C3 28.1 against 27.6 (same box, generic build,
        // profiles/r05_index_walk_shapes.txt); their issue priority makes no difference.
        const uint32_t r = b - l.commitBlocks;
        if (r < l.walkBlocks) { role = 3; index = r; }
        else if (r < l.walkBlocks + l.integrateBlocks) { role = 1; index = r - l.walkBlocks; }
        else { role = 2; index = r - l.walkBlocks - l.integrateBlocks; }
    }
    else if (b < l.commitBlocks + l.integrateBlocks) { role = 1; index = b - l.commitBlocks; }
    else {
        // the claim tiles are spread, in groups of 8, over the first l.claimSpan groups of the claim + walk workgroups
        // (grouped_role: multiply-high by l.claimRatio = ceil(claimGroups * 2^32 / claimSpan), no division in the kernel;
        // the host keeps l.commitBlocks + l.integrateBlocks a multiple of 8, so a walk ordinal = blockIdx mod 8)
        const bool claims = grouped_role(b - l.commitBlocks - l.integrateBlocks, l.claimBlocks, l.claimSpan, l.claimRatio, l.claimLead, index);
        role = claims ? 2u : 3u;
        if (claims && index >= l.claimBlocks) return;          // (fills up the last claim group)
    }
#ifdef VH_DEBUG_SKIP_ROLES
    if (l.skipRoles & (1u << role)) {
        // (the commit role also clears the rotating counter sets: left uncleared, the lists a later mask's TSDF update reads grow
        // over entries nobody wrote)
        const K &k = role_arguments<In, Depth, kLean>();
        if (role == 0u && b == 0u && threadIdx.x == 0 && l.hasOld) {
            clear_pipe_set(k.dpNew.counters, k.a.setClear);
            if (!l.hasNew) clear_pipe_set(k.dpNew.counters, k.a.setNew);
        }
        // (... and in a run's first launch the workgroup of claim tile 0 leaves the free-block count, below, skipped or not)
        if (!l.hasOld && role == 2u && index == 0u && threadIdx.x == 0)
            k.dpNew.counters[kPipeHeapFree + k.a.setNew] = k.dpNew.counters[kHeapCounter] + 1;
        return;
    }
    // (mask 16, the claim tiles end before their probes: the host sets kFlagDebugNoProbe in the context's flags, which selects
    // the generic build, and claim_tile reads it there)
#endif
    if (role >= 2u) {
        // ---- frame i+1: claim || walk ----
        if (!l.hasNew) return;
        if (serial && l.hasOld) {
            // (the commit and integrate workgroups have the lowest indices of the grid: they are running or done when this one starts)
            const K &k = role_arguments<In, Depth, kLean>();
            if (!wait_commit_done(k.dpNew.counters, k.a.doneTag, k.a.spinLimit)) return;
        }
        // the frame whose commit phase runs beside this workgroup: `live` is two words of device memory, the rest comes from
        // the far end of the arguments -- made behind a tile's own first loads
        const auto pending = [&](const K &k) {
            return Pending{l.hasOld && !serial ? k.dpOld.claim : nullptr, k.dpOld.candidates, k.fpOld.epoch,
                           pending_live<serial>(l.hasOld, k.dpNew.counters, k.a.setOld),
                           serial ? -1 : kPipeWinners + k.a.setNew,
                           k.a.filter && l.hasOld && !serial ? k.a.filter + k.a.filtOld : nullptr,
                           k.a.filter && !serial ? k.a.filter + k.a.filtNew : nullptr};
        };
        if (role == 3u && !walkIndexed) {
            // The reference's walk: tile and loads from the leading piece alone -- no wait, no spill and no other read between
            // the role decision and the last ptr load (a lean build; the generic one reads the flags word first).  A wave
            // that finds all its entries free -- nearly every wave -- ends there; only one that has something to list goes
            // on to read the arguments: frustum, list and counters, the pending frame.
            const uint32_t flags = kLean != kLeanNone ? lean.flags : role_arguments<In, Depth, kLean>().fpNew.flags;
            const uint32_t tile = walk_tile(index, l.walkGroups, l.walkReverse);
            // (the pointer arrived as two words of the leading vector: named a pointer to device memory here, or the loads
            // would be flat ones)
            typedef const __attribute__((address_space(1))) VoxelEntry *GlobalTable;
            // (walk_load_tile asks a FrameParams for the non-temporal flag and a DevPtrs for the table: two locals that hold
            // just those, the rest of them is never read)
            FrameParams loadFp{};
            DevPtrs loadDp{};
            loadFp.flags = flags;
            loadDp.table = (VoxelEntry *)(GlobalTable)(uintptr_t)l.table;
            const auto walk = [&](auto &ptrs) {
                walk_load_tile(loadFp, loadDp, l.numEntries, tile, ptrs);
                if (!walk_wave_live(ptrs)) return;
                const K &k = role_arguments<In, Depth, kLean>();
                walk_process_tile(k.fpNew, k.dpNew, tile, ptrs, CompactOut{kPipeScan + k.a.setNew, kPipeScanB + k.a.setNew, l.numEntries},
                                  pending(k));
            };
            if (flags & kFlagWalkShort) {
                int32_t ptrs[kEntriesPerLaneShort];
                walk(ptrs);
            } else {
                int32_t ptrs[kEntriesPerLane];
                walk(ptrs);
            }
            return;
        }
        const K &k = role_arguments<In, Depth, kLean>();
        if (role == 3u) {
            flatten_index_tile(k.fpNew, k.dpNew, index, CompactOut{kPipeScan + k.a.setNew, kPipeScanB + k.a.setNew, l.numEntries},
                               pending(k));                                        // (opt-in: not the reference's walk)
            return;
        }
        __builtin_amdgcn_s_setprio(3);
        // first launch of a run (no frame in flight): nobody pops the heap during it, so one of its workgroups -- the one of claim
        // tile 0: a claim tile has the time, a walk workgroup does not -- leaves the free-block count the NEXT launch will test
        // frame i+1's insertions against
        const auto leave_heap_free = [&]() {
            if (!l.hasOld && index == 0u && threadIdx.x == 0) k.dpNew.counters[kPipeHeapFree + k.a.setNew] = k.dpNew.counters[kHeapCounter] + 1;
        };
        if (!kBand && lean.claimPerWave) {
            // (a launch tile per wave: the host sized the role at a quarter of the tiles, vh_api_frame.hip)
            leave_heap_free();
            const uint32_t tile = index * (256u / kWave) + threadIdx.x / kWave;
            if (tile < num_tiles(k.fpNew))
                claim_tile_wave<In>(k.fpNew, k.dpNew, k.inNew, tile, kPipeCand + k.a.setNew, pending(k), k.a.planeNew, k.a.rawNew);
        } else {
            // the tile's pixels are requested first; what the probes need is read while they are in flight
            // (load_pixel here, with the private depth copy; claim_tile then takes the pixel from the register: LoadedPixel)
            const PixelVertex p = load_pixel(k.fpNew, k.inNew, index, threadIdx.x, k.a.planeNew, k.a.rawNew);
            leave_heap_free();
            claim_tile<LoadedPixel, kBand>(k.fpNew, k.dpNew, LoadedPixel{p.v, p.n}, index, kPipeCand + k.a.setNew, pending(k), nullptr, nullptr,
                                           walkIndexed);
        }
        return;
    }
    if (!l.hasOld) return;
    const K &k = role_arguments<In, Depth, kLean>();
    const FrameParams &fpNew = k.fpNew, &fpOld = k.fpOld;
    const DevPtrs &dpNew = k.dpNew, &dpOld = k.dpOld;
    const Depth &depthOld = k.depthOld;
    const PipeArgs &a = k.a;
    int32_t *counters = dpNew.counters;
    if (role == 1u) {
        // ---- frame i: TSDF update of the blocks its walk (and commit(i-1)) listed ----
        // (the two ends' counts are the role's first reads: its chain is counts -> entry -> voxels)
        const int scanOld = counters[kPipeScan + a.setOld], scanOldB = counters[kPipeScanB + a.setOld];
        integrate_list(fpOld, dpOld, dpOld.compact, scanOld, (int)index, (int)l.integrateBlocks, depthOld, scanOldB, l.numEntries);
        return;
    }
    // ---- frame i: commit ----
    // (its chain -- counts -> candidate -> bucket -> heap -> block -- starts before the filter's stores are issued)
    const int demandedOld = counters[kPipeCand + a.setOld];
    const int scanOld = counters[kPipeScan + a.setOld];
    const bool live = pending_live<serial>(l.hasOld, counters, a.setOld);
    const int candOld = min(demandedOld, (int)dpOld.candCapacity);
    // the filter frame i+2 will fill: cleared here (nobody reads or writes it during this launch); a flush launch clears
    // the one a new frame would have filled as well, so that a run always starts on an empty one
    if (a.filter) {
        for (uint32_t t = index * 256u + threadIdx.x; t < kPendFilterWords; t += l.commitBlocks * 256u) {
            a.filter[a.filtClear + t] = 0u;
            if (!l.hasNew) a.filter[a.filtNew + t] = 0u;
        }
    }
    __shared__ VoxelEntry newEntry;
    __shared__ int inserted;
    const int workers = max(1, min(candOld, (int)l.commitBlocks));
    if ((int)index >= workers) return;
    for (int i = (int)index; i < candOld; i += (int)l.commitBlocks) {
        if (threadIdx.x == 0) {
            inserted = 0;
            const int4 k = dpOld.candidates[i];
            if (live) {
                VoxelEntry e;
                inserted = commit_candidate(fpOld, dpOld, k, e, (uint32_t)i, false) ? 1 : 0;
                if (inserted) {
                    newEntry = e;
                    dpOld.compact[scanOld + atomicAdd(counters + kPipeNew + a.setOld, 1)] = e;
                    // what walk(i+1) would have listed had it seen the entry
                    if (l.hasNew && !serial && block_in_frustum(fpNew, e.pos[0], e.pos[1], e.pos[2]))
                        dpNew.compact[atomicAdd(counters + kPipeScan + a.setNew, 1)] = e;
                }
            } else {
                const uint32_t local = hash_block(k.x, k.y, k.z, fpOld.numBuckets) - fpOld.bucketLo;
                const unsigned long long w = dpOld.claim[local];
                if (claim_epoch(w) == fpOld.epoch && claim_slot(w) == (uint32_t)i) atomicAdd(counters + kHeapExhausted, 1);
            }
        }
        __syncthreads();
        if (inserted) integrate_block(fpOld, dpOld, newEntry, depthOld);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __threadfence();
        const int ticket = atomicAdd(counters + kCommitTicket, 1);
        if (ticket == workers - 1) {
            counters[kCompactCount] = scanOld + counters[kPipeScanB + a.setOld] + atomicAdd(counters + kPipeNew + a.setOld, 0);
            counters[kLastCandidates] = demandedOld;
            clear_pipe_set(counters, a.setClear);
            if (!l.hasNew) clear_pipe_set(counters, a.setNew);      // flush launch: the set a new frame would have filled is unused: the next
                                                                    // run starts on it (the host keeps rotating), and finds it empty
            counters[kPipeHeapFree + a.setNew] = atomicAdd(counters + kHeapCounter, 0) + 1;   // what the next launch starts with
            counters[kCommitTicket] = 0;
            if (serial) {                          // every committer fenced before its ticket: the table is settled
                __threadfence();
                __hip_atomic_store(counters + kPipeCommitDone, a.doneTag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// kBand: the new frame allocates a truncation band (vh_set_alloc_band > 0); false = the reference's frame, without the band code
// kLean != kLeanNone: everything the flags guard (overflow list, DDA band, TSDF-update variants, the other walk forms) is
// folded away by the compiler: 3.3 k instead of 6.8 k instructions; same box, same process: C2 18.35 -> 17.57 us, C3 69.4 ->
// 68.4.  (Folding the semantics and a bucket size of 5 in as well: C2 17.2 but C3 70.2; one at a time: the semantics C2 17.9 / C3 68.4, the bucket size 17.8 / 75.2, the shard's
// bucket range 17.45 / 69.0 against 17.6 / 68.5 -- not done: what the compiler makes of a smaller kernel is not monotone.
// The same builds of the two-launch kernels: no difference (C2 16.27 + 4.45 us either way, C3 63.0 + 11.7 / 63.4 + 11.4).)
// (Eight waves per SIMD instead of the seven the 106 SGPRs allow -- __launch_bounds__(256, 8): 78 SGPRs, 129 instead of 100 of
// them spilled to VGPR lanes -- measured in round 4, same box: C2 17.69 -> 18.37 us, C3 69.0 -> 69.4, C2 with the band 22.9 ->
// 25.4.  The launch does not lack wave slots; the spill traffic lengthens the claim tiles.  profiles/r04_ab_pipe_waves.txt)
// (the kernel itself reads its first parameter, the leading piece, and nothing of the second: role_arguments)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpsabi"
template <class In, class Depth, bool kBand, bool kSerial, int kLean>
__global__ __launch_bounds__(256) void frame_pipelined_kernel(const PipeLeadWords lead, const PipeKernargs<In, Depth>)
{
    // (the parameters are PipeSignature's members, in its order: role_arguments finds the second through that struct)
    static_assert(std::is_same<decltype(PipeSignature<In, Depth>::lead), PipeLeadWords>::value &&
                  std::is_same<decltype(PipeSignature<In, Depth>::rest), PipeKernargs<In, Depth>>::value, "keep PipeSignature in step");
    const PipeLead l = __builtin_bit_cast(PipeLead, lead);
    frame_pipelined<In, Depth, kBand, kSerial, kLean>(l);
}
#pragma clang diagnostic pop

}  // namespace vh
