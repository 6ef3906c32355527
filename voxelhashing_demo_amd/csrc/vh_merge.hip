// vh_merge.hip -- one TSDF model fused into another under a rigid transform: vh_merge (include/voxelhash.h
// states the rule, tests/merge_ref.py is its executable form; no counterpart in the reference).
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_sample.hip (the samples) and vh_gc.hip (the marks).
//   merge_keys_kernel      one lane per entry of src: the dst block keys its 8.5^3-voxel box can reach, counted (first pass) or
//                          written as the records of ONE key bin (second pass), which claim_bins_kernel + alloc_commit_kernel
//                          insert as they insert any bin
//   merge_missing_kernel   records of the bin whose key is dst's business and not in dst: what ends the allocation rounds
//   merge_list_kernel      the distinct blocks of the bin that dst holds, each once into the compact list (one mark bit per entry)
//   merge_update_kernel    the TSDF update's launch shape over that list: a 256-lane workgroup per 8^3 block, two x-neighbouring
//                          voxels per lane as one 16-byte cell, each sampled from src by sample_trilinear / the nearest sample
#pragma once

namespace vh {

// rows 0..2 of a rigid transform, row-major
struct MergeTransform { float m[12]; };

__device__ __forceinline__ float merge_row(const float *m, int r, float x, float y, float z)
{
    return ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// device words of a call (unsigned long long each)
enum MergeWord : int { kMergeSource = 0, kMergeSkipped, kMergeRecords, kMergeMissing, kMergeWords };
constexpr unsigned long long kMergeEntryCap = 1ull << 40;      // what one entry adds to the record count at most (refusal only)

// The candidate keys of src block k: the box [8k - 0.5, 8k + 8] in src voxels, its corners taken to dst voxel units, the blocks of
// gmin = ceil(lo) .. gmax = ceil(hi) - 1 per axis.  false: a corner outside the domain (the block is skipped).
struct MergeBox { int lo[3], n[3]; };

__device__ __forceinline__ bool merge_box(const int *pos, const MergeTransform &T, float vsSrc, float vsDst, MergeBox &box)
{
    float lo[3], hi[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float e[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const long long k8 = (long long)pos[a] * 8;
            e[a] = ((c >> a) & 1) ? (float)(k8 + 8) : (float)k8 - 0.5f;
        }
        const float x = e[0] * vsSrc, y = e[1] * vsSrc, z = e[2] * vsSrc;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float u = merge_row(T.m, r, x, y, z) / vsDst;
            ok = ok && __builtin_fabsf(u) < kSampleDomain;              // false for NaN
            lo[r] = c == 0 ? u : __builtin_fminf(lo[r], u);
            hi[r] = c == 0 ? u : __builtin_fmaxf(hi[r], u);
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int gmin = f2i_rz(__builtin_ceilf(lo[a])), gmax = f2i_rz(__builtin_ceilf(hi[a])) - 1;
        box.lo[a] = gmin >> 3;
        box.n[a] = max(0, (gmax >> 3) - (gmin >> 3) + 1);
    }
    return true;
}

// bin == nullptr: count only (words[kMergeSource / kMergeSkipped / kMergeRecords]).  Otherwise the records go into the bin
// (vh_shard.hip: record 0 = {count, 0, 0, 0}, then {x, y, z, rank}); rank = the src entry, so a key's contenders are told apart.
__global__ __launch_bounds__(256) void merge_keys_kernel(const VoxelEntry *__restrict__ srcTable, uint32_t srcEntries,
                                                         const MergeTransform T, float vsSrc, float vsDst,
                                                         unsigned long long *__restrict__ words, int4 *__restrict__ bin,
                                                         int32_t capacity)
{
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= srcEntries) return;
    const VoxelEntry e = srcTable[at];
    if (e.ptr == VH_FREE_BLOCK) return;
    MergeBox box;
    const bool ok = merge_box(e.pos, T, vsSrc, vsDst, box);
    if (!bin) {
        atomicAdd(words + kMergeSource, 1ull);
        if (!ok) { atomicAdd(words + kMergeSkipped, 1ull); return; }
        unsigned long long n = (unsigned long long)box.n[0] * (unsigned long long)box.n[1];       // each below 2^29
        n = n > kMergeEntryCap ? kMergeEntryCap : n * (unsigned long long)box.n[2];
        atomicAdd(words + kMergeRecords, n > kMergeEntryCap ? kMergeEntryCap : n);
        return;
    }
    if (!ok) return;
    // (the host has seen the count and let the call through: the product fits the bin, so an int)
    const int n = box.n[0] * box.n[1] * box.n[2];
    if (n <= 0) return;
    int slot = atomicAdd(&bin[0].x, n) + 1;
    for (int z = 0; z < box.n[2]; ++z)
        for (int y = 0; y < box.n[1]; ++y)
            for (int x = 0; x < box.n[0]; ++x, ++slot)
                if (slot < capacity) bin[slot] = make_int4(box.lo[0] + x, box.lo[1] + y, box.lo[2] + z, (int)at);
}

// entry index of the key in this table, or ~0u (the caller has checked that its bucket is owned)
__device__ __forceinline__ uint32_t merge_find_entry(const FrameParams &fp, const DevPtrs &dp, uint32_t local, int kx, int ky, int kz)
{
    if (fp.flags & kFlagOverflow) {
        uint32_t prev;
        return find_entry_overflow(fp, dp.table, owned_entries(fp), local, kx, ky, kz, prev);
    }
    const VoxelEntry *bucket = dp.table + (size_t)local * fp.bucketSize;
    for (uint32_t s = 0; s < fp.bucketSize; ++s) {
        const VoxelEntry e = bucket[s];
        if (e.ptr == VH_FREE_BLOCK) break;                          // entries form a prefix
        if (e.pos[0] == kx && e.pos[1] == ky && e.pos[2] == kz) return local * fp.bucketSize + s;
    }
    return ~0u;
}

// records (duplicates counted) whose key belongs to this table's bucket range and is not in it
__global__ __launch_bounds__(256) void merge_missing_kernel(const FrameParams fp, const DevPtrs dp, const int4 *__restrict__ bin,
                                                            int32_t count, unsigned long long *__restrict__ words)
{
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t mine = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const int4 k = bin[1 + i];
        const uint32_t h = hash_block(k.x, k.y, k.z, fp.numBuckets);
        if (h < fp.bucketLo || h >= fp.bucketHi) continue;
        mine += merge_find_entry(fp, dp, h - fp.bucketLo, k.x, k.y, k.z) == ~0u;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) mine += __shfl_xor(mine, d);
    if (lane == 0 && mine) atomicAdd(words + kMergeMissing, (unsigned long long)mine);
}

// The compact list of the call: every block of the bin that the table holds, once -- the first record to set the entry's mark
// bit appends it.  The host clears the marks behind the call (they are all zero between calls: vh_gc.hip).
__global__ __launch_bounds__(256) void merge_list_kernel(const FrameParams fp, const DevPtrs dp, const int4 *__restrict__ bin,
                                                         int32_t count)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const int4 k = bin[1 + i];
        const uint32_t h = hash_block(k.x, k.y, k.z, fp.numBuckets);
        if (h < fp.bucketLo || h >= fp.bucketHi) continue;
        const uint32_t at = merge_find_entry(fp, dp, h - fp.bucketLo, k.x, k.y, k.z);
        if (at == ~0u) continue;
        const uint32_t bit = 1u << (at & 31u);
        if (atomicOr(dp.gcMarks + (at >> 5), bit) & bit) continue;
        const int slot = atomicAdd(dp.counters + kCompactCount, 1);         // (at most one per entry: it fits the compact buffer)
        dp.compact[slot] = dp.table[at];
    }
}

// The VH_SAMPLE_NEAREST sdf and weight at u, by vh_sample.hip's pieces in sample_points_kernel's order (that kernel goes on to
// the gradient with the same runs and is left as it stands).  Called by every lane of the wave.
__device__ __forceinline__ SampleVoxel merge_sample_nearest(const FrameParams &fp, const DevPtrs &dp, int lane, const float u[3],
                                                            bool inDomain)
{
    int r[3] = {0, 0, 0};
    if (inDomain) {
#pragma unroll
        for (int a = 0; a < 3; ++a) r[a] = f2i_rz(u[a] + __builtin_copysignf(0.5f, u[a]));
    }
    const int kx = r[0] >> 3, ky = r[1] >> 3, kz = r[2] >> 3;
    const SampleRuns runs = sample_runs(lane, kx, ky, kz);
    const int resolved = sample_resolve(fp, dp, lane, runs, inDomain, kx, ky, kz);
    return sample_voxel(dp, inDomain ? resolved : VH_FREE_BLOCK, sample_index(r[0], r[1], r[2]));
}

// dst voxel (gx, gy, gz) <- the sample of src at Tinv * (g * vsDst); true: the voxel changed
template <int kMode>
__device__ __forceinline__ bool merge_voxel(const FrameParams &dst, const FrameParams &src, const DevPtrs &srcDp,
                                            const MergeTransform &Tinv, int lane, int gx, int gy, int gz, float &sdfIO, float &wIO)
{
    const float px = (float)gx * dst.voxelSize, py = (float)gy * dst.voxelSize, pz = (float)gz * dst.voxelSize;
    float u[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = merge_row(Tinv.m, r, px, py, pz) / src.voxelSize;
    const bool inDomain = __builtin_fabsf(u[0]) < kSampleDomain && __builtin_fabsf(u[1]) < kSampleDomain &&
                          __builtin_fabsf(u[2]) < kSampleDomain;          // false for NaN
    float s, w;
    if constexpr (kMode == kSampleNearest) {
        const SampleVoxel v = merge_sample_nearest(src, srcDp, lane, u, inDomain);
        s = v.sdf; w = v.weight;
    } else {
        const SampleTrilinear v = sample_trilinear(src, srcDp, lane, u, inDomain);
        s = v.sdf; w = v.weight;
    }
    if (!(s == s) || !(w > 0.0f)) return false;
    s = (s >= 0.0f) ? __builtin_fminf(dst.truncation, s) : __builtin_fmaxf(-dst.truncation, s);
    const float os = sdfIO, ow = wIO;
    if (!(ow > 0.0f)) {
        sdfIO = s;
        wIO = __builtin_fminf(dst.weightMax, w);
    } else {
        sdfIO = ((os * ow) + (s * w)) / (ow + w);                       // combineVoxel's form
        wIO = __builtin_fminf(dst.weightMax, ow + w);
    }
    return true;
}

// One block of dst's compact list per workgroup pass (the list is uniform across the workgroup, so every lane of every wave
// reaches the samples' cross-lane reads).  src is only read.
template <int kMode>
__global__ __launch_bounds__(256) void merge_update_kernel(const FrameParams dst, const DevPtrs dstDp, const FrameParams src,
                                                           const DevPtrs srcDp, const MergeTransform Tinv)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int count = dstDp.counters[kCompactCount];
    for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
        const LaneCell c = lane_cell(dstDp, dstDp.compact[k]);
        float4 v = *c.cell;
        const bool u0 = merge_voxel<kMode>(dst, src, srcDp, Tinv, lane, c.bx, c.by, c.bz, v.x, v.y);
        const bool u1 = merge_voxel<kMode>(dst, src, srcDp, Tinv, lane, c.bx + 1, c.by, c.bz, v.z, v.w);
        if (u0 || u1) *c.cell = v;
    }
}

}  // namespace vh
