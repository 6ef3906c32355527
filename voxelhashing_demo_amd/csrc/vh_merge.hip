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
//   merge_color_update_kernel   the same launch with the colour step in it (vh_merge_color): the sample's blocks
//                          resolved once, both of src's volumes read through those pointers, the colour pair one 8-byte cell
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

// The point of src that dst voxel (gx, gy, gz) is sampled at, u = Tinv * (g * vsDst) / vsSrc; returns inDomain
__device__ __forceinline__ bool merge_source_point(const FrameParams &dst, const FrameParams &src, const MergeTransform &Tinv, int gx,
                                                   int gy, int gz, float u[3])
{
    const float px = (float)gx * dst.voxelSize, py = (float)gy * dst.voxelSize, pz = (float)gz * dst.voxelSize;
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = merge_row(Tinv.m, r, px, py, pz) / src.voxelSize;
    return __builtin_fabsf(u[0]) < kSampleDomain && __builtin_fabsf(u[1]) < kSampleDomain &&
           __builtin_fabsf(u[2]) < kSampleDomain;                       // false for NaN
}

// src's sample (s, w) combined into a dst voxel; false: no sample, the voxel stays
__device__ __forceinline__ bool merge_combine(const FrameParams &dst, float s, float w, float &sdfIO, float &wIO)
{
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

// dst voxel (gx, gy, gz) <- the sample of src at its source point; true: the voxel changed.  Called by every lane of the wave.
template <int kMode>
__device__ __forceinline__ bool merge_voxel(const FrameParams &dst, const FrameParams &src, const DevPtrs &srcDp,
                                            const MergeTransform &Tinv, int lane, int gx, int gy, int gz, float &sdfIO, float &wIO)
{
    float u[3];
    const bool inDomain = merge_source_point(dst, src, Tinv, gx, gy, gz, u);
    float s, w;
    if constexpr (kMode == kSampleNearest) {
        const SampleNearest n = sample_nearest_block(src, srcDp, lane, u, inDomain);
        const SampleVoxel v = sample_voxel(srcDp, n.ptr, sample_index(n.r[0], n.r[1], n.r[2]));
        s = v.sdf; w = v.weight;
    } else {
        const SampleTrilinear v = sample_trilinear(src, srcDp, sample_cell(src, srcDp, lane, u, inDomain), inDomain);
        s = v.sdf; w = v.weight;
    }
    return merge_combine(dst, s, w, sdfIO, wIO);
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

// ---- geometry and colour in one launch: vh_merge_color (the rule: include/voxelhash.h, tests/merge_color_ref.py) ----
// The sample's source blocks are resolved once and both of src's volumes are read through those pointers: the TSDF sample is
// merge_voxel's (the same bits), the colour sample reads the words beside the voxels it used.  The colour volumes are no
// members of DevPtrs (vh_color.hip): they travel as kernel arguments.

// src's colour sample combined into dst's word c; wIn > 0
__device__ __forceinline__ uint32_t merge_color_word(uint32_t c, uint32_t rgb, uint32_t wIn, uint32_t weightMax)
{
    const uint32_t wd = c >> 24;
    if (wd == 0u) return rgb | (min(wIn, weightMax) << 24);
    const float fd = (float)wd, fs = (float)wIn, den = (float)(wd + wIn);
    uint32_t out = min(wd + wIn, weightMax) << 24;
#pragma unroll
    for (int k = 0; k < 24; k += 8) {
        const float f = ((float)((c >> k) & 255u) * fd + (float)((rgb >> k) & 255u) * fs) / den;
        out |= (uint32_t)(f + 0.5f) << k;       // (at most 255: a weighted mean of bytes)
    }
    return out;
}

// The VH_SAMPLE_TRILINEAR sdf, weight and colour at u: sample_trilinear's sdf and weight, and the colour words of the cell's
// corners (vh_sample.hip), the channels one at a time over the eight words so that no more than those stay live.  count == 0:
// no colour sample.  Called by every lane of the wave.
struct MergeColorSample { float sdf, weight; uint32_t rgb, count; };

__device__ __forceinline__ MergeColorSample merge_color_trilinear(const FrameParams &fp, const DevPtrs &dp,
                                                                  const uint32_t *__restrict__ color, int lane, const float u[3],
                                                                  bool inDomain)
{
    const SampleCell cell = sample_cell(fp, dp, lane, u, inDomain);
    const SampleTrilinear t = sample_trilinear(fp, dp, cell, inDomain);
    MergeColorSample r = {t.sdf, t.weight, 0u, 0u};
    if (!(r.weight > 0.0f)) return r;           // (no TSDF step, so no colour step: the words are not read)
    // a sample, so eight valid corners: every ptr names a block, inside src's colour volume as it is inside its SDF volume
    uint32_t w[8], least = 255u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        w[c] = color[(size_t)cell.ptr[c] + (size_t)sample_cell_index(cell, c)];
        least = min(least, w[c] >> 24);
    }
    if (least == 0u) return r;
    r.count = least;
#pragma unroll
    for (int k = 0; k < 24; k += 8) {
        float s[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) s[c] = (float)((w[c] >> k) & 255u);
        r.rgb |= (uint32_t)(cell_lerp(s, cell.t) + 0.5f) << k;
    }
    return r;
}

// the VH_SAMPLE_NEAREST form: the voxel and the word beside it
__device__ __forceinline__ MergeColorSample merge_color_nearest(const FrameParams &fp, const DevPtrs &dp,
                                                                const uint32_t *__restrict__ color, int lane, const float u[3],
                                                                bool inDomain)
{
    const SampleNearest n = sample_nearest_block(fp, dp, lane, u, inDomain);
    const int index = sample_index(n.r[0], n.r[1], n.r[2]);
    const SampleVoxel v = sample_voxel(dp, n.ptr, index);
    MergeColorSample out = {v.sdf, v.weight, 0u, 0u};
    if (v.sdf == v.sdf) {                       // (a valid voxel: ptr names a block)
        const uint32_t word = color[(size_t)n.ptr + (size_t)index];
        out.rgb = word & 0xffffffu;
        out.count = word >> 24;
    }
    return out;
}

// merge_voxel with the colour step behind it: bit 0 = the voxel changed, bit 1 = the word did
template <int kMode>
__device__ __forceinline__ int merge_color_voxel(const FrameParams &dst, const FrameParams &src, const DevPtrs &srcDp,
                                                 const uint32_t *__restrict__ srcColor, const MergeTransform &Tinv, int lane,
                                                 uint32_t weightMax, int gx, int gy, int gz, float &sdfIO, float &wIO, uint32_t &cIO)
{
    float u[3];
    const bool inDomain = merge_source_point(dst, src, Tinv, gx, gy, gz, u);
    MergeColorSample v;
    if constexpr (kMode == kSampleNearest) v = merge_color_nearest(src, srcDp, srcColor, lane, u, inDomain);
    else v = merge_color_trilinear(src, srcDp, srcColor, lane, u, inDomain);
    if (!merge_combine(dst, v.sdf, v.weight, sdfIO, wIO)) return 0;
    if (v.count == 0u) return 1;
    const uint32_t c = merge_color_word(cIO, v.rgb, v.count, weightMax);
    const int changed = c != cIO ? 3 : 1;
    cIO = c;
    return changed;
}

// merge_update_kernel's shape: one block of dst's compact list per workgroup pass, lane t voxels 2t and 2t + 1 -- the TSDF pair
// one 16-byte load and store, the colour pair one 8-byte load and store, each stored only when something in it changed.  No
// lane leaves before the samples' cross-lane reads.  src's two volumes are only read.
template <int kMode>
__global__ __launch_bounds__(256) void merge_color_update_kernel(const FrameParams dst, const DevPtrs dstDp, uint32_t *__restrict__ dstColor,
                                                                 const FrameParams src, const DevPtrs srcDp,
                                                                 const uint32_t *__restrict__ srcColor, const MergeTransform Tinv,
                                                                 uint32_t weightMax)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int count = dstDp.counters[kCompactCount];
    for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) {
        const VoxelEntry e = dstDp.compact[k];
        const LaneCell c = lane_cell(dstDp, e);
        float4 v = *c.cell;
        uint2 *words = reinterpret_cast<uint2 *>(dstColor + (size_t)e.ptr + 2 * threadIdx.x);
        uint2 w = *words;
        const int u0 = merge_color_voxel<kMode>(dst, src, srcDp, srcColor, Tinv, lane, weightMax, c.bx, c.by, c.bz, v.x, v.y, w.x);
        const int u1 = merge_color_voxel<kMode>(dst, src, srcDp, srcColor, Tinv, lane, weightMax, c.bx + 1, c.by, c.bz, v.z, v.w, w.y);
        if ((u0 | u1) & 1) *c.cell = v;
        if ((u0 | u1) & 2) *words = w;
    }
}

}  // namespace vh
