// vh_stream.hip -- block streaming between the model and caller memory: vh_stream_out / vh_stream_in (DESIGN.md 4.16;
// include/voxelhash.h states the rule, tests/stream_ref.py is its executable form; Niessner et al. 2013, section 5; no counterpart
// in the reference).  Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after everything else: the scans are
// vh_mesh.hip's, the lookup vh_merge.hip's, the marks and the deletion vh_gc.hip's, the insertion vh_shard.hip's and vh_alloc.hip's.
//   stream_list_kernel<false>  vh_mesh.hip's list walk with the streaming region as predicate: allocated entries inside counted
//   stream_list_kernel<true>   the same walk, entries written in ascending entry index as {x, y, z, ptr}
//   stream_pack_kernel         one workgroup pass per listed block: key + 4 KiB of voxels into a vh_view_record, 16 bytes per lane
//                              (view_pack_kernel's copy), and the 2 KiB of colour words, 8 bytes per lane
//   stream_classify_kernel     one lane per incoming record: FOREIGN, PRESENT, or a record of the key bin the allocation rounds take
//   stream_place_kernel        one workgroup pass per record: the entry looked up, its mark bit taken, the winner's 4 KiB + 2 KiB
//                              copied into the block
#pragma once

namespace vh {

// vh_stream_region as the kernels take it: radius2 = radius * radius, rounded once on the host
struct StreamRegion {
    int kind, invert;
    int lo[3], hi[3];
    float centre[3], radius2;
};
constexpr int kStreamBox = 0, kStreamSphere = 1;               // VH_STREAM_BOX / VH_STREAM_SPHERE
constexpr int kStreamPending = -1;                             // a record the classification left for the rounds
constexpr int kStreamRecordBytes = 4112;                       // sizeof(vh_view_record)

// The selection rule, float32, every operation rounded on its own (the file is built without contraction)
__device__ __forceinline__ bool stream_selected(const int *pos, const StreamRegion &rg, float voxelSize)
{
    bool inside;
    if (rg.kind == kStreamBox) {
        inside = pos[0] >= rg.lo[0] && pos[0] < rg.hi[0] && pos[1] >= rg.lo[1] && pos[1] < rg.hi[1] && pos[2] >= rg.lo[2] &&
                 pos[2] < rg.hi[2];
    } else {
        // (8 * key in wrapping 32-bit arithmetic, as block_in_frustum has it: exact inside the key domain)
        const float x0 = ((float)(int)((uint32_t)pos[0] * 8u) + 3.5f) * voxelSize - rg.centre[0];
        const float x1 = ((float)(int)((uint32_t)pos[1] * 8u) + 3.5f) * voxelSize - rg.centre[1];
        const float x2 = ((float)(int)((uint32_t)pos[2] * 8u) + 3.5f) * voxelSize - rg.centre[2];
        const float d2 = (x0 * x0 + x1 * x1) + x2 * x2;
        inside = d2 <= rg.radius2;
    }
    return inside != (rg.invert != 0);
}

__device__ __forceinline__ bool stream_listed(const VoxelEntry &e, const StreamRegion &rg, float voxelSize)
{
    return e.ptr != VH_FREE_BLOCK && stream_selected(e.pos, rg, voxelSize);
}

// mesh_list_kernel (vh_mesh.hip) for this predicate: one lane per bucket, 64 consecutive buckets per round, every slot looked at
// (with the overflow list an entry may sit anywhere), the lanes' counts put in lane order by a wave scan.
// kWrite = false: sliceCount[wave] = listed entries of the wave's slice.  kWrite = true: they are written from
// tileBase[wave / kMeshScanTile] + sliceCount[wave] (what the scan left there) on.
template <bool kWrite>
__global__ __launch_bounds__(256) void stream_list_kernel(const FrameParams fp, const DevPtrs dp, const StreamRegion rg,
                                                          uint32_t ownedBuckets, uint32_t numSlices, uint32_t *sliceCount,
                                                          const unsigned long long *__restrict__ tileBase, int4 *items,
                                                          uint32_t capacity)
{
    const uint32_t lane = threadIdx.x & 63u, slice = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slice >= numSlices) return;
    uint32_t running = 0;
    if (kWrite) running = (uint32_t)tileBase[slice / kMeshScanTile] + sliceCount[slice];
    const uint32_t first = slice * (uint32_t)kMeshSliceBuckets;
    for (uint32_t r = 0; r < (uint32_t)kMeshSliceBuckets; r += 64u) {
        const uint32_t b = first + r + lane;
        const bool occupied = b < ownedBuckets && ((dp.bucketBits[b >> 5] >> (b & 31u)) & 1u);
        if (__ballot(occupied) == 0ull) continue;
        const VoxelEntry *bucket = dp.table + (size_t)b * fp.bucketSize;
        uint32_t n = 0;
        if (occupied)
            for (uint32_t s = 0; s < fp.bucketSize; ++s) n += stream_listed(bucket[s], rg, fp.voxelSize) ? 1u : 0u;
        uint32_t incl = n;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        if (kWrite && n) {
            uint32_t at = running + incl - n;
            for (uint32_t s = 0; s < fp.bucketSize; ++s) {
                const VoxelEntry e = bucket[s];
                if (!stream_listed(e, rg, fp.voxelSize)) continue;
                if (at < capacity) items[at] = make_int4(e.pos[0], e.pos[1], e.pos[2], e.ptr);
                ++at;
            }
        }
        running += __shfl(incl, 63);
    }
    if (!kWrite && lane == 0) sliceCount[slice] = running;
}

// Record b <- listed block b, b < count (the host has read the list's length): lane t copies voxels 2t, 2t + 1 as one 16-byte
// cell and, with `colors`, their two colour words as one 8-byte cell (zeros where the context has no colour volume).
__global__ __launch_bounds__(256) void stream_pack_kernel(const DevPtrs dp, const uint32_t *__restrict__ color,
                                                          const int4 *__restrict__ items, uint32_t count,
                                                          uint8_t *__restrict__ records, uint32_t *__restrict__ colors)
{
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 it = items[b];
        uint8_t *rec = records + (size_t)b * kStreamRecordBytes;
        if (threadIdx.x == 0) *reinterpret_cast<int4 *>(rec) = make_int4(it.x, it.y, it.z, 0);
        reinterpret_cast<float4 *>(rec + 16)[threadIdx.x] = reinterpret_cast<const float4 *>(dp.blocks + (size_t)it.w)[threadIdx.x];
        if (colors) {
            uint2 w = make_uint2(0u, 0u);
            if (color) w = reinterpret_cast<const uint2 *>(color + (size_t)it.w)[threadIdx.x];
            reinterpret_cast<uint2 *>(colors + (size_t)b * kBlockVoxels)[threadIdx.x] = w;
        }
    }
}

// One lane per record: a key of another shard's bucket range is FOREIGN, a key the table holds PRESENT; the rest stay pending
// and go into the bin (vh_shard.hip: record 0 = {count, 0, 0, 0}, then {x, y, z, rank}; rank = the record, so equal keys are
// told apart).  The bin has room for every record.
__global__ __launch_bounds__(256) void stream_classify_kernel(const FrameParams fp, const DevPtrs dp,
                                                              const uint8_t *__restrict__ records, uint32_t n,
                                                              int32_t *__restrict__ status, int4 *__restrict__ bin)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int4 k = *reinterpret_cast<const int4 *>(records + (size_t)i * kStreamRecordBytes);
    const uint32_t h = hash_block(k.x, k.y, k.z, fp.numBuckets);
    int32_t st = kStreamPending;
    if (h < fp.bucketLo || h >= fp.bucketHi) st = VH_STREAM_FOREIGN;
    else if (merge_find_entry(fp, dp, h - fp.bucketLo, k.x, k.y, k.z) != ~0u) st = VH_STREAM_PRESENT;
    status[i] = st;
    if (st == kStreamPending) bin[atomicAdd(&bin[0].x, 1) + 1] = make_int4(k.x, k.y, k.z, (int)i);
}

// One record per workgroup pass.  A pending record looks its entry up (lane 0): none = UNPLACED; otherwise the entry's mark bit
// decides among the records of one key -- the record that sets it copies its 4 KiB (and its 2 KiB of colour) into the block,
// whole, the others are PRESENT.  totals[status] counts every record of the call.  The host clears the marks behind the launch.
__global__ __launch_bounds__(256) void stream_place_kernel(const FrameParams fp, const DevPtrs dp, uint32_t *__restrict__ color,
                                                           const uint8_t *__restrict__ records,
                                                           const uint32_t *__restrict__ colors, uint32_t n,
                                                           int32_t *__restrict__ status, unsigned long long *__restrict__ totals)
{
    __shared__ int sPtr;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint8_t *rec = records + (size_t)r * kStreamRecordBytes;
        if (threadIdx.x == 0) {
            int32_t st = status[r];
            int ptr = VH_FREE_BLOCK;
            if (st == kStreamPending) {
                const int4 k = *reinterpret_cast<const int4 *>(rec);
                const uint32_t h = hash_block(k.x, k.y, k.z, fp.numBuckets);     // (inside the bucket range: it was classified)
                const uint32_t at = merge_find_entry(fp, dp, h - fp.bucketLo, k.x, k.y, k.z);
                if (at == ~0u) {
                    st = VH_STREAM_UNPLACED;
                } else {
                    const uint32_t bit = 1u << (at & 31u);
                    if (atomicOr(dp.gcMarks + (at >> 5), bit) & bit) {
                        st = VH_STREAM_PRESENT;
                    } else {
                        st = VH_STREAM_PLACED;
                        ptr = dp.table[at].ptr;
                    }
                }
                status[r] = st;
            }
            atomicAdd(totals + st, 1ull);
            sPtr = ptr;
        }
        __syncthreads();
        const int ptr = sPtr;
        if (ptr != VH_FREE_BLOCK) {
            reinterpret_cast<float4 *>(dp.blocks + (size_t)ptr)[threadIdx.x] = reinterpret_cast<const float4 *>(rec + 16)[threadIdx.x];
            if (colors)
                reinterpret_cast<uint2 *>(color + (size_t)ptr)[threadIdx.x] =
                    reinterpret_cast<const uint2 *>(colors + (size_t)r * kBlockVoxels)[threadIdx.x];
        }
        __syncthreads();                         // (sPtr is free for the next pass)
    }
}

}  // namespace vh
