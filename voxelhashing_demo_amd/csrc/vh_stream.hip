// vh_stream.hip -- block streaming between the model and caller memory: vh_stream_out / vh_stream_in (DESIGN.md 4.16;
// include/voxelhash.h states the rule, tests/stream_ref.py is its executable form; Niessner et al. 2013, section 5; no counterpart
// in the reference).  Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after everything else: the list and its
// scans are vh_blocklist.hip's, the lookup vh_merge.hip's, the marks and the deletion vh_gc.hip's, the insertion vh_shard.hip's and vh_alloc.hip's.
//   (vh_blocklist.hip          the ordered block list with the streaming region, a StreamSelect, as predicate)
//   stream_pack_kernel         one workgroup pass per listed block: key + 4 KiB of voxels into a vh_view_record, 16 bytes per lane
//                              (view_pack_kernel's copy), and the 2 KiB of colour words, 8 bytes per lane
//   stream_classify_kernel     one lane per incoming record: FOREIGN, PRESENT, or a record of the key bin the allocation rounds take
//   stream_place_kernel        one workgroup pass per record: the entry looked up, its mark bit taken, the winner's 4 KiB + 2 KiB
//                              copied into the block
#pragma once

namespace vh {

constexpr int kStreamBox = 0, kStreamSphere = 1;               // VH_STREAM_BOX / VH_STREAM_SPHERE
constexpr int kStreamPending = -1;                             // a record the classification left for the rounds
constexpr int kStreamRecordBytes = 4112;                       // sizeof(vh_view_record)

// vh_stream_region as the list walk takes it, its predicate: radius2 = radius * radius, rounded once on the host
struct StreamSelect {
    int kind, invert;
    BlockBox box;
    float centre[3], radius2, voxelSize;
    __device__ __forceinline__ bool operator()(const VoxelEntry &e) const;
};

// The selection rule, float32, every operation rounded on its own (the file is built without contraction)
__device__ __forceinline__ bool stream_selected(const int *pos, const StreamSelect &rg)
{
    bool inside;
    if (rg.kind == kStreamBox) {
        inside = rg.box.holds(pos[0], pos[1], pos[2]);
    } else {
        // (8 * key in wrapping 32-bit arithmetic, as block_in_frustum has it: exact inside the key domain)
        const float x0 = ((float)(int)((uint32_t)pos[0] * 8u) + 3.5f) * rg.voxelSize - rg.centre[0];
        const float x1 = ((float)(int)((uint32_t)pos[1] * 8u) + 3.5f) * rg.voxelSize - rg.centre[1];
        const float x2 = ((float)(int)((uint32_t)pos[2] * 8u) + 3.5f) * rg.voxelSize - rg.centre[2];
        const float d2 = (x0 * x0 + x1 * x1) + x2 * x2;
        inside = d2 <= rg.radius2;
    }
    return inside != (rg.invert != 0);
}

__device__ __forceinline__ bool StreamSelect::operator()(const VoxelEntry &e) const
{
    return e.ptr != VH_FREE_BLOCK && stream_selected(e.pos, *this);
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
