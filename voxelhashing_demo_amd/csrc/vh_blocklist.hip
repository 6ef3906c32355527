// vh_blocklist.hip -- the ordered block list and its scans: the front end of every call that reads the model block by block
// in a fixed order (vh_extract_mesh, vh_extract_mesh_indexed, vh_components / vh_remove_components, vh_stream_out).
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip ahead of vh_mesh.hip.
//
// The order is ascending entry index, so nothing here takes an output slot with a bare atomicAdd:
//   block_list_kernel<false>   per-wave slice of the bucket range: the entries the predicate selects, counted
//   block_scan_*               exclusive scan of the slice counts
//   block_list_kernel<true>    the same walk, entries written in order as {x, y, z, ptr}: the block list
// The callers' per-block rounds (count -> block_scan_* -> emit over the listed blocks) use the same scans.
#pragma once

namespace vh {

constexpr int kListSliceBuckets = 1024;        // buckets per wave of the list walk (16 rounds of 64)
constexpr int kScanTile = 1024;                // elements per workgroup of the scan's first level

// The predicate of the mesh and the components: allocated entries of the blocks lo <= k < hi
struct BlockBox {
    int lo[3], hi[3];
    __device__ __forceinline__ bool holds(int x, int y, int z) const
    {
        return x >= lo[0] && x < hi[0] && y >= lo[1] && y < hi[1] && z >= lo[2] && z < hi[2];
    }
    __device__ __forceinline__ bool operator()(const VoxelEntry &e) const
    {
        return e.ptr != VH_FREE_BLOCK && holds(e.pos[0], e.pos[1], e.pos[2]);
    }
};

// inclusive scan over the 64 lanes of a wave
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// what the two-level scan left for element i: its tile's base plus its prefix inside the tile
__device__ __forceinline__ unsigned long long scanned_at(const unsigned long long *__restrict__ tileBase, const uint32_t *counts,
                                                         uint32_t i)
{
    return tileBase[i / (uint32_t)kScanTile] + counts[i];
}

// One lane per bucket, 64 consecutive buckets per round: a lane looks at the slots of its bucket in order (with the overflow
// list an entry may sit anywhere, so every slot is looked at), and the lanes' counts are put in lane order by a wave scan.
// kWrite = false: sliceCount[wave] = selected entries of the wave's slice.  kWrite = true: they are written from
// tileBase[wave / kScanTile] + sliceCount[wave] (what the scan left there) on, as {x, y, z, ptr}.
template <bool kWrite, class Pred>
__global__ __launch_bounds__(256) void block_list_kernel(const FrameParams fp, const DevPtrs dp, const Pred pred,
                                                         uint32_t ownedBuckets, uint32_t numSlices, uint32_t *sliceCount,
                                                         const unsigned long long *__restrict__ tileBase, int4 *items,
                                                         uint32_t capacity)
{
    const uint32_t lane = threadIdx.x & 63u, slice = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slice >= numSlices) return;
    uint32_t running = 0;
    if (kWrite) running = (uint32_t)scanned_at(tileBase, sliceCount, slice);
    const uint32_t first = slice * (uint32_t)kListSliceBuckets;
    for (uint32_t r = 0; r < (uint32_t)kListSliceBuckets; r += 64u) {
        const uint32_t b = first + r + lane;
        const bool occupied = b < ownedBuckets && ((dp.bucketBits[b >> 5] >> (b & 31u)) & 1u);
        if (__ballot(occupied) == 0ull) continue;
        const VoxelEntry *bucket = dp.table + (size_t)b * fp.bucketSize;
        uint32_t n = 0;
        if (occupied)
            for (uint32_t s = 0; s < fp.bucketSize; ++s) n += pred(bucket[s]) ? 1u : 0u;
        const uint32_t incl = wave_inclusive_scan(n, (int)lane);
        if (kWrite && n) {
            uint32_t at = running + incl - n;
            for (uint32_t s = 0; s < fp.bucketSize; ++s) {
                const VoxelEntry e = bucket[s];
                if (!pred(e)) continue;
                if (at < capacity) items[at] = make_int4(e.pos[0], e.pos[1], e.pos[2], e.ptr);
                ++at;
            }
        }
        running += __shfl(incl, 63);
    }
    if (!kWrite && lane == 0) sliceCount[slice] = running;
}

// ---------------------------------------------------------------------------
// exclusive scan, two levels: tiles of kScanTile counts in place (32-bit prefixes inside the tile, the tile's total as
// 64 bits), then one workgroup over the tile totals.  n = *nPtr when nPtr is given (a length only the device knows).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_wg_scan(uint32_t v, uint32_t *sWave, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(v, lane);
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += (w < wave) ? sWave[w] : 0u;
    total = sWave[0] + sWave[1] + sWave[2] + sWave[3];
    __syncthreads();                      // (sWave is free for the caller's next scan)
    return before + incl - v;             // exclusive
}

__global__ __launch_bounds__(256) void block_scan_tiles_kernel(uint32_t *counts, const unsigned long long *nPtr, uint32_t nHost,
                                                               unsigned long long *tileTotal)
{
    __shared__ uint32_t sWave[4];
    const uint32_t n = nPtr ? (uint32_t)*nPtr : nHost;
    const uint32_t base = blockIdx.x * (uint32_t)kScanTile + threadIdx.x * 4u;
    if (blockIdx.x * (uint32_t)kScanTile >= n) return;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < n ? counts[base + k] : 0u; sum += v[k]; }
    uint32_t total;
    uint32_t at = block_wg_scan(sum, sWave, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < n) counts[base + k] = at; at += v[k]; }
    if (threadIdx.x == 0) tileTotal[blockIdx.x] = total;
}

// one workgroup: tileTotal[0 .. ceil(n / kScanTile)) becomes its exclusive scan, *totalOut the sum (at most `cap`: a list's length)
__global__ __launch_bounds__(256) void block_scan_totals_kernel(unsigned long long *tileTotal, const unsigned long long *nPtr,
                                                                uint32_t nHost, unsigned long long cap, unsigned long long *totalOut)
{
    __shared__ unsigned long long sWave[4];
    const uint32_t n = nPtr ? (uint32_t)*nPtr : nHost;
    const uint32_t tiles = (n + (uint32_t)kScanTile - 1u) / (uint32_t)kScanTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += 256u) {
        const uint32_t t = t0 + threadIdx.x;
        const unsigned long long v = t < tiles ? tileTotal[t] : 0ull;
        const unsigned long long incl = wave_inclusive_scan(v, lane);
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += sWave[w];
        if (t < tiles) tileTotal[t] = before + incl - v;
        carry += sWave[0] + sWave[1] + sWave[2] + sWave[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *totalOut = carry < cap ? carry : cap;
}

}  // namespace vh
