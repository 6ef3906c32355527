// vh_mesh.hip -- iso-surface extraction: the fused TSDF as a triangle list (vh_extract_mesh; DESIGN.md "mesh").
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_raycast.hip (lookup_block).
//
// Marching tetrahedra on the Kuhn split of every cell whose eight corner voxels are valid (block allocated, weight > 0;
// inside iff sdf <= 0).  The output order is fixed -- blocks in ascending entry index, cells in ascending voxel index,
// tetrahedra 0..5, triangles in table order -- so nothing here takes an output slot with a bare atomicAdd:
//   mesh_list_kernel<false>   per-wave slice of the bucket range: allocated entries (inside the region) counted
//   mesh_scan_*               exclusive scan of the slice counts
//   mesh_list_kernel<true>    the same walk, entries written in order: the block list
//   mesh_block_kernel<.., false>   one workgroup pass per listed block: 9^3 apron in LDS, triangles of the block counted
//   mesh_scan_*               exclusive scan of the block counts (64-bit offsets)
//   mesh_block_kernel<.., true>    the same pass, triangles (and normals) written at offset[block] + in-block prefix
#pragma once

#include "vh_mesh_table.h"

namespace vh {

struct MeshRegion { int lo[3], hi[3]; };       // blocks lo <= k < hi

constexpr int kMeshSliceBuckets = 1024;        // buckets per wave of the list walk (16 rounds of 64)
constexpr int kMeshScanTile = 1024;            // elements per workgroup of the scan's first level
constexpr int kApronSide = 9, kApronVoxels = 9 * 9 * 9;

// ---------------------------------------------------------------------------
// the block list
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool mesh_listed(const VoxelEntry &e, const MeshRegion &rg)
{
    return e.ptr != VH_FREE_BLOCK && e.pos[0] >= rg.lo[0] && e.pos[0] < rg.hi[0] && e.pos[1] >= rg.lo[1] &&
           e.pos[1] < rg.hi[1] && e.pos[2] >= rg.lo[2] && e.pos[2] < rg.hi[2];
}

// One lane per bucket, 64 consecutive buckets per round: a lane looks at the slots of its bucket in order (with the overflow
// list an entry may sit anywhere, so every slot is looked at), and the lanes' counts are put in lane order by a wave scan.
// kWrite = false: sliceCount[wave] = listed entries of the wave's slice.  kWrite = true: they are written from
// tileBase[wave / kMeshScanTile] + sliceCount[wave] (what the scan left there) on, as {x, y, z, ptr}.
template <bool kWrite>
__global__ __launch_bounds__(256) void mesh_list_kernel(const FrameParams fp, const DevPtrs dp, const MeshRegion rg,
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
            for (uint32_t s = 0; s < fp.bucketSize; ++s) n += mesh_listed(bucket[s], rg) ? 1u : 0u;
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
                if (!mesh_listed(e, rg)) continue;
                if (at < capacity) items[at] = make_int4(e.pos[0], e.pos[1], e.pos[2], e.ptr);
                ++at;
            }
        }
        running += __shfl(incl, 63);
    }
    if (!kWrite && lane == 0) sliceCount[slice] = running;
}

// ---------------------------------------------------------------------------
// exclusive scan, two levels: tiles of kMeshScanTile counts in place (32-bit prefixes inside the tile, the tile's total as
// 64 bits), then one workgroup over the tile totals.  n = *nPtr when nPtr is given (a length only the device knows).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mesh_wg_scan(uint32_t v, uint32_t *sWave, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += (w < wave) ? sWave[w] : 0u;
    total = sWave[0] + sWave[1] + sWave[2] + sWave[3];
    __syncthreads();                      // (sWave is free for the caller's next scan)
    return before + incl - v;             // exclusive
}

__global__ __launch_bounds__(256) void mesh_scan_tiles_kernel(uint32_t *counts, const unsigned long long *nPtr, uint32_t nHost,
                                                              unsigned long long *tileTotal)
{
    __shared__ uint32_t sWave[4];
    const uint32_t n = nPtr ? (uint32_t)*nPtr : nHost;
    const uint32_t base = blockIdx.x * (uint32_t)kMeshScanTile + threadIdx.x * 4u;
    if (blockIdx.x * (uint32_t)kMeshScanTile >= n) return;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < n ? counts[base + k] : 0u; sum += v[k]; }
    uint32_t total;
    uint32_t at = mesh_wg_scan(sum, sWave, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < n) counts[base + k] = at; at += v[k]; }
    if (threadIdx.x == 0) tileTotal[blockIdx.x] = total;
}

// one workgroup: tileTotal[0 .. ceil(n / kMeshScanTile)) becomes its exclusive scan, *totalOut the sum (at most `cap`: a list's length)
__global__ __launch_bounds__(256) void mesh_scan_totals_kernel(unsigned long long *tileTotal, const unsigned long long *nPtr,
                                                               uint32_t nHost, unsigned long long cap, unsigned long long *totalOut)
{
    __shared__ unsigned long long sWave[4];
    const uint32_t n = nPtr ? (uint32_t)*nPtr : nHost;
    const uint32_t tiles = (n + (uint32_t)kMeshScanTile - 1u) / (uint32_t)kMeshScanTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += 256u) {
        const uint32_t t = t0 + threadIdx.x;
        const unsigned long long v = t < tiles ? tileTotal[t] : 0ull;
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
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

// ---------------------------------------------------------------------------
// one block
// ---------------------------------------------------------------------------
// sdf of a voxel, NaN where the voxel is not valid (block absent or weight 0).  A stored NaN sdf counts as not valid too.
__device__ __forceinline__ float mesh_voxel(const DevPtrs &dp, int ptr, int index)
{
    if (ptr == VH_FREE_BLOCK) return __builtin_nanf("");
    const Voxel v = dp.blocks[(size_t)ptr + (size_t)index];
    return v.weight > 0.0f ? v.sdf : __builtin_nanf("");
}

// Where the corners of the block's cells come from.  Local coordinates 0..8 (8 = first layer of the +neighbour).
struct MeshApron {            // the 9^3 samples staged in LDS
    const float *s;
    __device__ __forceinline__ float at(int x, int y, int z) const { return s[(z * kApronSide + y) * kApronSide + x]; }
};
struct MeshDirect {           // straight from global memory through the 27 resolved neighbour pointers
    const DevPtrs &dp;
    const int *nb;            // [3][3][3], offsets -1..1
    __device__ __forceinline__ float at(int x, int y, int z) const
    {
        const int p = nb[((z >> 3) + 1) * 9 + ((y >> 3) + 1) * 3 + ((x >> 3) + 1)];
        return mesh_voxel(dp, p, ((z & 7) << 6) | ((y & 7) << 3) | (x & 7));
    }
};

// triangles of a tetrahedron by the number of inside slots: 0 1 1 2 1 2 2 1 1 2 2 1 2 1 1 0, two bits each
constexpr uint32_t kMeshTriCount = 0x16696994u;

// mask of inside corners of cell (x,y,z), 0 when a corner is not valid (0 and 255 emit nothing)
template <class Src>
__device__ __forceinline__ uint32_t mesh_cell_mask(const Src &src, int x, int y, int z)
{
    uint32_t mask = 0;
    bool valid = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float s = src.at(x + (i & 1), y + ((i >> 1) & 1), z + (i >> 2));
        valid = valid && (s == s);
        mask |= (s <= 0.0f ? 1u : 0u) << i;
    }
    return valid ? mask : 0u;
}

__device__ __forceinline__ uint32_t mesh_tet_mask(uint32_t cell, uint32_t corners)
{
    return (cell & 1u) | (((cell >> ((corners >> 8) & 7u)) & 1u) << 1) | (((cell >> ((corners >> 16) & 7u)) & 1u) << 2) |
           ((cell >> 7) << 3);
}

__device__ __forceinline__ uint32_t mesh_cell_count(uint32_t cell)
{
    if (cell == 0u || cell == 255u) return 0u;
    uint32_t n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) n += (kMeshTriCount >> (2u * mesh_tet_mask(cell, kMeshTet[t]))) & 3u;
    return n;
}

// TSDF gradient at local voxel (x,y,z), the rule of dda_normal (central difference where both neighbours are valid, one-sided
// where one is, else none), not normalised.  The voxel itself is valid (a corner of an emitting cell).
__device__ __forceinline__ bool mesh_gradient(const MeshDirect &src, int x, int y, int z, float here, float g[3])
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float sp = src.at(x + (a == 0), y + (a == 1), z + (a == 2));
        const float sm = src.at(x - (a == 0), y - (a == 1), z - (a == 2));
        const bool hp = sp == sp, hm = sm == sm;
        g[a] = 0.0f;
        if (hp && hm) g[a] = (sp - sm) * 0.5f;
        else if (hp) g[a] = sp - here;
        else if (hm) g[a] = here - sm;
        else ok = false;
    }
    return ok;
}

// The vertex on the edge between cell corners ca and cb (ca a subset of cb as bit sets: ca is componentwise the smaller voxel).
// Always from ca to cb, so the bits depend on the edge alone.
template <class Src, bool kNormals>
__device__ __forceinline__ void mesh_vertex(const FrameParams &fp, const Src &src, const MeshDirect &far, const int4 &item, int x,
                                            int y, int z, uint32_t ca, uint32_t cb, float *pos, float *nrm)
{
    const int ax = x + (int)(ca & 1u), ay = y + (int)((ca >> 1) & 1u), az = z + (int)(ca >> 2);
    const int bx = x + (int)(cb & 1u), by = y + (int)((cb >> 1) & 1u), bz = z + (int)(cb >> 2);
    const float sA = src.at(ax, ay, az), sB = src.at(bx, by, bz);
    const float t = sA / (sA - sB);
    const uint32_t d = ca ^ cb;
    const float gx = (float)((int)((uint32_t)item.x * 8u) + ax), gy = (float)((int)((uint32_t)item.y * 8u) + ay),
                gz = (float)((int)((uint32_t)item.z * 8u) + az);
    pos[0] = ((d & 1u) ? gx + t : gx) * fp.voxelSize;
    pos[1] = ((d & 2u) ? gy + t : gy) * fp.voxelSize;
    pos[2] = ((d & 4u) ? gz + t : gz) * fp.voxelSize;
    if (kNormals) {
        float gA[3], gB[3];
        const bool okA = mesh_gradient(far, ax, ay, az, sA, gA), okB = mesh_gradient(far, bx, by, bz, sB, gB), ok = okA && okB;
        const float nx = gA[0] + t * (gB[0] - gA[0]), ny = gA[1] + t * (gB[1] - gA[1]), nz = gA[2] + t * (gB[2] - gA[2]);
        const float len = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
        const bool good = ok && len > 0.0f;
        nrm[0] = good ? nx / len : 0.0f;
        nrm[1] = good ? ny / len : 0.0f;
        nrm[2] = good ? nz / len : 0.0f;
    }
}

template <class Src, bool kNormals>
__device__ __forceinline__ void mesh_emit_cell(const FrameParams &fp, const Src &src, const MeshDirect &far, const int4 &item,
                                               int cellIndex, uint32_t cell, unsigned long long at,
                                               unsigned long long capacity, float *__restrict__ positions,
                                               float *__restrict__ normals)
{
    const int x = cellIndex & 7, y = (cellIndex >> 3) & 7, z = cellIndex >> 6;
    for (int t = 0; t < 6; ++t) {
        const uint32_t corners = kMeshTet[t];
        uint32_t word = kMeshTable[t][mesh_tet_mask(cell, corners)];
        const uint32_t n = word & 3u;
        word >>= 2;
        for (uint32_t k = 0; k < n; ++k, ++at) {
            if (at >= capacity) return;
            float p[9], q[9];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t e = word & 15u;
                word >>= 4;
                mesh_vertex<Src, kNormals>(fp, src, far, item, x, y, z, (corners >> (8u * (e & 3u))) & 7u,
                                           (corners >> (8u * (e >> 2))) & 7u, p + 3 * j, q + 3 * j);
            }
            float *out = positions + at * 9ull;
#pragma unroll
            for (int j = 0; j < 9; ++j) out[j] = p[j];
            if (kNormals) {
                float *no = normals + at * 9ull;
#pragma unroll
                for (int j = 0; j < 9; ++j) no[j] = q[j];
            }
        }
    }
}

// One listed block per workgroup pass, two x-neighbouring cells per lane (cells 2*tid and 2*tid + 1, so that lane order is
// cell order).  kApron: the block's 512 voxels (one 16-byte load per lane) and the 217 voxels of the first layer of its seven
// +neighbours are staged in LDS as one float each (2.9 KB); otherwise every corner is read from global memory.
// kEmit = false: blockCount[b] = triangles of the block.  kEmit = true: blockCount holds the scanned offsets, and the
// triangles are written at tileBase[b / tile] + blockCount[b] + (prefix of the cells before), clipped at `capacity`.
template <bool kApron, bool kEmit, bool kNormals>
__global__ __launch_bounds__(256) void mesh_block_kernel(const FrameParams fp, const DevPtrs dp, const int4 *__restrict__ items,
                                                         const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                         uint32_t *blockCount, const unsigned long long *__restrict__ tileBase,
                                                         unsigned long long capacity, float *__restrict__ positions,
                                                         float *__restrict__ normals)
{
    __shared__ float sApron[kApron ? kApronVoxels : 1];
    __shared__ int sNb[27];
    __shared__ uint32_t sWave[4];
    const uint32_t count = min((uint32_t)*numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        // neighbour blocks through the hash: the 7 towards +x/+y/+z for the cells, all 26 for the normals' gradients
        if (tid < 27) {
            const int ox = tid % 3 - 1, oy = (tid / 3) % 3 - 1, oz = tid / 9 - 1;
            int p = VH_FREE_BLOCK;
            if (tid == 13) p = item.w;
            else if (kNormals || (ox >= 0 && oy >= 0 && oz >= 0)) p = lookup_block(fp, dp, item.x + ox, item.y + oy, item.z + oz);
            sNb[tid] = p;
        }
        __syncthreads();
        const MeshDirect direct{dp, sNb};
        if (kApron) {
            const float4 v = *reinterpret_cast<const float4 *>(dp.blocks + (size_t)item.w + 2 * tid);
            const int i0 = 2 * tid, x0 = i0 & 7, y0 = (i0 >> 3) & 7, z0 = i0 >> 6;
            float *row = sApron + (z0 * kApronSide + y0) * kApronSide + x0;
            row[0] = v.y > 0.0f ? v.x : __builtin_nanf("");
            row[1] = v.w > 0.0f ? v.z : __builtin_nanf("");
            for (int i = tid; i < kApronVoxels; i += 256) {
                const int x = i % kApronSide, y = (i / kApronSide) % kApronSide, z = i / (kApronSide * kApronSide);
                if (x == 8 || y == 8 || z == 8) sApron[i] = direct.at(x, y, z);
            }
            __syncthreads();
        }
        uint32_t c0, c1, m0, m1;
        const int x = (2 * tid) & 7, y = (tid >> 2) & 7, z = tid >> 5;
        if (kApron) {
            const MeshApron src{sApron};
            m0 = mesh_cell_mask(src, x, y, z);
            m1 = mesh_cell_mask(src, x + 1, y, z);
        } else {
            m0 = mesh_cell_mask(direct, x, y, z);
            m1 = mesh_cell_mask(direct, x + 1, y, z);
        }
        c0 = mesh_cell_count(m0);
        c1 = mesh_cell_count(m1);
        uint32_t total;
        const uint32_t before = mesh_wg_scan(c0 + c1, sWave, total);      // (its barriers also fence sNb / sApron for the next pass)
        if (!kEmit) {
            if (tid == 0) blockCount[b] = total;
        } else if (total) {
            const unsigned long long at = tileBase[b / (uint32_t)kMeshScanTile] + blockCount[b] + before;
            if (kApron) {
                const MeshApron src{sApron};
                if (c0) mesh_emit_cell<MeshApron, kNormals>(fp, src, direct, item, 2 * tid, m0, at, capacity, positions, normals);
                if (c1) mesh_emit_cell<MeshApron, kNormals>(fp, src, direct, item, 2 * tid + 1, m1, at + c0, capacity, positions, normals);
            } else {
                if (c0) mesh_emit_cell<MeshDirect, kNormals>(fp, direct, direct, item, 2 * tid, m0, at, capacity, positions, normals);
                if (c1) mesh_emit_cell<MeshDirect, kNormals>(fp, direct, direct, item, 2 * tid + 1, m1, at + c0, capacity, positions, normals);
            }
            __syncthreads();              // the emitters read sApron / sNb: not before they are done may the next pass overwrite them
        }
    }
}

}  // namespace vh
