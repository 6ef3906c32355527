// vh_mesh.hip -- iso-surface extraction: the fused TSDF as a triangle list (vh_extract_mesh; DESIGN.md "mesh").
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_raycast.hip (lookup_block) and vh_blocklist.hip.
//
// Marching tetrahedra on the Kuhn split of every cell whose eight corner voxels are valid (block allocated, weight > 0;
// inside iff sdf <= 0).  The output order is fixed -- blocks in ascending entry index, cells in ascending voxel index,
// tetrahedra 0..5, triangles in table order -- so nothing here takes an output slot with a bare atomicAdd:
//   (vh_blocklist.hip              the ordered block list with the region, a BlockBox, as predicate)
//   mesh_block_kernel<.., false>   one workgroup pass per listed block: 9^3 apron in LDS, triangles of the block counted
//   block_scan_*                   exclusive scan of the block counts (64-bit offsets)
//   mesh_block_kernel<.., true>    the same pass, triangles (and normals) written at offset[block] + in-block prefix
#pragma once

#include "vh_mesh_table.h"

namespace vh {

constexpr int kApronSide = 9, kApronVoxels = 9 * 9 * 9;

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
        const uint32_t before = block_wg_scan(c0 + c1, sWave, total);      // (its barriers also fence sNb / sApron for the next pass)
        if (!kEmit) {
            if (tid == 0) blockCount[b] = total;
        } else if (total) {
            const unsigned long long at = scanned_at(tileBase, blockCount, b) + before;
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

// ---------------------------------------------------------------------------
// the indexed mesh (vh_extract_mesh_indexed): one vertex per edge, three indices per triangle
// ---------------------------------------------------------------------------
// A vertex is its edge (A, d): A the voxel of the lower end, d = 1..7 the axes on which the upper end is A + 1.  It exists iff
// the ends are valid with different inside flags and one of the cells that contain the edge (corner 0 at A - o, o disjoint
// from d) has eight valid corners and lies in a block of the region.  Vertices are ordered by (block of A in list order,
// voxel index of A, d), so they take their slots by count -> scan -> write like the triangles:
//   (vh_blocklist.hip              the block list over the region grown by one block towards +: A may sit in a +neighbour)
//   mesh_indexed_count_kernel      per listed block: 10^3 apron (local -1..8), a word {prefix << 7 | 7-bit mask} per voxel, the
//                                  block's vertices and (inside the region) triangles; listPos[ptr / 512] = list position
//   block_scan_*                   twice: vertex offsets, triangle offsets
//   mesh_indexed_emit_kernel       vertices (and normals) at base[block] + prefix + popcount(mask below d); indices per
//                                  triangle in vh_extract_mesh's order, read from the word of A in A's block
constexpr int kApron10Side = 10, kApron10Voxels = 10 * 10 * 10;
constexpr int kCellSide = 9, kCellFlags = 9 * 9 * 9;            // cells with corner 0 at local -1..7

struct MeshApron10 {          // 10^3 samples in LDS, local coordinates -1..8
    const float *s;
    __device__ __forceinline__ float at(int x, int y, int z) const
    {
        return s[((z + 1) * kApron10Side + (y + 1)) * kApron10Side + (x + 1)];
    }
};

// the 27 blocks around `item` through the hash (sNb), then its 512 voxels and the 488 around them towards - and + (sApron)
__device__ __forceinline__ void mesh_stage_apron10(const FrameParams &fp, const DevPtrs &dp, const int4 &item, int *sNb, float *sApron)
{
    const int tid = threadIdx.x;
    if (tid < 27) {
        const int ox = tid % 3 - 1, oy = (tid / 3) % 3 - 1, oz = tid / 9 - 1;
        sNb[tid] = tid == 13 ? item.w : lookup_block(fp, dp, item.x + ox, item.y + oy, item.z + oz);
    }
    __syncthreads();
    const MeshDirect direct{dp, sNb};
    const float4 v = *reinterpret_cast<const float4 *>(dp.blocks + (size_t)item.w + 2 * tid);
    const int i0 = 2 * tid, x0 = i0 & 7, y0 = (i0 >> 3) & 7, z0 = i0 >> 6;
    float *row = sApron + ((z0 + 1) * kApron10Side + (y0 + 1)) * kApron10Side + (x0 + 1);
    row[0] = v.y > 0.0f ? v.x : __builtin_nanf("");
    row[1] = v.w > 0.0f ? v.z : __builtin_nanf("");
    for (int i = tid; i < kApron10Voxels; i += 256) {
        const int x = i % kApron10Side - 1, y = (i / kApron10Side) % kApron10Side - 1, z = i / (kApron10Side * kApron10Side) - 1;
        if ((unsigned)x > 7u || (unsigned)y > 7u || (unsigned)z > 7u) sApron[i] = direct.at(x, y, z);
    }
    __syncthreads();
}

// bit o (o = dx | dy << 1 | dz << 2): the block at key - (dx, dy, dz) lies in the region
__device__ __forceinline__ uint32_t mesh_region_bits(const int4 &item, const BlockBox &rg)
{
    uint32_t bits = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        // (|key| < 2^28: the subtraction cannot wrap)
        bits |= (rg.holds(item.x - (o & 1), item.y - ((o >> 1) & 1), item.z - (o >> 2)) ? 1u : 0u) << o;
    }
    return bits;
}

// the 7-bit mask of the vertices anchored at local voxel (x,y,z): bit d - 1 for edge d.  sCell[c] = cell c emits if it has a sign change.
__device__ __forceinline__ uint32_t mesh_voxel_edges(const MeshApron10 &ap, const uint8_t *sCell, int x, int y, int z)
{
    const float sA = ap.at(x, y, z);
    if (!(sA == sA)) return 0u;
    const bool inA = sA <= 0.0f;
    uint32_t mask = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        const float sB = ap.at(x + (d & 1), y + ((d >> 1) & 1), z + (d >> 2));
        if (!(sB == sB) || (sB <= 0.0f) == inA) continue;
        uint32_t any = 0;
#pragma unroll
        for (int o = 0; o < 8; ++o)
            if (!(o & d)) any |= sCell[((z + 1 - (o >> 2)) * kCellSide + (y + 1 - ((o >> 1) & 1))) * kCellSide + (x + 1 - (o & 1))];
        if (any) mask |= 1u << (d - 1);
    }
    return mask;
}

// One listed block (of the grown region) per workgroup pass, two x-neighbouring voxels per lane.  word[b * 512 + voxel] =
// prefix of the block's vertices before the voxel << 7 | mask; vertexCount[b], triangleCount[b] (0 outside the region).
__global__ __launch_bounds__(256) void mesh_indexed_count_kernel(const FrameParams fp, const DevPtrs dp, const BlockBox rg,
                                                                 const int4 *__restrict__ items,
                                                                 const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                                 uint32_t *__restrict__ listPos, uint32_t listPosSize,
                                                                 uint32_t *__restrict__ word, uint32_t *__restrict__ vertexCount,
                                                                 uint32_t *__restrict__ triangleCount)
{
    __shared__ float sApron[kApron10Voxels];
    __shared__ uint8_t sCell[kCellFlags];
    __shared__ int sNb[27];
    __shared__ uint32_t sWave[4];
    const uint32_t count = min((uint32_t)*numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        mesh_stage_apron10(fp, dp, item, sNb, sApron);
        const MeshApron10 ap{sApron};
        const uint32_t inRegion = mesh_region_bits(item, rg);
        for (int i = tid; i < kCellFlags; i += 256) {
            const int cx = i % kCellSide - 1, cy = (i / kCellSide) % kCellSide - 1, cz = i / (kCellSide * kCellSide) - 1;
            bool ok = (inRegion >> ((cx < 0 ? 1 : 0) | (cy < 0 ? 2 : 0) | (cz < 0 ? 4 : 0))) & 1u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float s = ap.at(cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2));
                ok = ok && (s == s);
            }
            sCell[i] = ok ? 1 : 0;
        }
        __syncthreads();
        const int x = (2 * tid) & 7, y = (tid >> 2) & 7, z = tid >> 5;
        const uint32_t e0 = mesh_voxel_edges(ap, sCell, x, y, z), e1 = mesh_voxel_edges(ap, sCell, x + 1, y, z);
        const uint32_t v0 = __popc(e0), v1 = __popc(e1);
        uint32_t tris = 0;
        if (inRegion & 1u) tris = mesh_cell_count(mesh_cell_mask(ap, x, y, z)) + mesh_cell_count(mesh_cell_mask(ap, x + 1, y, z));
        // one scan for both: a block has at most 3 584 vertices and 6 144 triangles, 16 bits each
        uint32_t total;
        const uint32_t before = block_wg_scan((v0 + v1) | (tris << 16), sWave, total) & 0xffffu;   // (its barriers fence the LDS for the next pass)
        *reinterpret_cast<uint2 *>(word + (size_t)b * 512u + 2 * tid) = make_uint2((before << 7) | e0, ((before + v0) << 7) | e1);
        if (tid == 0) {
            vertexCount[b] = total & 0xffffu;
            triangleCount[b] = total >> 16;
            const uint32_t heap = (uint32_t)item.w >> 9;
            if (heap < listPosSize) listPos[heap] = b;
        }
    }
}

// index of vertex (A, d) from the word of A and the first vertex of A's block
__device__ __forceinline__ uint32_t mesh_vertex_index(uint32_t base, uint32_t w, uint32_t d)
{
    return base + (w >> 7) + __popc(w & ((1u << (d - 1u)) - 1u));
}

// The same pass over the listed blocks, after the two scans.  Vertices: the lane of voxel A writes the vertices anchored there.
// Indices (blocks inside the region): the lane of a cell writes its triangles; the vertex on edge (A, d) is found through the
// word of A, in this block (LDS) or in one of the seven +neighbours (their list position through listPos).
// result = {listed blocks, vertices, triangles}: nothing is written when the vertices do not fit 32 bits.
template <bool kNormals>
__global__ __launch_bounds__(256) void mesh_indexed_emit_kernel(const FrameParams fp, const DevPtrs dp, const BlockBox rg,
                                                                const int4 *__restrict__ items,
                                                                const unsigned long long *__restrict__ result, uint32_t listCapacity,
                                                                const uint32_t *__restrict__ listPos, uint32_t listPosSize,
                                                                const uint32_t *__restrict__ word,
                                                                const uint32_t *__restrict__ vertexOffset,
                                                                const unsigned long long *__restrict__ vertexTiles,
                                                                const uint32_t *__restrict__ triangleOffset,
                                                                const unsigned long long *__restrict__ triangleTiles,
                                                                unsigned long long capacityVertices, unsigned long long capacityTriangles,
                                                                float *__restrict__ vertices, float *__restrict__ normals,
                                                                uint32_t *__restrict__ indices)
{
    __shared__ float sApron[kApron10Voxels];
    __shared__ uint32_t sWord[512];
    __shared__ int sNb[27];
    __shared__ uint32_t sWave[4];
    __shared__ uint32_t sPos[8], sBase[8];
    const uint32_t count = min((uint32_t)result[0], listCapacity);
    if (result[1] > 0xffffffffull) return;
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        mesh_stage_apron10(fp, dp, item, sNb, sApron);
        const MeshApron10 ap{sApron};
        const MeshDirect direct{dp, sNb};
        const uint2 w = *reinterpret_cast<const uint2 *>(word + (size_t)b * 512u + 2 * tid);
        sWord[2 * tid] = w.x;
        sWord[2 * tid + 1] = w.y;
        if (tid < 8) {
            // the block that holds local voxel 8 on the axes of tid: valid voxels there mean it is allocated and listed
            const int p = sNb[((tid >> 2) + 1) * 9 + (((tid >> 1) & 1) + 1) * 3 + ((tid & 1) + 1)];
            uint32_t pos = 0, base = 0;
            if (p != VH_FREE_BLOCK && ((uint32_t)p >> 9) < listPosSize) {
                pos = listPos[(uint32_t)p >> 9];
                if (pos < count) base = (uint32_t)scanned_at(vertexTiles, vertexOffset, pos);
                else pos = 0;
            }
            sPos[tid] = pos;
            sBase[tid] = base;
        }
        __syncthreads();
        const int x = (2 * tid) & 7, y = (tid >> 2) & 7, z = tid >> 5;
        // vertices anchored at the lane's two voxels
        if (capacityVertices > 0 && (((w.x | w.y) & 127u) != 0u)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t wv = h ? w.y : w.x;
                unsigned long long at = (unsigned long long)sBase[0] + (wv >> 7);
                for (uint32_t d = 1; d < 8; ++d) {
                    if (!((wv >> (d - 1u)) & 1u)) continue;
                    if (at >= capacityVertices) break;
                    float p[3], q[3];
                    mesh_vertex<MeshApron10, kNormals>(fp, ap, direct, item, x + h, y, z, 0u, d, p, q);
                    float *out = vertices + at * 3ull;
                    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
                    if (kNormals) {
                        float *no = normals + at * 3ull;
                        no[0] = q[0]; no[1] = q[1]; no[2] = q[2];
                    }
                    ++at;
                }
            }
        }
        // indices of the block's cells
        if ((mesh_region_bits(item, rg) & 1u) && capacityTriangles > 0) {        // (uniform over the workgroup)
            const uint32_t m[2] = {mesh_cell_mask(ap, x, y, z), mesh_cell_mask(ap, x + 1, y, z)};
            const uint32_t c[2] = {mesh_cell_count(m[0]), mesh_cell_count(m[1])};
            uint32_t total;
            const uint32_t before = block_wg_scan(c[0] + c[1], sWave, total);
            unsigned long long at = scanned_at(triangleTiles, triangleOffset, b) + before;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!c[h]) continue;
                for (int t = 0; t < 6; ++t) {
                    const uint32_t corners = kMeshTet[t];
                    uint32_t tw = kMeshTable[t][mesh_tet_mask(m[h], corners)];
                    const uint32_t n = tw & 3u;
                    tw >>= 2;
                    for (uint32_t k = 0; k < n; ++k, ++at) {
                        uint32_t idx[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            const uint32_t e = tw & 15u;
                            tw >>= 4;
                            const uint32_t ca = (corners >> (8u * (e & 3u))) & 7u, cb = (corners >> (8u * (e >> 2))) & 7u;
                            const int ax = x + h + (int)(ca & 1u), ay = y + (int)((ca >> 1) & 1u), az = z + (int)(ca >> 2);
                            const uint32_t o = (uint32_t)(ax >> 3) | ((uint32_t)(ay >> 3) << 1) | ((uint32_t)(az >> 3) << 2);
                            const uint32_t voxel = (uint32_t)(((az & 7) << 6) | ((ay & 7) << 3) | (ax & 7));
                            const uint32_t wa = o ? word[(size_t)sPos[o] * 512u + voxel] : sWord[voxel];
                            idx[j] = mesh_vertex_index(sBase[o], wa, ca ^ cb);
                        }
                        if (at < capacityTriangles) {
                            uint32_t *out = indices + at * 3ull;
                            out[0] = idx[0]; out[1] = idx[1]; out[2] = idx[2];
                        }
                    }
                }
            }
        }
        __syncthreads();              // sWord / sPos / sApron are read until here
    }
}

}  // namespace vh
