// vh_sample.hip -- the fused TSDF as a distance field: vh_sample_sdf, vh_sample_lattice.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_mesh.hip (lookup_block comes from vh_raycast.hip).
//
// Validity is the mesh's rule (mesh_voxel): block allocated in this table, weight > 0, sdf == sdf.  The arithmetic is the
// specification's (tests/sample_ref.py), unfused fp32 in its order, so the outputs are its bits.
//   sample_points_kernel          one point per lane.  The lanes of a wave that ask for the same block form runs, a run's
//                                 first lane looks the block up and the others read the pointer across lanes; a point
//                                 resolves the 1, 2, 4 or 8 distinct blocks of its cell only, and the two corners of an
//                                 x-edge inside a block are one 16-byte load.  (One lookup_block per voxel read and eight
//                                 scalar loads, the form this one was measured against: DESIGN_LOG.md.)
//   sample_lattice_kernel         one workgroup pass per 8^3 brick that meets the box: one lookup, two voxels per lane.
// The trilinear cell (sample_cell, sample_cell_voxels, cell_lerp, cell_gradient) and the nearest lookup (sample_nearest_block)
// are stated here once for every kernel that samples the model: vh_color.hip, vh_merge.hip and vh_track.hip call them.
#pragma once

namespace vh {

constexpr int kSampleNearest = 0, kSampleTrilinear = 1;
constexpr float kSampleDomain = 1073741824.0f;     // 2^30: |p / voxelSize| below it, so that voxel +- 1 fits an int32

struct SampleVoxel { float sdf, weight; };         // {NaN, 0} where the voxel is not valid

__device__ __forceinline__ SampleVoxel sample_judge(float sdf, float weight)
{
    SampleVoxel r = {__builtin_nanf(""), 0.0f};
    if (weight > 0.0f && sdf == sdf) { r.sdf = sdf; r.weight = weight; }
    return r;
}

__device__ __forceinline__ SampleVoxel sample_voxel(const DevPtrs &dp, int ptr, int index)
{
    if (ptr == VH_FREE_BLOCK) return SampleVoxel{__builtin_nanf(""), 0.0f};
    const Voxel v = dp.blocks[(size_t)ptr + (size_t)index];
    return sample_judge(v.sdf, v.weight);
}

__device__ __forceinline__ int sample_index(int x, int y, int z) { return ((z & 7) << 6) | ((y & 7) << 3) | (x & 7); }

// two x-neighbouring voxels of one block: 16 bytes, aligned to 8 (the first voxel's x may be odd)
struct __attribute__((aligned(8))) VoxelPair { float s0, w0, s1, w1; };

__device__ __forceinline__ float sample_lerp(float a, float b, float t) { return a + t * (b - a); }

// The runs of equal block keys among the lanes of a wave, as the claim phase forms them (vh_alloc.hip): head = the first lane
// of this lane's run, mine = the lanes of the run.  Every lane of the wave takes part, with or without a point.
struct SampleRuns {
    int head;
    unsigned long long mine;
};

__device__ __forceinline__ SampleRuns sample_runs(int lane, int kx, int ky, int kz)
{
    const int px = __shfl_up(kx, 1), py = __shfl_up(ky, 1), pz = __shfl_up(kz, 1);
    const unsigned long long heads = __ballot(lane == 0 || px != kx || py != ky || pz != kz);
    const unsigned long long upTo = (2ull << lane) - 1ull;                 // lanes 0..lane (all of them for lane 63)
    SampleRuns r;
    r.head = 63 - __builtin_clzll(heads & upTo);                           // (lane 0 is a head: never empty)
    const unsigned long long above = heads & ~upTo;
    const unsigned long long below = above ? (1ull << __builtin_ctzll(above)) - 1ull : ~0ull;      // lanes before the next head
    r.mine = below & ~((1ull << r.head) - 1ull);
    return r;
}

// The block (kx, ky, kz) for the lanes that `need` it.  The key is the same in every lane of a run; the run's head looks it
// up if a lane of the run needs it.  Called by every lane of the wave.
__device__ __forceinline__ int sample_resolve(const FrameParams &fp, const DevPtrs &dp, int lane, const SampleRuns &runs, bool need,
                                              int kx, int ky, int kz)
{
    const bool wanted = (__ballot(need) & runs.mine) != 0ull;
    int p = VH_FREE_BLOCK;
    if (lane == runs.head && wanted) p = lookup_block(fp, dp, kx, ky, kz);
    return __shfl(p, runs.head);
}

// The cell of the VH_SAMPLE_TRILINEAR sample at u = p / voxelSize (inDomain: |u| < 2^30 on every axis) and the blocks of its
// eight corners, stated once for every trilinear reader of the model: sample_trilinear, merge_color_trilinear (vh_merge.hip),
// color_points_kernel (vh_color.hip) and the joint round (vh_track.hip).  Called by every lane of the wave, with or without a
// point (inDomain false): the lanes of a run share the look-ups, and a point resolves the 1, 2, 4 or 8 distinct blocks of its
// cell only.
struct SampleCell {
    int i[3];            // the voxel of corner 0; (0, 0, 0) where inDomain is false
    float t[3];
    int cross;           // bit a: the cell crosses a block face on axis a
    // The block of corner c, VH_FREE_BLOCK where the table has none.  A lane without a point has the key (0, 0, 0) and sits in
    // a run like any other: it holds that block's pointer whenever a lane of its run asked for the block, so ptr says nothing
    // about inDomain.  Every caller gates on inDomain itself -- before it judges the voxels (sample_trilinear,
    // merge_color_trilinear) or before it reads through ptr (color_points_kernel); the reads of sample_cell_voxels need no
    // gate: a pointer that is not VH_FREE_BLOCK names a whole block.
    int ptr[8];
};

__device__ __forceinline__ SampleCell sample_cell(const FrameParams &fp, const DevPtrs &dp, int lane, const float u[3], bool inDomain)
{
    SampleCell cell = {{0, 0, 0}, {0.0f, 0.0f, 0.0f}, 0, {}};
    if (inDomain) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float f = __builtin_floorf(u[a]);
            cell.i[a] = f2i_rz(f);
            cell.t[a] = u[a] - f;
        }
    }
    const int kx = cell.i[0] >> 3, ky = cell.i[1] >> 3, kz = cell.i[2] >> 3;
    // which axes the cell crosses a block face on: corner c lies in block (key + (c & cross))
    const int cross = ((cell.i[0] & 7) == 7 ? 1 : 0) | ((cell.i[1] & 7) == 7 ? 2 : 0) | ((cell.i[2] & 7) == 7 ? 4 : 0);
    cell.cross = cross;
    const SampleRuns runs = sample_runs(lane, kx, ky, kz);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // 1, 2, 4 or 8 distinct blocks: a corner whose bits all cross is a block of its own, any other shares the block of
        // the corner without one of its non-crossing bits (resolved before it)
        const int p = sample_resolve(fp, dp, lane, runs, inDomain && (c & ~cross) == 0, kx + (c & 1), ky + ((c >> 1) & 1),
                                     kz + (c >> 2));
        if ((c & ~cross) == 0) cell.ptr[c] = p;
        else if (c & ~cross & 1) cell.ptr[c] = cell.ptr[c & 6];
        else if (c & ~cross & 2) cell.ptr[c] = cell.ptr[c & 5];
        else cell.ptr[c] = cell.ptr[c & 3];
    }
    return cell;
}

__device__ __forceinline__ int sample_cell_index(const SampleCell &cell, int c)
{
    return sample_index(cell.i[0] + (c & 1), cell.i[1] + ((c >> 1) & 1), cell.i[2] + (c >> 2));
}

// The eight voxels of the cell, judged.  The two corners of an x-edge inside a block are one 16-byte load.  No cross-lane read.
__device__ __forceinline__ void sample_cell_voxels(const DevPtrs &dp, const SampleCell &cell, SampleVoxel v[8])
{
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        const int index = sample_cell_index(cell, c);
        if (!(cell.cross & 1)) {
            v[c] = v[c + 1] = SampleVoxel{__builtin_nanf(""), 0.0f};
            if (cell.ptr[c] != VH_FREE_BLOCK) {
                const VoxelPair pair = *reinterpret_cast<const VoxelPair *>(dp.blocks + (size_t)cell.ptr[c] + (size_t)index);
                v[c] = sample_judge(pair.s0, pair.w0);
                v[c + 1] = sample_judge(pair.s1, pair.w1);
            }
        } else {
            v[c] = sample_voxel(dp, cell.ptr[c], index);
            v[c + 1] = sample_voxel(dp, cell.ptr[c + 1], sample_cell_index(cell, c + 1));
        }
    }
}

// the lerp nest (x innermost, then y, then z) and the corner-difference gradient over the eight values of a cell
__device__ __forceinline__ float cell_lerp(const float s[8], const float t[3])
{
    return sample_lerp(sample_lerp(sample_lerp(s[0], s[1], t[0]), sample_lerp(s[2], s[3], t[0]), t[1]),
                       sample_lerp(sample_lerp(s[4], s[5], t[0]), sample_lerp(s[6], s[7], t[0]), t[1]), t[2]);
}

__device__ __forceinline__ void cell_gradient(const float s[8], const float t[3], float voxelSize, float g[3])
{
    g[0] = sample_lerp(sample_lerp(s[1] - s[0], s[3] - s[2], t[1]), sample_lerp(s[5] - s[4], s[7] - s[6], t[1]), t[2]) / voxelSize;
    g[1] = sample_lerp(sample_lerp(s[2] - s[0], s[3] - s[1], t[0]), sample_lerp(s[6] - s[4], s[7] - s[5], t[0]), t[2]) / voxelSize;
    g[2] = sample_lerp(sample_lerp(s[4] - s[0], s[5] - s[1], t[0]), sample_lerp(s[6] - s[2], s[7] - s[3], t[0]), t[1]) / voxelSize;
}

// The VH_SAMPLE_TRILINEAR sample in a cell (sample_cell's, with the inDomain it was given).  No sample: {NaN, 0, NaN}.  No
// cross-lane read.
struct SampleTrilinear { float sdf, weight, g[3]; };

__device__ __forceinline__ SampleTrilinear sample_trilinear(const FrameParams &fp, const DevPtrs &dp, const SampleCell &cell,
                                                            bool inDomain)
{
    const float nan = __builtin_nanf("");
    SampleTrilinear r = {nan, 0.0f, {nan, nan, nan}};
    SampleVoxel v[8];
    sample_cell_voxels(dp, cell, v);
    bool all = inDomain;
#pragma unroll
    for (int c = 0; c < 8; ++c) all = all && v[c].sdf == v[c].sdf;
    if (all) {
        float s[8], w[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { s[c] = v[c].sdf; w[c] = v[c].weight; }
        r.sdf = cell_lerp(s, cell.t);
        r.weight = cell_lerp(w, cell.t);
        cell_gradient(s, cell.t, fp.voxelSize, r.g);
    }
    return r;
}

// The VH_SAMPLE_NEAREST voxel of u and its block.  Called by every lane of the wave, with or without a point.
struct SampleNearest {
    int r[3];            // the voxel; (0, 0, 0) where inDomain is false
    SampleRuns runs;     // of the voxel's block key, for a caller that goes on to its neighbours
    int ptr;             // the block, VH_FREE_BLOCK where the table has none or inDomain is false
};

__device__ __forceinline__ SampleNearest sample_nearest_block(const FrameParams &fp, const DevPtrs &dp, int lane, const float u[3],
                                                              bool inDomain)
{
    SampleNearest n = {{0, 0, 0}, {}, VH_FREE_BLOCK};
    if (inDomain) {
#pragma unroll
        for (int a = 0; a < 3; ++a) n.r[a] = f2i_rz(u[a] + __builtin_copysignf(0.5f, u[a]));
    }
    const int kx = n.r[0] >> 3, ky = n.r[1] >> 3, kz = n.r[2] >> 3;
    n.runs = sample_runs(lane, kx, ky, kz);
    const int resolved = sample_resolve(fp, dp, lane, n.runs, inDomain, kx, ky, kz);
    n.ptr = inDomain ? resolved : VH_FREE_BLOCK;        // (a lane without a sample may sit in a run that has one)
    return n;
}

__global__ __launch_bounds__(256) void sample_points_kernel(const FrameParams fp, const DevPtrs dp, int mode, uint32_t n,
                                                            const float *__restrict__ points, float *__restrict__ sdfOut,
                                                            float *__restrict__ weightOut, float *__restrict__ gradOut)
{
    const int lane = threadIdx.x & 63;
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    const bool have = at < n;                       // (no early return: the lanes without a point serve the cross-lane reads)
    const float nan = __builtin_nanf("");
    float u[3] = {nan, nan, nan};
    if (have) {
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = points[(size_t)at * 3u + a] / fp.voxelSize;
    }
    const bool inDomain = __builtin_fabsf(u[0]) < kSampleDomain && __builtin_fabsf(u[1]) < kSampleDomain &&
                          __builtin_fabsf(u[2]) < kSampleDomain;          // false for NaN
    float sdf = nan, weight = 0.0f, g[3] = {nan, nan, nan};

    if (mode == kSampleNearest) {
        const SampleNearest near = sample_nearest_block(fp, dp, lane, u, inDomain);
        const int *r = near.r;
        const int ptr = near.ptr, kx = r[0] >> 3, ky = r[1] >> 3, kz = r[2] >> 3;
        const SampleRuns &runs = near.runs;
        const SampleVoxel here = sample_voxel(dp, ptr, sample_index(r[0], r[1], r[2]));
        sdf = here.sdf;
        weight = here.weight;
        if (gradOut) {                              // (wave-uniform)
            const bool valid = here.sdf == here.sdf;
            bool ok = valid;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int l = r[a] & 7;
                const int dx = a == 0, dy = a == 1, dz = a == 2;
                // a neighbour in this block needs no lookup, one across a face needs that block (the same key in every lane of
                // the run)
                const bool up = l == 7, down = l == 0;
                const int pp = sample_resolve(fp, dp, lane, runs, valid && up, kx + dx, ky + dy, kz + dz);
                const int pm = sample_resolve(fp, dp, lane, runs, valid && down, kx - dx, ky - dy, kz - dz);
                float sp = nan, sm = nan;
                if (valid) {
                    sp = sample_voxel(dp, up ? pp : ptr, sample_index(r[0] + dx, r[1] + dy, r[2] + dz)).sdf;
                    sm = sample_voxel(dp, down ? pm : ptr, sample_index(r[0] - dx, r[1] - dy, r[2] - dz)).sdf;
                }
                const bool hp = sp == sp, hm = sm == sm;
                float d = 0.0f;
                if (hp && hm) d = (sp - sm) * 0.5f;
                else if (hp) d = sp - here.sdf;
                else if (hm) d = here.sdf - sm;
                else ok = false;
                g[a] = d / fp.voxelSize;
            }
            if (!ok) g[0] = g[1] = g[2] = nan;
        }
    } else {
        const SampleTrilinear r = sample_trilinear(fp, dp, sample_cell(fp, dp, lane, u, inDomain), inDomain);
        sdf = r.sdf;
        weight = r.weight;
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = r.g[a];
    }
    if (!have) return;
    sdfOut[at] = sdf;
    if (weightOut) weightOut[at] = weight;
    if (gradOut) {
#pragma unroll
        for (int a = 0; a < 3; ++a) gradOut[(size_t)at * 3u + a] = g[a];
    }
}

// The box lo <= voxel < lo + dims, x fastest.  brick0 = the block of `lo`, bricks = blocks per axis that meet the box.  A
// workgroup takes the bricks blockIdx.x, + gridDim.x, ...; lane t holds voxels 2t and 2t + 1 of the brick (one 16-byte load).
struct LatticeBox { int lo[3], dims[3], brick0[3], bricks[3]; };

__global__ __launch_bounds__(256) void sample_lattice_kernel(const FrameParams fp, const DevPtrs dp, const LatticeBox box,
                                                             unsigned long long numBricks, float *__restrict__ sdfOut,
                                                             float *__restrict__ weightOut)
{
    __shared__ int sPtr;
    const int x = (threadIdx.x & 3) * 2, y = (threadIdx.x >> 2) & 7, z = threadIdx.x >> 5;
    for (unsigned long long b = blockIdx.x; b < numBricks; b += gridDim.x) {
        const unsigned long long row = b / (unsigned long long)box.bricks[0];
        const int bx = box.brick0[0] + (int)(b - row * (unsigned long long)box.bricks[0]);
        const int by = box.brick0[1] + (int)(row % (unsigned long long)box.bricks[1]);
        const int bz = box.brick0[2] + (int)(row / (unsigned long long)box.bricks[1]);
        __syncthreads();                            // (the pass before has read sPtr)
        if (threadIdx.x == 0) sPtr = lookup_block(fp, dp, bx, by, bz);
        __syncthreads();
        const int ptr = sPtr;
        // position inside the box, as 64 bits: a brick's first voxel may lie before lo
        const long long i = (long long)bx * 8 + x - box.lo[0], j = (long long)by * 8 + y - box.lo[1],
                        k = (long long)bz * 8 + z - box.lo[2];
        if (j < 0 || j >= box.dims[1] || k < 0 || k >= box.dims[2]) continue;
        SampleVoxel v[2] = {{__builtin_nanf(""), 0.0f}, {__builtin_nanf(""), 0.0f}};
        if (ptr != VH_FREE_BLOCK) {
            const float4 pair = *reinterpret_cast<const float4 *>(dp.blocks + (size_t)ptr + (size_t)sample_index(x, y, z));
            v[0] = sample_judge(pair.x, pair.y);
            v[1] = sample_judge(pair.z, pair.w);
        }
        const size_t rowAt = ((size_t)k * (size_t)box.dims[1] + (size_t)j) * (size_t)box.dims[0];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (i + e < 0 || i + e >= box.dims[0]) continue;
            sdfOut[rowAt + (size_t)(i + e)] = v[e].sdf;
            if (weightOut) weightOut[rowAt + (size_t)(i + e)] = v[e].weight;
        }
    }
}

}  // namespace vh
