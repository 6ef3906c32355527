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

// The VH_SAMPLE_TRILINEAR sample at u = p / voxelSize (inDomain: |u| < 2^30 on every axis), stated once for sample_points_kernel
// and sdf_round_kernel (vh_track.hip).  Called by every lane of the wave, with or without a point (inDomain false): the lanes
// of a run share the look-ups, a point resolves the 1, 2, 4 or 8 distinct blocks of its cell only, and the two corners of
// an x-edge inside a block are one 16-byte load.  No sample: {NaN, 0, NaN}.
struct SampleTrilinear { float sdf, weight, g[3]; };

__device__ __forceinline__ SampleTrilinear sample_trilinear(const FrameParams &fp, const DevPtrs &dp, int lane, const float u[3],
                                                            bool inDomain)
{
    const float nan = __builtin_nanf("");
    SampleTrilinear r = {nan, 0.0f, {nan, nan, nan}};
    int i[3] = {0, 0, 0};
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (inDomain) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float f = __builtin_floorf(u[a]);
            i[a] = f2i_rz(f);
            t[a] = u[a] - f;
        }
    }
    const int kx = i[0] >> 3, ky = i[1] >> 3, kz = i[2] >> 3;
    // which axes the cell crosses a block face on: corner c lies in block (key + (c & cross))
    const int cross = ((i[0] & 7) == 7 ? 1 : 0) | ((i[1] & 7) == 7 ? 2 : 0) | ((i[2] & 7) == 7 ? 4 : 0);
    const SampleRuns runs = sample_runs(lane, kx, ky, kz);
    int ptr[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // 1, 2, 4 or 8 distinct blocks: a corner whose bits all cross is a block of its own, any other shares the block of
        // the corner without one of its non-crossing bits (resolved before it)
        const int p = sample_resolve(fp, dp, lane, runs, inDomain && (c & ~cross) == 0, kx + (c & 1), ky + ((c >> 1) & 1),
                                     kz + (c >> 2));
        if ((c & ~cross) == 0) ptr[c] = p;
        else if (c & ~cross & 1) ptr[c] = ptr[c & 6];
        else if (c & ~cross & 2) ptr[c] = ptr[c & 5];
        else ptr[c] = ptr[c & 3];
    }
    SampleVoxel v[8];
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        const int index = sample_index(i[0], i[1] + ((c >> 1) & 1), i[2] + (c >> 2));
        if (!(cross & 1)) {
            v[c] = v[c + 1] = SampleVoxel{nan, 0.0f};
            if (ptr[c] != VH_FREE_BLOCK) {
                const VoxelPair pair = *reinterpret_cast<const VoxelPair *>(dp.blocks + (size_t)ptr[c] + (size_t)index);
                v[c] = sample_judge(pair.s0, pair.w0);
                v[c + 1] = sample_judge(pair.s1, pair.w1);
            }
        } else {
            v[c] = sample_voxel(dp, ptr[c], index);
            v[c + 1] = sample_voxel(dp, ptr[c + 1], sample_index(i[0] + 1, i[1] + ((c >> 1) & 1), i[2] + (c >> 2)));
        }
    }
    bool all = inDomain;
#pragma unroll
    for (int c = 0; c < 8; ++c) all = all && v[c].sdf == v[c].sdf;
    if (all) {
        const float tx = t[0], ty = t[1], tz = t[2];
        const float s0 = v[0].sdf, s1 = v[1].sdf, s2 = v[2].sdf, s3 = v[3].sdf, s4 = v[4].sdf, s5 = v[5].sdf, s6 = v[6].sdf,
                    s7 = v[7].sdf;
        r.sdf = sample_lerp(sample_lerp(sample_lerp(s0, s1, tx), sample_lerp(s2, s3, tx), ty),
                            sample_lerp(sample_lerp(s4, s5, tx), sample_lerp(s6, s7, tx), ty), tz);
        r.weight = sample_lerp(sample_lerp(sample_lerp(v[0].weight, v[1].weight, tx), sample_lerp(v[2].weight, v[3].weight, tx), ty),
                               sample_lerp(sample_lerp(v[4].weight, v[5].weight, tx), sample_lerp(v[6].weight, v[7].weight, tx), ty), tz);
        r.g[0] = sample_lerp(sample_lerp(s1 - s0, s3 - s2, ty), sample_lerp(s5 - s4, s7 - s6, ty), tz) / fp.voxelSize;
        r.g[1] = sample_lerp(sample_lerp(s2 - s0, s3 - s1, tx), sample_lerp(s6 - s4, s7 - s5, tx), tz) / fp.voxelSize;
        r.g[2] = sample_lerp(sample_lerp(s4 - s0, s5 - s1, tx), sample_lerp(s6 - s2, s7 - s3, tx), ty) / fp.voxelSize;
    }
    return r;
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
        int r[3] = {0, 0, 0};
        if (inDomain) {
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = f2i_rz(u[a] + __builtin_copysignf(0.5f, u[a]));
        }
        const int kx = r[0] >> 3, ky = r[1] >> 3, kz = r[2] >> 3;
        const SampleRuns runs = sample_runs(lane, kx, ky, kz);
        const int resolved = sample_resolve(fp, dp, lane, runs, inDomain, kx, ky, kz);
        const int ptr = inDomain ? resolved : VH_FREE_BLOCK;       // (a lane without a sample may sit in a run that has one)
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
        const SampleTrilinear r = sample_trilinear(fp, dp, lane, u, inDomain);
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
