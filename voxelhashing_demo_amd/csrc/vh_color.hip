// vh_color.hip -- the model in colour: vh_integrate_color, vh_sample_color, the colour half of block deletion (DESIGN.md 4.14;
// the rule: include/voxelhash.h, "the model in colour", and tests/color_ref.py).  No counterpart in the reference.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_sample.hip (lane_cell comes from vh_integrate.hip,
// sample_cell / sample_nearest_block / sample_voxel / cell_lerp from vh_sample.hip).
//
// Colour is a second volume beside dp.blocks, one uint32 per voxel at the same index: r | g << 8 | b << 16 | w << 24 with w the
// sample count (1..255); the word 0 is "no colour".  It is not a member of DevPtrs (a by-value argument of every kernel, whose
// layout stays): the pointer travels as a kernel argument of its own.
//   color_integrate_kernel   the TSDF update's launch shape: 256 lanes own one 8^3 block per pass, lane t voxels 2t and 2t + 1;
//                            one 16-byte load of the TSDF pair (read only), one 8-byte load of the colour pair, one 4-byte
//                            gather per voxel from the image, one 8-byte store when a word changed
//   color_deintegrate_kernel the same launch with the sample taken back out of the running average (vh_deintegrate_color)
//   color_release_kernel     the colour words of the blocks a deletion freed, zeroed (ahead of gc_release_kernel, same list)
//   color_points_kernel      one point per lane, the run-sharing look-ups of sample_points_kernel
#pragma once

namespace vh {

// The frame's colour sample of voxel (vx, vy, vz) combined into its word c; ow is the voxel's stored TSDF weight.
// true: the word changed.  The camera point, the projection, the bounds test and the depth read are tsdf_apply's
// (vh_integrate.hip), stated a second time so that the kernels of the TSDF update keep their code.  Two compile-time tails, as
// tsdf_apply has them: kColorAdd averages the pixel in, kColorRemove takes it back out (vh_deintegrate_color; weightMax unused).
enum ColorOp { kColorAdd, kColorRemove };

template <ColorOp kOp, class Depth>
__device__ __forceinline__ bool color_apply(const FrameParams &fp, const Depth &src, const uint32_t *__restrict__ rgba, float band,
                                            uint32_t weightMax, int vx, int vy, int vz, float ow, uint32_t &c)
{
    if (!(ow > 0.0f)) {                     // a voxel that holds nothing has no colour (also what a de-integration orphaned)
        const bool had = c != 0u;
        c = 0u;
        return had;
    }
    float cx, cy, cz;
    if (fp.semantics == VH_SEM_REFERENCE) {
        const float4 r = mat4_mul(fp.Tinv, (float)vx, (float)vy, (float)vz, 1.0f);
        cx = (float)f2i_rz(r.x) * fp.voxelSize;
        cy = (float)f2i_rz(r.y) * fp.voxelSize;
        cz = (float)f2i_rz(r.z) * fp.voxelSize;
    } else {
        const float4 r = mat4_mul(fp.Tinv, (float)vx * fp.voxelSize, (float)vy * fp.voxelSize, (float)vz * fp.voxelSize, 1.0f);
        cx = r.x; cy = r.y; cz = r.z;
    }
    int sx, sy;
    project(fp.proj, cx, cy, cz, sx, sy);
    if (sx < 0 || sx >= fp.width || sy < 0 || sy >= fp.height) return false;
    const float depth = src.at(sx, sy, fp.width);
    if (depth <= 0.0f) return false;
    const float s = depth - cz;             // no truncation: colour belongs to the surface
    if (!(__builtin_fabsf(s) <= band)) return false;
    if constexpr (kOp == kColorRemove) {
        const uint32_t w = c >> 24;
        if (w == 0u) return false;          // nothing to take out
        if (w == 1u) { c = 0u; return true; }
        const uint32_t in = rgba[(size_t)sy * fp.width + sx];
        const float fw = (float)w, den = (float)(w - 1u);
        uint32_t out = (w - 1u) << 24;
#pragma unroll
        for (int k = 0; k < 24; k += 8) {
            float f = ((float)((c >> k) & 255u) * fw - (float)((in >> k) & 255u)) / den;
            f = __builtin_fminf(__builtin_fmaxf(f, 0.0f), 255.0f);      // (the stored mean was rounded: the inverse may leave a byte)
            out |= (uint32_t)(f + 0.5f) << k;
        }
        c = out;                            // (the count moved: the word changed)
        return true;
    }
    if (weightMax == 0u) return false;      // the sweep only
    const uint32_t in = rgba[(size_t)sy * fp.width + sx];
    const uint32_t w = c >> 24;
    const float fw = (float)w, den = (float)(w + 1u);
    uint32_t out = min(w + 1u, weightMax) << 24;
#pragma unroll
    for (int k = 0; k < 24; k += 8) {
        const float f = ((float)((c >> k) & 255u) * fw + (float)((in >> k) & 255u)) / den;
        out |= (uint32_t)(f + 0.5f) << k;   // (at most 255: a mean of bytes)
    }
    const bool changed = out != c;
    c = out;
    return changed;
}

// The fixed grid of the TSDF update over the dense compact list the step-level flatten left for `pose` (entries of allocated
// blocks only, so every e.ptr names a whole block inside dp.blocks and inside the colour volume, which has a word per voxel).
template <class Depth>
__global__ __launch_bounds__(256) void color_integrate_kernel(const FrameParams fp, const DevPtrs dp, const Depth src,
                                                              uint32_t *__restrict__ color, const uint32_t *__restrict__ rgba,
                                                              float band, uint32_t weightMax)
{
    const int count = dp.counters[kCompactCount];
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        const VoxelEntry e = dp.compact[k];
        const LaneCell cell = lane_cell(dp, e);
        const float4 v = *cell.cell;                                                        // {sdf0, w0, sdf1, w1}
        uint2 *words = reinterpret_cast<uint2 *>(color + (size_t)e.ptr + 2 * threadIdx.x);
        uint2 c = *words;
        const bool u0 = color_apply<kColorAdd>(fp, src, rgba, band, weightMax, cell.bx, cell.by, cell.bz, v.y, c.x);
        const bool u1 = color_apply<kColorAdd>(fp, src, rgba, band, weightMax, cell.bx + 1, cell.by, cell.bz, v.w, c.y);
        if (u0 || u1) *words = c;
    }
}

// The same grid over the list the flatten left for the frame's pose, the frame's colour sample taken back out of every word
// that passes color_apply's tests (the TSDF is read as it stands: the call goes ahead of the frame's vh_deintegrate_depth).
template <class Depth>
__global__ __launch_bounds__(256) void color_deintegrate_kernel(const FrameParams fp, const DevPtrs dp, const Depth src,
                                                                uint32_t *__restrict__ color, const uint32_t *__restrict__ rgba,
                                                                float band)
{
    const int count = dp.counters[kCompactCount];
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        const VoxelEntry e = dp.compact[k];
        const LaneCell cell = lane_cell(dp, e);
        const float4 v = *cell.cell;                                                        // {sdf0, w0, sdf1, w1}
        uint2 *words = reinterpret_cast<uint2 *>(color + (size_t)e.ptr + 2 * threadIdx.x);
        uint2 c = *words;
        const bool u0 = color_apply<kColorRemove>(fp, src, rgba, band, 0u, cell.bx, cell.by, cell.bz, v.y, c.x);
        const bool u1 = color_apply<kColorRemove>(fp, src, rgba, band, 0u, cell.bx + 1, cell.by, cell.bz, v.w, c.y);
        if (u0 || u1) *words = c;
    }
}

// One freed block per workgroup pass: its 2 KiB of colour words go back to "no colour" (blocks are handed out zeroed).  Reads
// the freed list gc_release_kernel is about to consume.
__global__ __launch_bounds__(256) void color_release_kernel(const DevPtrs dp, uint32_t *__restrict__ color)
{
    const int n = dp.counters[kGcFreed];
    const int32_t *freed = reinterpret_cast<const int32_t *>(dp.compact);
    for (int b = blockIdx.x; b < n; b += gridDim.x)
        reinterpret_cast<uint2 *>(color + (size_t)freed[b])[threadIdx.x] = make_uint2(0u, 0u);
}

// the colour word of voxel `index` of block ptr if that voxel is valid (sample_voxel's rule), else 0
__device__ __forceinline__ uint32_t color_voxel(const DevPtrs &dp, const uint32_t *__restrict__ color, int ptr, int index)
{
    if (ptr == VH_FREE_BLOCK) return 0u;
    const SampleVoxel v = sample_voxel(dp, ptr, index);
    return v.sdf == v.sdf ? color[(size_t)ptr + (size_t)index] : 0u;
}

struct ColorPoints {
    const float *points;     // n * 3 world metres, or (toWorld) n float4 camera-frame points, .z == 0: no point
    float T[12];             // rows 0..2 of the camera -> world pose
    int toWorld;
};

// Lanes without a point stay in for the cross-lane reads of sample_nearest_block / sample_cell (vh_sample.hip): no early return.
__global__ __launch_bounds__(256) void color_points_kernel(const FrameParams fp, const DevPtrs dp, const uint32_t *__restrict__ color,
                                                           int mode, uint32_t n, const ColorPoints in, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    const bool have = at < n;
    const float nan = __builtin_nanf("");
    float u[3] = {nan, nan, nan};
    if (have) {
        if (in.toWorld) {
            const float4 p = reinterpret_cast<const float4 *>(in.points)[at];
            if (p.z != 0.0f) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    u[r] = (((in.T[4 * r + 0] * p.x + in.T[4 * r + 1] * p.y) + in.T[4 * r + 2] * p.z) + in.T[4 * r + 3]) / fp.voxelSize;
            }
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) u[a] = in.points[(size_t)at * 3u + a] / fp.voxelSize;
        }
    }
    const bool inDomain = __builtin_fabsf(u[0]) < kSampleDomain && __builtin_fabsf(u[1]) < kSampleDomain &&
                          __builtin_fabsf(u[2]) < kSampleDomain;          // false for NaN
    uint32_t rgb = 0u;

    if (mode == kSampleNearest) {
        const SampleNearest near = sample_nearest_block(fp, dp, lane, u, inDomain);
        const uint32_t c = color_voxel(dp, color, near.ptr, sample_index(near.r[0], near.r[1], near.r[2]));
        if (c >> 24) rgb = (c & 0xffffffu) | 0xff000000u;
    } else {
        const SampleCell cell = sample_cell(fp, dp, lane, u, inDomain);
        uint32_t w[8];
        bool all = inDomain;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            // (a lane without a point may hold the pointer of block (0, 0, 0): SampleCell::ptr)
            w[c] = color_voxel(dp, color, inDomain ? cell.ptr[c] : VH_FREE_BLOCK, sample_cell_index(cell, c));
            all = all && (w[c] >> 24) != 0u;
        }
        if (all) {
            rgb = 0xff000000u;
#pragma unroll
            for (int k = 0; k < 24; k += 8) {
                float s[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) s[c] = (float)((w[c] >> k) & 255u);
                rgb |= (uint32_t)(cell_lerp(s, cell.t) + 0.5f) << k;
            }
        }
    }
    if (have) out[at] = rgb;
}

}  // namespace vh
