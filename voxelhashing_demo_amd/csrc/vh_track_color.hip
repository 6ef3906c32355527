// vh_track_color.hip -- camera tracking against the model's shape and colour together: vh_sdf_color_align,
// vh_sdf_color_build_system, vh_sdf_color_residuals (the rule: include/voxelhash.h, "tracking against the
// model's colour and shape", and tests/sdf_color_track_ref.py).  No counterpart in the reference: the photometric term is that
// of Kerl et al., "Dense Visual SLAM for RGB-D Cameras", IROS 2013, taken against the fused colour volume instead of a key
// frame.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_color.hip.
//
// A round is vh_track.hip's round with a second row per pixel: where the point has a distance sample and the eight corners of
// its cell all hold a colour, the luminance of the model there minus the luminance of the input pixel is a second residual and
// color_weight times the luminance's gradient its normal, J = [h, q x h] -- the form of the geometric row, so the 29 sums, the
// reduction, the ticket hand-off and the solve are vh_icp.hip's functions, called, and the two rows share one system.
#pragma once

namespace vh {

struct SdfColorTrackParams {
    float T[12];         // rows 0..2 of the camera -> world estimate (step API; Align takes them from state->delta)
    float distThres;
    float colorWeight;   // > 0 (the host runs sdf_round_kernel where there is no photometric row to form)
    float colorThres;
    int32_t npix;
};

// The cell of the VH_SAMPLE_TRILINEAR sample at u and the blocks of its eight corners: the corner walk of sample_trilinear
// (vh_sample.hip) up to the pointers, which a second volume at the same indices needs.  (sample_trilinear, color_points_kernel
// and merge_color_trilinear keep their own statement of it: their kernels' code stays as compiled.)  Called by every lane of
// the wave, with or without a point (inDomain false).
struct SampleCell {
    int i[3];            // the voxel of corner 0
    float t[3];
    int cross;           // bit a: the cell crosses a block face on axis a
    int ptr[8];          // VH_FREE_BLOCK where the corner's block is absent (or inDomain is false)
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
    const int cross = ((cell.i[0] & 7) == 7 ? 1 : 0) | ((cell.i[1] & 7) == 7 ? 2 : 0) | ((cell.i[2] & 7) == 7 ? 4 : 0);
    cell.cross = cross;
    const SampleRuns runs = sample_runs(lane, kx, ky, kz);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
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

// sample_trilinear's lerp nest and corner-difference gradient over eight values
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

// Y of a colour word (or an rgba pixel): an integer sum, then one conversion and one division; 0..1
__device__ __forceinline__ float color_luminance(uint32_t w)
{
    return (float)(77u * (w & 255u) + 150u * ((w >> 8) & 255u) + 29u * ((w >> 16) & 255u)) / 65280.0f;
}

// One launch per round on the grid vh_icp_create chose: sdf_round_kernel's loop (vh_track.hip) with the photometric row.  The
// look-ups of sample_cell are shared across the lanes of a wave, so every lane runs every pass: the trip count is the same for
// the whole grid, a lane beyond the image takes part without a point, and nothing returns before the last sample.  The colour
// words are read behind the cross-lane part, by the lanes whose pixel is geometrically kept: eight valid corners, so every
// pointer names a block, inside the colour volume as it is inside the SDF volume.
//   useState, points / sdf / gradient: as sdf_round_kernel
//   colorRes / colorGrad (kWriteMaps): per pixel e (NaN where the pixel has no photometric row) and gC (0, 0, 0 where none)
template <bool kWriteMaps>
__global__ __launch_bounds__(kIcpThreads) void sdf_color_round_kernel(const FrameParams fp, const DevPtrs dp, SdfColorTrackParams tp,
                                                                      const float4 *__restrict__ input,
                                                                      const uint32_t *__restrict__ rgba,
                                                                      const uint32_t *__restrict__ color,
                                                                      float *__restrict__ partials, float *__restrict__ points,
                                                                      float *__restrict__ sdfOut, float *__restrict__ gradOut,
                                                                      float *__restrict__ colorRes, float *__restrict__ colorGrad,
                                                                      IcpState *__restrict__ state, int useState, int solve)
{
    __shared__ float4 sums4[kIcpSumFloats / 4];
    __shared__ float sm[8][kIcpStride];
    __shared__ float total[kIcpStride];
    __shared__ int drawn;
    float *sums = reinterpret_cast<float *>(sums4);
    if (useState) {
        if (state->done) return;                    // (the whole grid)
#pragma unroll
        for (int i = 0; i < 12; ++i) tp.T[i] = state->delta[i];
    }
    float acc[kIcpTerms];
#pragma unroll
    for (int k = 0; k < kIcpTerms; ++k) acc[k] = 0.0f;
    const int lane = threadIdx.x & (kWave - 1);
    const int stride = gridDim.x * kIcpThreads;
    const int passes = (tp.npix + stride - 1) / stride;
    const float nan = __builtin_nanf("");
    for (int pass = 0; pass < passes; ++pass) {
        const int idx = pass * stride + blockIdx.x * kIcpThreads + threadIdx.x;
        const bool inImage = idx < tp.npix;
        const float4 p = inImage ? input[idx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const bool have = p.z != 0.0f;              // the ICP's rule (icp_project)
        float q[3] = {0.0f, 0.0f, 0.0f}, u[3] = {nan, nan, nan};
        if (have) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                q[r] = ((tp.T[4 * r + 0] * p.x + tp.T[4 * r + 1] * p.y) + tp.T[4 * r + 2] * p.z) + tp.T[4 * r + 3];
                u[r] = q[r] / fp.voxelSize;
            }
        }
        const bool inDomain = __builtin_fabsf(u[0]) < kSampleDomain && __builtin_fabsf(u[1]) < kSampleDomain &&
                              __builtin_fabsf(u[2]) < kSampleDomain;      // false for NaN
        const SampleCell cell = sample_cell(fp, dp, lane, u, inDomain);
        // ---- no cross-lane read from here to the end of the pass ----
        float v[8];
        bool all = inDomain;
#pragma unroll
        for (int c = 0; c < 8; c += 2) {
            const int index = sample_cell_index(cell, c);
            if (!(cell.cross & 1)) {                // the two corners of an x-edge inside a block: one 16-byte load
                v[c] = v[c + 1] = nan;
                if (cell.ptr[c] != VH_FREE_BLOCK) {
                    const VoxelPair pair = *reinterpret_cast<const VoxelPair *>(dp.blocks + (size_t)cell.ptr[c] + (size_t)index);
                    v[c] = sample_judge(pair.s0, pair.w0).sdf;
                    v[c + 1] = sample_judge(pair.s1, pair.w1).sdf;
                }
            } else {
                v[c] = sample_voxel(dp, cell.ptr[c], index).sdf;
                v[c + 1] = sample_voxel(dp, cell.ptr[c + 1], sample_cell_index(cell, c + 1)).sdf;
            }
            all = all && v[c] == v[c] && v[c + 1] == v[c + 1];
        }
        float s = nan, g[3] = {nan, nan, nan};
        if (all) {
            s = cell_lerp(v, cell.t);
            cell_gradient(v, cell.t, fp.voxelSize, g);
        }
        // no sample: s is NaN and the comparison false
        const bool kept = __builtin_fabsf(s) < tp.distThres && __builtin_isfinite(g[0]) && __builtin_isfinite(g[1]) &&
                          __builtin_isfinite(g[2]);
        if (kept) icp_accumulate(acc, make_float4(q[0], q[1], q[2], 1.0f), make_float4(g[0], g[1], g[2], 0.0f), s);
        float e = nan, gC[3] = {0.0f, 0.0f, 0.0f};
        bool photo = false;
        if (kept) {                                 // (so: in the image, and every cell.ptr a block)
            uint32_t least = 255u;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t w = color[(size_t)cell.ptr[c] + (size_t)sample_cell_index(cell, c)];
                least = min(least, w >> 24);
                v[c] = color_luminance(w);
            }
            if (least != 0u) {
                e = cell_lerp(v, cell.t) - color_luminance(rgba[idx]);
                photo = __builtin_fabsf(e) < tp.colorThres;
                if (photo) cell_gradient(v, cell.t, fp.voxelSize, gC);
                else e = nan;
            }
        }
        if (photo)
            icp_accumulate(acc, make_float4(q[0], q[1], q[2], 1.0f),
                           make_float4(tp.colorWeight * gC[0], tp.colorWeight * gC[1], tp.colorWeight * gC[2], 0.0f),
                           tp.colorWeight * e);
        if constexpr (kWriteMaps) {
            if (inImage) {
                sdfOut[idx] = kept ? s : nan;
                colorRes[idx] = e;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    points[(size_t)idx * 3u + a] = q[a];
                    gradOut[(size_t)idx * 3u + a] = kept ? g[a] : 0.0f;
                    colorGrad[(size_t)idx * 3u + a] = gC[a];
                }
            }
        }
    }
    if (icp_store_record(acc, sums, &drawn, partials, &state->ticket) != (int)gridDim.x - 1) return;
    icp_close_round(partials, state, solve, sm, total);
}

}  // namespace vh
