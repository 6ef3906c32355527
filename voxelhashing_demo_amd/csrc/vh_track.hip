// vh_track.hip -- camera tracking against the model itself, by its shape (vh_sdf_align, vh_sdf_build_system, vh_sdf_residuals:
// DESIGN.md 4.12; the rule: include/voxelhash.h, "tracking against the model itself", and tests/sdf_track_ref.py) and by its
// shape and colour together (vh_sdf_color_align, vh_sdf_color_build_system, vh_sdf_color_residuals: DESIGN.md 4.21; the rule:
// "tracking against the model's colour and shape", and tests/sdf_color_track_ref.py).  No counterpart in the reference: the
// geometric rule is Bylow et al., "Real-Time Camera Tracking and 3D Reconstruction Using Signed Distance Functions", RSS 2013;
// the photometric term is that of Kerl et al., "Dense Visual SLAM for RGB-D Cameras", IROS 2013, taken against the fused
// colour volume instead of a key frame.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_sample.hip and vh_icp.hip.
//
// A round is the ICP's round (icp_round_kernel) with the model's own distance field where the ICP has a rendered target:
// every input point is moved by the running camera -> world estimate, the trilinear sample there (sample_trilinear, the
// sample of vh_sample_sdf) is the residual and its gradient the normal, J = [g, q x g].  Nothing is rendered and nothing is
// projected.  The joint round (kPhoto) has a second row per pixel: where the point has a distance sample and the eight corners
// of its cell all hold a colour, the luminance of the model there minus the luminance of the input pixel is a second residual
// and color_weight times the luminance's gradient its normal, J = [h, q x h] -- the form of the geometric row, so the two rows
// share one system.  The 29 sums, their fixed-order reduction, the ticket hand-off and the solve in the last workgroup are
// vh_icp.hip's functions, called.
#pragma once

namespace vh {

struct SdfTrackParams {
    float T[12];         // rows 0..2 of the camera -> world estimate (step API; Align takes them from state->delta)
    float distThres;
    float colorWeight;   // kPhoto: > 0 (the host runs the geometric round where there is no photometric row to form)
    float colorThres;
    int32_t npix;
};

// what vh_sdf_residuals / vh_sdf_color_residuals write per pixel (kWriteMaps)
struct SdfTrackMaps {
    float *points, *sdf, *gradient;      // q (0, 0, 0 where the pixel has no point), the residual (NaN where the pixel is not
                                         // kept) and the gradient (0, 0, 0 where it is not kept)
    float *colorRes, *colorGrad;         // kPhoto: e (NaN where the pixel has no photometric row) and gC (0, 0, 0 where none)
};

// Y of a colour word (or an rgba pixel): an integer sum, then one conversion and one division; 0..1
__device__ __forceinline__ float color_luminance(uint32_t w)
{
    return (float)(77u * (w & 255u) + 150u * ((w >> 8) & 255u) + 29u * ((w >> 16) & 255u)) / 65280.0f;
}

// One launch per round on the grid vh_icp_create chose.  The look-ups of sample_cell are shared across the lanes of a wave, so
// every lane runs every pass: the trip count is the same for the whole grid, a lane beyond the image takes part without a
// point, and nothing returns before the last sample.  The colour words (kPhoto: rgba the input image, color the model's
// volume) are read behind the cross-lane part, by the lanes whose pixel is geometrically kept: eight valid corners, so every
// pointer names a block, inside the colour volume as it is inside the SDF volume.
//   useState: take the estimate from state->delta (Align) instead of tp.T (step API)
template <bool kWriteMaps, bool kPhoto>
__global__ __launch_bounds__(kIcpThreads) void sdf_round_kernel(const FrameParams fp, const DevPtrs dp, SdfTrackParams tp,
                                                                const float4 *__restrict__ input,
                                                                const uint32_t *__restrict__ rgba,
                                                                const uint32_t *__restrict__ color, float *__restrict__ partials,
                                                                const SdfTrackMaps maps, IcpState *__restrict__ state,
                                                                int useState, int solve)
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
        const SampleTrilinear s = sample_trilinear(fp, dp, cell, inDomain);
        // no sample: s.sdf is NaN and the comparison false
        const bool kept = __builtin_fabsf(s.sdf) < tp.distThres && __builtin_isfinite(s.g[0]) && __builtin_isfinite(s.g[1]) &&
                          __builtin_isfinite(s.g[2]);
        if (kept) icp_accumulate(acc, make_float4(q[0], q[1], q[2], 1.0f), make_float4(s.g[0], s.g[1], s.g[2], 0.0f), s.sdf);
        float e = nan, gC[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (kPhoto) {
            bool photo = false;
            if (kept) {                             // (so: in the image, and every cell.ptr a block)
                float y[8];
                uint32_t least = 255u;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const uint32_t w = color[(size_t)cell.ptr[c] + (size_t)sample_cell_index(cell, c)];
                    least = min(least, w >> 24);
                    y[c] = color_luminance(w);
                }
                if (least != 0u) {
                    e = cell_lerp(y, cell.t) - color_luminance(rgba[idx]);
                    photo = __builtin_fabsf(e) < tp.colorThres;
                    if (photo) cell_gradient(y, cell.t, fp.voxelSize, gC);
                    else e = nan;
                }
            }
            if (photo)
                icp_accumulate(acc, make_float4(q[0], q[1], q[2], 1.0f),
                               make_float4(tp.colorWeight * gC[0], tp.colorWeight * gC[1], tp.colorWeight * gC[2], 0.0f),
                               tp.colorWeight * e);
        }
        if constexpr (kWriteMaps) {
            if (inImage) {
                maps.sdf[idx] = kept ? s.sdf : nan;
                if constexpr (kPhoto) maps.colorRes[idx] = e;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    maps.points[(size_t)idx * 3u + a] = q[a];
                    maps.gradient[(size_t)idx * 3u + a] = kept ? s.g[a] : 0.0f;
                    if constexpr (kPhoto) maps.colorGrad[(size_t)idx * 3u + a] = gC[a];
                }
            }
        }
    }
    if (icp_store_record(acc, sums, &drawn, partials, &state->ticket) != (int)gridDim.x - 1) return;
    icp_close_round(partials, state, solve, sm, total);
}

}  // namespace vh
