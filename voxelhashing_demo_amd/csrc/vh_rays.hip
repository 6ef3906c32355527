// vh_rays.hip -- the DDA raycast for arbitrary ray batches: vh_cast_rays (the rule: include/voxelhash.h and
// tests/rays_ref.py).  Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_sample.hip (the walk, DdaAxis
// and the gradient come from vh_raycast.hip).
//
// The walk is dda_lane_walk itself, instantiated over RayWalkArgs: what a view keeps uniform (t_max, the plane that places
// the samples, the hang-guard budget) is the ray's own here and lives in registers.  One ray per lane; lanes share nothing,
// so there is no beam front end and no early exit of a wave's lanes is needed by anyone.  The arithmetic is the rule's,
// unfused fp32 in its order: with the rays of a pinhole view and row 2 of the inverse pose as the plane, the outputs are the
// bits of vh_raycast.
#pragma once

namespace vh {

struct RayWalkArgs {
    float tMax;
    float zrow[4];            // the ray parameter of a voxel centre: ((zrow0 * x + zrow1 * y) + zrow2 * z) + zrow3
    int budget;               // hang guard: the ray's step bound
};

struct RayPlane {
    float w[4];               // the shared plane (P0 vs, P1 vs, P2 vs, P3)
    int shared;               // 0: every ray places its samples at the voxel centre's projection onto itself
};

constexpr int kRayStatusHit = 1, kRayStatusMiss = 0, kRayStatusRefused = -1;

// Cells enumerated ahead per round: 2, as raycast_dda_kernel, whose walk this is -- two loads in flight per memory round
// trip.  A candidate costs seven registers and the kernel sits at its bound of 96 with two (3 dwords of scratch), so a
// third would be paid in scratch; 1 and 3 were not measured here (DESIGN.md 4.6 has the per-lane walk's own history).
#ifndef VH_RAYS_K
#define VH_RAYS_K 2
#endif
constexpr int kRaysK = VH_RAYS_K;      // (a macro, as VH_DDA_WAVES: tuning builds compile the alternatives, tools/rays_time.py times them)
// 256 lanes = 4 waves per workgroup, the shape of the other DDA kernels: a wave is the unit that matters (64 consecutive
// rays), a workgroup of four gives the XCD renumbering below runs of 256 rays.  Waves per SIMD: VH_DDA_WAVES (5, at most
// 96 VGPRs), chosen for raycast_dda_kernel on the same walk; the per-ray t_max, plane and budget cost six
// registers more than there (compile-time figures: DESIGN.md 4.10).
constexpr int kRaysBlock = 256;

// The host rounds the grid up to a multiple of 8 workgroups.  Workgroup b runs on XCD b % 8 (each with its own L2): the
// renumbering gives every XCD one contiguous eighth of the ray list, so rays that are neighbours in the list -- and, in a
// list with any order to it, in space -- read their blocks through one L2 (xcd_tile does the same for image tiles).
__global__ __launch_bounds__(kRaysBlock, VH_DDA_WAVES) void cast_rays_kernel(const FrameParams fp, const DevPtrs dp, const RayPlane plane,
                                                                             uint32_t n, const float4 *__restrict__ rays,
                                                                             float *__restrict__ tOut, float *__restrict__ normalOut,
                                                                             int32_t *__restrict__ voxelOut)
{
    const uint32_t nb = gridDim.x, b = blockIdx.x;
    const uint32_t group = xcd_contiguous(b, nb);
    const uint32_t at = group * (uint32_t)kRaysBlock + threadIdx.x;
    if (at >= n) return;
    const float4 r0 = rays[2 * (size_t)at], r1 = rays[2 * (size_t)at + 1];          // origin, t_min; direction, t_max
    const float O[3] = {r0.x, r0.y, r0.z}, D[3] = {r1.x, r1.y, r1.z};
    const float tMin = r0.w, tMax = r1.w;
    const float vs = fp.voxelSize;
    const float inf = __builtin_inff();
    const float dd = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2];
    bool ok = __builtin_fabsf(tMin) < inf && __builtin_fabsf(tMax) < inf && tMax > tMin;          // (false for NaN)
    DdaAxis ax[3];
    int c[3];
    // the two bounds vh_raycast applies per view, per ray and in double: the step bound (also the ray's budget) and the reach
    double steps = 16.0;
    const double range = (double)tMax - (double)tMin, ends = __builtin_fabs((double)tMax) + __builtin_fabs((double)tMin);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ok = ok && __builtin_fabsf(O[a]) < inf && __builtin_fabsf(D[a]) < inf;
        dda_axis_init(ax[a], O[a] / vs + 0.5f, D[a] / vs);
        c[a] = dda_coord(ax[a], tMin);
        const double e = __builtin_fabs((double)D[a]) / (double)vs;
        steps += 1.01 * range * e + 2.0;
        ok = ok && __builtin_fabs((double)ax[a].G) + ends * e < 8388608.0;
    }
    ok = ok && dd != 0.0f && steps < 4194304.0;
    RayWalkArgs ra;
    ra.tMax = tMax;
    ra.budget = ok ? (int)steps : 0;
    if (plane.shared) {
        ra.zrow[0] = plane.w[0]; ra.zrow[1] = plane.w[1]; ra.zrow[2] = plane.w[2]; ra.zrow[3] = plane.w[3];
    } else {
        const float k = 1.0f / dd;
        ra.zrow[0] = (D[0] * k) * vs; ra.zrow[1] = (D[1] * k) * vs; ra.zrow[2] = (D[2] * k) * vs;
        ra.zrow[3] = -(((O[0] * D[0] + O[1] * D[1]) + O[2] * D[2]) * k);
    }
    const DdaHit h = dda_lane_walk<kRaysK>(fp, dp, ra, ax, c, ok);              // (a refused ray: no walk)
    tOut[at] = h.found ? h.hit : __builtin_nanf("");
    if (voxelOut) {
        int32_t *v = voxelOut + 4 * (size_t)at;
        v[0] = h.found ? h.hx : 0; v[1] = h.found ? h.hy : 0; v[2] = h.found ? h.hz : 0;
        v[3] = h.found ? kRayStatusHit : ok ? kRayStatusMiss : kRayStatusRefused;
    }
    if (normalOut) {
        float w[3] = {0.0f, 0.0f, 0.0f};
        if (h.found) (void)dda_gradient(fp, dp, h.hx, h.hy, h.hz, h.hptr, w);      // world frame, not rotated
        float *o = normalOut + 3 * (size_t)at;
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    }
}

}  // namespace vh
