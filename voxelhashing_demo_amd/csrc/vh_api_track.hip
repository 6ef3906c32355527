// vh_api_track.hip -- C-ABI, tracking against the model itself: vh_sdf_build_system, vh_sdf_residuals, vh_sdf_align,
// vh_fusion_step_sdf, and against its colour and shape together: vh_sdf_color_build_system, vh_sdf_color_residuals,
// vh_sdf_color_align, vh_fusion_step_sdf_color (kernel: vh_track.hip).  Included by vh_api.hip behind vh_api_icp.hip (same
// translation unit: shares fail(), VH_HIP, DeviceGuard, flush_pending(), struct vh_icp, system_from_sums() and
// check_color_frame()).
// The vh_icp is the workspace: its partial records, its device-resident IcpState, its grid and its image size.
// The colour calls pass their image, d_rgba; the geometric calls pass nullptr.  Where no photometric row can be formed --
// color_weight == 0, a context without a colour volume, a view table (whose ptrs address records, which carry no colour) -- the
// round launched is the geometric one, so the answer has vh_sdf_*'s bits.

static bool all_finite(const float *v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// the thresholds of a call
struct SdfTrackLimits { float dist, colorWeight, colorThres; };

static int sdf_track_check(const vh_context *c, const vh_icp *p, const uint32_t *d_rgba, const SdfTrackLimits &lim)
{
    if (d_rgba) {
        if (!std::isfinite(lim.colorWeight) || lim.colorWeight < 0.0f)
            return fail(VH_ERR_INVALID_ARGUMENT, "color_weight must be finite and >= 0");
        if (!std::isfinite(lim.colorThres) || !(lim.colorThres > 0.0f))
            return fail(VH_ERR_INVALID_ARGUMENT, "color_thres must be finite and > 0");
    }
    if (!std::isfinite(lim.dist) || !(lim.dist > 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "dist_thres must be finite and > 0");
    if (p->device != c->device || p->stream != c->stream)
        return fail(VH_ERR_INVALID_ARGUMENT, "the tracker workspace must have the table's device and stream");
    return VH_OK;
}

// the call has photometric rows
static bool sdf_color_rows(const vh_context *c, const uint32_t *d_rgba, const SdfTrackLimits &lim)
{
    return d_rgba && lim.colorWeight != 0.0f && c->color && !c->viewBlocks;
}

static SdfTrackParams sdf_track_params(const vh_icp *p, const float *pose, const SdfTrackLimits &lim)
{
    SdfTrackParams tp;
    if (pose) std::memcpy(tp.T, pose, sizeof tp.T);
    else std::memset(tp.T, 0, sizeof tp.T);
    tp.distThres = lim.dist;
    tp.colorWeight = lim.colorWeight;
    tp.colorThres = lim.colorThres;
    tp.npix = p->width * p->height;
    return tp;
}

// one round, joint where `photo`: useState 0 takes the estimate from tp.T, 1 from the device-resident state; maps: null for none
static void sdf_round(vh_context *c, vh_icp *p, const SdfTrackParams &tp, const vh_float4 *d_input, const uint32_t *d_rgba, bool photo,
                      const SdfTrackMaps *maps, int useState, int solve)
{
    DevPtrs dp = model_ptrs(c);
    const auto kernel = maps ? (photo ? sdf_round_kernel<true, true> : sdf_round_kernel<true, false>)
                             : (photo ? sdf_round_kernel<false, true> : sdf_round_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(p->blocks), dim3(kIcpThreads), 0, c->stream, c->fp, dp, tp, reinterpret_cast<const float4 *>(d_input),
                       photo ? d_rgba : nullptr, photo ? c->color.get() : nullptr, p->partials.get(), maps ? *maps : SdfTrackMaps{},
                       p->state.get(), useState, solve);
}

static int sdf_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, const float pose[16],
                      const SdfTrackLimits &lim, const SdfTrackMaps *maps, vh_icp_system *out)
{
    if (!all_finite(pose, 16)) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
    int rc = sdf_track_check(c, p, d_rgba, lim);
    if (rc != VH_OK) return rc;
    const bool photo = sdf_color_rows(c, d_rgba, lim);
    DeviceGuard guard(c->device);
    if (d_rgba && !photo && maps) {                  // no photometric row anywhere: e = NaN, gC = 0
        const size_t npix = (size_t)p->width * (size_t)p->height;
        VH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(maps->colorRes), 0x7fc00000, npix, c->stream));
        VH_HIP(hipMemsetAsync(maps->colorGrad, 0, sizeof(float) * 3u * npix, c->stream));
    }
    if ((rc = flush_pending(c)) != VH_OK) return rc;        // the frames queued so far are part of the model
    VH_HIP(hipMemsetAsync(p->state, 0, sizeof(IcpState), c->stream));
    sdf_round(c, p, sdf_track_params(p, pose, lim), d_input, d_rgba, photo, maps, 0, 0);
    VH_HIP(hipGetLastError());
    IcpState &hs = *p->hostState;
    VH_HIP(hipMemcpyAsync(&hs, p->state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    system_from_sums(hs.sums, out);
    return VH_OK;
}

// A chain of one-launch rounds queued at once, the VH_ICP_PERSISTENT=0 form of vh_icp_align: round i's last workgroup solves
// the system on the device and leaves the new estimate where round i + 1 reads it, rounds behind a stop condition fall
// through, one copy each way.  The start is used as given (no log / exp round trip): a call that takes no step returns it.
static int sdf_align(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, const SdfTrackLimits &lim,
                     int32_t max_iters, const char *iters_refusal, double pose[16], vh_icp_system *last, int32_t *iterations)
{
    if (max_iters < 0 || max_iters > kIcpMaxIters) return fail(VH_ERR_INVALID_ARGUMENT, iters_refusal);
    IcpState start;
    std::memset(&start, 0, sizeof start);
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(pose[i]) || !std::isfinite((float)pose[i])) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
        start.T[i] = pose[i];
        start.delta[i] = (float)pose[i];
    }
    int rc = sdf_track_check(c, p, d_rgba, lim);
    if (rc != VH_OK) return rc;
    const bool photo = sdf_color_rows(c, d_rgba, lim);
    DeviceGuard guard(c->device);
    if ((rc = flush_pending(c)) != VH_OK) return rc;
    IcpState &hs = *p->hostState;
    hs = start;
    VH_HIP(hipMemcpyAsync(p->state, &hs, sizeof hs, hipMemcpyHostToDevice, c->stream));
    const SdfTrackParams tp = sdf_track_params(p, nullptr, lim);
    for (int it = 0; it < max_iters; ++it) sdf_round(c, p, tp, d_input, d_rgba, photo, nullptr, 1, 1);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(&hs, p->state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(pose, hs.T, 16 * sizeof(double));
    if (last) system_from_sums(hs.sums, last);
    if (iterations) *iterations = hs.rounds - (hs.done ? 1 : 0);
    return VH_OK;
}

extern "C" int vh_sdf_build_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const float pose[16], float dist_thres,
                                   vh_icp_system *out)
{
    VH_TRACE("vh_sdf_build_system");
    if (!c || !p || !d_input || !pose || !out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_system(c, p, d_input, nullptr, pose, {dist_thres, 0.0f, 0.0f}, nullptr, out);
}

extern "C" int vh_sdf_residuals(vh_context *c, vh_icp *p, const vh_float4 *d_input, const float pose[16], float dist_thres,
                                float *d_points, float *d_sdf, float *d_gradient, vh_icp_system *out)
{
    VH_TRACE("vh_sdf_residuals");
    if (!c || !p || !d_input || !pose || !d_points || !d_sdf || !d_gradient || !out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    const SdfTrackMaps maps = {d_points, d_sdf, d_gradient, nullptr, nullptr};
    return sdf_system(c, p, d_input, nullptr, pose, {dist_thres, 0.0f, 0.0f}, &maps, out);
}

extern "C" int vh_sdf_align(vh_context *c, vh_icp *p, const vh_float4 *d_input, float dist_thres, int32_t max_iters, double pose[16],
                            vh_icp_system *last, int32_t *iterations)
{
    VH_TRACE("vh_sdf_align");
    if (!c || !p || !d_input || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_align(c, p, d_input, nullptr, {dist_thres, 0.0f, 0.0f}, max_iters, "vh_sdf_align: max_iters outside 0..65536", pose, last,
                     iterations);
}

extern "C" int vh_sdf_color_build_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba,
                                         const float pose[16], float dist_thres, float color_weight, float color_thres,
                                         vh_icp_system *out)
{
    VH_TRACE("vh_sdf_color_build_system");
    if (!c || !p || !d_input || !d_rgba || !pose || !out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_system(c, p, d_input, d_rgba, pose, {dist_thres, color_weight, color_thres}, nullptr, out);
}

extern "C" int vh_sdf_color_residuals(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, const float pose[16],
                                      float dist_thres, float color_weight, float color_thres, float *d_points, float *d_sdf,
                                      float *d_gradient, float *d_color_residual, float *d_color_gradient, vh_icp_system *out)
{
    VH_TRACE("vh_sdf_color_residuals");
    if (!c || !p || !d_input || !d_rgba || !pose || !d_points || !d_sdf || !d_gradient || !d_color_residual || !d_color_gradient || !out)
        return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    const SdfTrackMaps maps = {d_points, d_sdf, d_gradient, d_color_residual, d_color_gradient};
    return sdf_system(c, p, d_input, d_rgba, pose, {dist_thres, color_weight, color_thres}, &maps, out);
}

extern "C" int vh_sdf_color_align(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, float dist_thres,
                                  float color_weight, float color_thres, int32_t max_iters, double pose[16], vh_icp_system *last,
                                  int32_t *iterations)
{
    VH_TRACE("vh_sdf_color_align");
    if (!c || !p || !d_input || !d_rgba || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_align(c, p, d_input, d_rgba, {dist_thres, color_weight, color_thres}, max_iters,
                     "vh_sdf_color_align: max_iters outside 0..65536", pose, last, iterations);
}

// One tracked frame without a raycast: pre-process -> Align against the model as it stands -> integrate at the new pose.
extern "C" int vh_fusion_step_sdf(vh_context *c, vh_icp *p, const uint16_t *d_depth, const float k_inv[9], float dist_thres,
                                  int32_t max_iters, vh_float4 *d_input_vertices, vh_float4 *d_input_normals, double pose[16],
                                  vh_icp_system *last, int32_t *iterations)
{
    VH_TRACE("vh_fusion_step_sdf");
    if (!c || !p || !d_depth || !k_inv || !d_input_vertices || !d_input_normals || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (p->width != c->fp.width || p->height != c->fp.height)
        return fail(VH_ERR_INVALID_ARGUMENT, "vh_fusion_step_sdf: the tracker must have the table's image size");
    // (what vh_sdf_align would refuse, before the pre-process is queued: a refused call launches nothing)
    if (max_iters < 0 || max_iters > kIcpMaxIters) return fail(VH_ERR_INVALID_ARGUMENT, "vh_fusion_step_sdf: max_iters outside 0..65536");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite((float)pose[i])) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
    int rc = sdf_track_check(c, p, nullptr, {dist_thres, 0.0f, 0.0f});
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = vh_preprocess(d_depth, k_inv, p->width, p->height, d_input_vertices, d_input_normals, c->stream)) != VH_OK) return rc;
    if ((rc = vh_sdf_align(c, p, d_input_vertices, dist_thres, max_iters, pose, last, iterations)) != VH_OK) return rc;
    float p32[16];
    for (int i = 0; i < 16; ++i) p32[i] = (float)pose[i];
    return vh_integrate_depth(c, p32, d_depth, k_inv);
}

// One tracked colour frame without a raycast: pre-process -> joint Align against the model as it stands -> depth and colour
// integrated at the new pose.  Every refusal of a later part is met before the pre-process is queued.
extern "C" int vh_fusion_step_sdf_color(vh_context *c, vh_icp *p, const uint16_t *d_depth, const float k_inv[9], const uint32_t *d_rgba,
                                        float dist_thres, float color_weight, float color_thres, int32_t max_iters, float band,
                                        int32_t weight_max, vh_float4 *d_input_vertices, vh_float4 *d_input_normals, double pose[16],
                                        vh_icp_system *last, int32_t *iterations)
{
    VH_TRACE("vh_fusion_step_sdf_color");
    if (!c || !p || !d_depth || !k_inv || !d_rgba || !d_input_vertices || !d_input_normals || !pose)
        return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (p->width != c->fp.width || p->height != c->fp.height)
        return fail(VH_ERR_INVALID_ARGUMENT, "vh_fusion_step_sdf_color: the tracker must have the table's image size");
    if (max_iters < 0 || max_iters > kIcpMaxIters) return fail(VH_ERR_INVALID_ARGUMENT, "vh_fusion_step_sdf_color: max_iters outside 0..65536");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite((float)pose[i])) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
    int rc = sdf_track_check(c, p, d_rgba, {dist_thres, color_weight, color_thres});
    if (rc == VH_OK) rc = check_color_frame(c, band, weight_max);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = vh_preprocess(d_depth, k_inv, p->width, p->height, d_input_vertices, d_input_normals, c->stream)) != VH_OK) return rc;
    if ((rc = vh_sdf_color_align(c, p, d_input_vertices, d_rgba, dist_thres, color_weight, color_thres, max_iters, pose, last,
                                 iterations)) != VH_OK)
        return rc;
    float p32[16];
    for (int i = 0; i < 16; ++i) p32[i] = (float)pose[i];
    return vh_integrate_depth_color(c, p32, d_depth, k_inv, d_rgba, band, weight_max);
}
