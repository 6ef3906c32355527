// vh_api_track_color.hip -- C-ABI, tracking against the model's colour and shape: vh_sdf_color_build_system,
// vh_sdf_color_residuals, vh_sdf_color_align, vh_fusion_step_sdf_color (kernel: vh_track_color.hip).  Included by vh_api.hip
// behind vh_api_track.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, flush_pending(), struct vh_icp,
// system_from_sums(), all_finite(), sdf_track_check() and sdf_round()).
// Where no photometric row can be formed -- color_weight == 0, a context without a colour volume, a view table (whose ptrs
// address records, which carry no colour) -- the round launched is vh_sdf_*'s own, so the answer has its bits.

static int sdf_color_check(const vh_context *c, const vh_icp *p, float dist_thres, float color_weight, float color_thres)
{
    if (!std::isfinite(color_weight) || color_weight < 0.0f) return fail(VH_ERR_INVALID_ARGUMENT, "color_weight must be finite and >= 0");
    if (!std::isfinite(color_thres) || !(color_thres > 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "color_thres must be finite and > 0");
    return sdf_track_check(c, p, dist_thres);
}

static bool sdf_color_rows(vh_context *c, float color_weight) { return color_weight != 0.0f && c->color && !c->viewBlocks; }

// one round with the photometric row (sdf_color_rows() holds)
static void sdf_color_round(vh_context *c, vh_icp *p, const SdfColorTrackParams &tp, const vh_float4 *d_input, const uint32_t *d_rgba,
                            float *d_points, float *d_sdf, float *d_gradient, float *d_color_residual, float *d_color_gradient,
                            int useState, int solve)
{
    const float4 *in = reinterpret_cast<const float4 *>(d_input);
    const uint32_t *color = c->color.get();
    if (d_points)
        hipLaunchKernelGGL(sdf_color_round_kernel<true>, dim3(p->blocks), dim3(kIcpThreads), 0, c->stream, c->fp, c->dp, tp, in, d_rgba,
                           color, p->partials.get(), d_points, d_sdf, d_gradient, d_color_residual, d_color_gradient, p->state.get(),
                           useState, solve);
    else
        hipLaunchKernelGGL(sdf_color_round_kernel<false>, dim3(p->blocks), dim3(kIcpThreads), 0, c->stream, c->fp, c->dp, tp, in, d_rgba,
                           color, p->partials.get(), (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr,
                           (float *)nullptr, p->state.get(), useState, solve);
}

static int sdf_color_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, const float pose[16],
                            float dist_thres, float color_weight, float color_thres, float *d_points, float *d_sdf, float *d_gradient,
                            float *d_color_residual, float *d_color_gradient, vh_icp_system *out)
{
    if (!all_finite(pose, 16)) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
    int rc = sdf_color_check(c, p, dist_thres, color_weight, color_thres);
    if (rc != VH_OK) return rc;
    if (!sdf_color_rows(c, color_weight)) {
        DeviceGuard guard(c->device);
        if (d_points) {                              // no photometric row anywhere: e = NaN, gC = 0
            const size_t npix = (size_t)p->width * (size_t)p->height;
            VH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_color_residual), 0x7fc00000, npix, c->stream));
            VH_HIP(hipMemsetAsync(d_color_gradient, 0, sizeof(float) * 3u * npix, c->stream));
        }
        return sdf_system(c, p, d_input, pose, dist_thres, d_points, d_sdf, d_gradient, out);
    }
    DeviceGuard guard(c->device);
    if ((rc = flush_pending(c)) != VH_OK) return rc;        // the frames queued so far are part of the model
    SdfColorTrackParams tp;
    std::memcpy(tp.T, pose, sizeof tp.T);
    tp.distThres = dist_thres;
    tp.colorWeight = color_weight;
    tp.colorThres = color_thres;
    tp.npix = p->width * p->height;
    VH_HIP(hipMemsetAsync(p->state, 0, sizeof(IcpState), c->stream));
    sdf_color_round(c, p, tp, d_input, d_rgba, d_points, d_sdf, d_gradient, d_color_residual, d_color_gradient, 0, 0);
    VH_HIP(hipGetLastError());
    IcpState &hs = *p->hostState;
    VH_HIP(hipMemcpyAsync(&hs, p->state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    system_from_sums(hs.sums, out);
    return VH_OK;
}

extern "C" int vh_sdf_color_build_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba,
                                         const float pose[16], float dist_thres, float color_weight, float color_thres,
                                         vh_icp_system *out)
{
    VH_TRACE("vh_sdf_color_build_system");
    if (!c || !p || !d_input || !d_rgba || !pose || !out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_color_system(c, p, d_input, d_rgba, pose, dist_thres, color_weight, color_thres, nullptr, nullptr, nullptr, nullptr,
                            nullptr, out);
}

extern "C" int vh_sdf_color_residuals(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, const float pose[16],
                                      float dist_thres, float color_weight, float color_thres, float *d_points, float *d_sdf,
                                      float *d_gradient, float *d_color_residual, float *d_color_gradient, vh_icp_system *out)
{
    VH_TRACE("vh_sdf_color_residuals");
    if (!c || !p || !d_input || !d_rgba || !pose || !d_points || !d_sdf || !d_gradient || !d_color_residual || !d_color_gradient || !out)
        return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_color_system(c, p, d_input, d_rgba, pose, dist_thres, color_weight, color_thres, d_points, d_sdf, d_gradient,
                            d_color_residual, d_color_gradient, out);
}

// vh_sdf_align's chain of one-launch rounds with the joint round.
extern "C" int vh_sdf_color_align(vh_context *c, vh_icp *p, const vh_float4 *d_input, const uint32_t *d_rgba, float dist_thres,
                                  float color_weight, float color_thres, int32_t max_iters, double pose[16], vh_icp_system *last,
                                  int32_t *iterations)
{
    VH_TRACE("vh_sdf_color_align");
    if (!c || !p || !d_input || !d_rgba || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (max_iters < 0 || max_iters > kIcpMaxIters) return fail(VH_ERR_INVALID_ARGUMENT, "vh_sdf_color_align: max_iters outside 0..65536");
    IcpState start;
    std::memset(&start, 0, sizeof start);
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(pose[i]) || !std::isfinite((float)pose[i])) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
        start.T[i] = pose[i];
        start.delta[i] = (float)pose[i];
    }
    int rc = sdf_color_check(c, p, dist_thres, color_weight, color_thres);
    if (rc != VH_OK) return rc;
    if (!sdf_color_rows(c, color_weight)) return vh_sdf_align(c, p, d_input, dist_thres, max_iters, pose, last, iterations);
    DeviceGuard guard(c->device);
    if ((rc = flush_pending(c)) != VH_OK) return rc;
    IcpState &hs = *p->hostState;
    hs = start;
    VH_HIP(hipMemcpyAsync(p->state, &hs, sizeof hs, hipMemcpyHostToDevice, c->stream));
    SdfColorTrackParams tp;
    std::memset(tp.T, 0, sizeof tp.T);
    tp.distThres = dist_thres;
    tp.colorWeight = color_weight;
    tp.colorThres = color_thres;
    tp.npix = p->width * p->height;
    for (int it = 0; it < max_iters; ++it)
        sdf_color_round(c, p, tp, d_input, d_rgba, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(&hs, p->state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(pose, hs.T, 16 * sizeof(double));
    if (last) system_from_sums(hs.sums, last);
    if (iterations) *iterations = hs.rounds - (hs.done ? 1 : 0);
    return VH_OK;
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
    int rc = sdf_color_check(c, p, dist_thres, color_weight, color_thres);
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
