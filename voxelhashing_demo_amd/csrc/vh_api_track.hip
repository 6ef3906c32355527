// vh_api_track.hip -- C-ABI, tracking against the model itself: vh_sdf_build_system, vh_sdf_residuals, vh_sdf_align,
// vh_fusion_step_sdf (kernel: vh_track.hip).  Included by vh_api.hip behind vh_api_icp.hip (same translation unit: shares
// fail(), VH_HIP, DeviceGuard, flush_pending(), struct vh_icp and system_from_sums()).
// The vh_icp is the workspace: its partial records, its device-resident IcpState, its grid and its image size.

static bool all_finite(const float *v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

static int sdf_track_check(const vh_context *c, const vh_icp *p, float dist_thres)
{
    if (!std::isfinite(dist_thres) || !(dist_thres > 0.0f)) return fail(VH_ERR_INVALID_ARGUMENT, "dist_thres must be finite and > 0");
    if (p->device != c->device || p->stream != c->stream)
        return fail(VH_ERR_INVALID_ARGUMENT, "the tracker workspace must have the table's device and stream");
    return VH_OK;
}

// one round: useState 0 takes the estimate from tp.T, 1 from the device-resident state
static void sdf_round(vh_context *c, vh_icp *p, const SdfTrackParams &tp, const vh_float4 *d_input, float *d_points, float *d_sdf,
                      float *d_gradient, int useState, int solve)
{
    DevPtrs dp = c->dp;
    if (c->viewBlocks) dp.blocks = const_cast<Voxel *>(c->viewBlocks);     // view table: voxels live in the records
    const float4 *in = reinterpret_cast<const float4 *>(d_input);
    if (d_points)
        hipLaunchKernelGGL(sdf_round_kernel<true>, dim3(p->blocks), dim3(kIcpThreads), 0, c->stream, c->fp, dp, tp, in,
                           p->partials.get(), d_points, d_sdf, d_gradient, p->state.get(), useState, solve);
    else
        hipLaunchKernelGGL(sdf_round_kernel<false>, dim3(p->blocks), dim3(kIcpThreads), 0, c->stream, c->fp, dp, tp, in,
                           p->partials.get(), (float *)nullptr, (float *)nullptr, (float *)nullptr, p->state.get(), useState, solve);
}

static int sdf_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const float pose[16], float dist_thres, float *d_points,
                      float *d_sdf, float *d_gradient, vh_icp_system *out)
{
    if (!all_finite(pose, 16)) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
    int rc = sdf_track_check(c, p, dist_thres);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = flush_pending(c)) != VH_OK) return rc;        // the frames queued so far are part of the model
    SdfTrackParams tp;
    std::memcpy(tp.T, pose, sizeof tp.T);
    tp.distThres = dist_thres;
    tp.npix = p->width * p->height;
    VH_HIP(hipMemsetAsync(p->state, 0, sizeof(IcpState), c->stream));
    sdf_round(c, p, tp, d_input, d_points, d_sdf, d_gradient, 0, 0);
    VH_HIP(hipGetLastError());
    IcpState &hs = *p->hostState;
    VH_HIP(hipMemcpyAsync(&hs, p->state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    system_from_sums(hs.sums, out);
    return VH_OK;
}

extern "C" int vh_sdf_build_system(vh_context *c, vh_icp *p, const vh_float4 *d_input, const float pose[16], float dist_thres,
                                   vh_icp_system *out)
{
    VH_TRACE("vh_sdf_build_system");
    if (!c || !p || !d_input || !pose || !out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_system(c, p, d_input, pose, dist_thres, nullptr, nullptr, nullptr, out);
}

extern "C" int vh_sdf_residuals(vh_context *c, vh_icp *p, const vh_float4 *d_input, const float pose[16], float dist_thres,
                                float *d_points, float *d_sdf, float *d_gradient, vh_icp_system *out)
{
    VH_TRACE("vh_sdf_residuals");
    if (!c || !p || !d_input || !pose || !d_points || !d_sdf || !d_gradient || !out) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return sdf_system(c, p, d_input, pose, dist_thres, d_points, d_sdf, d_gradient, out);
}

// A chain of one-launch rounds queued at once, the VH_ICP_PERSISTENT=0 form of vh_icp_align: round i's last workgroup solves
// the system on the device and leaves the new estimate where round i + 1 reads it, rounds behind a stop condition fall
// through, one copy each way.  The start is used as given (no log / exp round trip): a call that takes no step returns it.
extern "C" int vh_sdf_align(vh_context *c, vh_icp *p, const vh_float4 *d_input, float dist_thres, int32_t max_iters, double pose[16],
                            vh_icp_system *last, int32_t *iterations)
{
    VH_TRACE("vh_sdf_align");
    if (!c || !p || !d_input || !pose) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (max_iters < 0 || max_iters > kIcpMaxIters) return fail(VH_ERR_INVALID_ARGUMENT, "vh_sdf_align: max_iters outside 0..65536");
    IcpState start;
    std::memset(&start, 0, sizeof start);
    for (int i = 0; i < 16; ++i) {
        if (!std::isfinite(pose[i]) || !std::isfinite((float)pose[i])) return fail(VH_ERR_INVALID_ARGUMENT, "the pose must be finite");
        start.T[i] = pose[i];
        start.delta[i] = (float)pose[i];
    }
    int rc = sdf_track_check(c, p, dist_thres);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = flush_pending(c)) != VH_OK) return rc;
    IcpState &hs = *p->hostState;
    hs = start;
    VH_HIP(hipMemcpyAsync(p->state, &hs, sizeof hs, hipMemcpyHostToDevice, c->stream));
    SdfTrackParams tp;
    std::memset(tp.T, 0, sizeof tp.T);
    tp.distThres = dist_thres;
    tp.npix = p->width * p->height;
    for (int it = 0; it < max_iters; ++it) sdf_round(c, p, tp, d_input, nullptr, nullptr, nullptr, 1, 1);
    VH_HIP(hipGetLastError());
    VH_HIP(hipMemcpyAsync(&hs, p->state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(pose, hs.T, 16 * sizeof(double));
    if (last) system_from_sums(hs.sums, last);
    if (iterations) *iterations = hs.rounds - (hs.done ? 1 : 0);
    return VH_OK;
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
    int rc = sdf_track_check(c, p, dist_thres);
    if (rc != VH_OK) return rc;
    DeviceGuard guard(c->device);
    if ((rc = vh_preprocess(d_depth, k_inv, p->width, p->height, d_input_vertices, d_input_normals, c->stream)) != VH_OK) return rc;
    if ((rc = vh_sdf_align(c, p, d_input_vertices, dist_thres, max_iters, pose, last, iterations)) != VH_OK) return rc;
    float p32[16];
    for (int i = 0; i < 16; ++i) p32[i] = (float)pose[i];
    return vh_integrate_depth(c, p32, d_depth, k_inv);
}
