// vh_api_sample.hip -- C-ABI, the model as a distance field: vh_sample_sdf, vh_sample_lattice (kernels: vh_sample.hip).
// Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, flush_pending()).
// Both device calls only enqueue: no scratch, no read-back, no synchronisation.

extern "C" int vh_sample_sdf(vh_context *c, int32_t mode, uint64_t n, const float *d_points, float *d_sdf, float *d_weight,
                             float *d_gradient)
{
    VH_TRACE("vh_sample_sdf");
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (mode != VH_SAMPLE_NEAREST && mode != VH_SAMPLE_TRILINEAR) return fail(VH_ERR_INVALID_ARGUMENT, "unknown sample mode");
    if (n > (uint64_t)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 points: sample in parts");
    if (n == 0) return VH_OK;
    if (!d_points || !d_sdf) return fail(VH_ERR_INVALID_ARGUMENT, "points need a point and an sdf buffer");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // the frames queued so far are part of the model

    FrameParams fp = c->fp;
    DevPtrs dp = model_ptrs(c);
    const unsigned grid = (unsigned)grid_for((size_t)n, 256);
    hipLaunchKernelGGL(sample_points_kernel, dim3(grid), dim3(256), 0, c->stream, fp, dp, (int)mode, (uint32_t)n, d_points, d_sdf,
                       d_weight, d_gradient);
    VH_HIP(hipGetLastError());
    return VH_OK;
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade): device buffers for the call's
// lifetime, one copy each way.  Not a hot path.
extern "C" int vh_sample_sdf_host(vh_context *c, int32_t mode, uint64_t n, const float *h_points, float *h_sdf, float *h_weight,
                                  float *h_gradient)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (n == 0 || n > (uint64_t)INT32_MAX || !h_points || !h_sdf)
        return vh_sample_sdf(c, mode, n, h_points, h_sdf, h_weight, h_gradient);      // nothing to copy: its answer
    DeviceGuard guard(c->device);
    DevBuf<float> pts, sdf, wgt, grd;
    int rc = pts.alloc(n * 3, "sample points");
    if (rc == VH_OK) rc = sdf.alloc(n, "sample sdf");
    if (rc == VH_OK && h_weight) rc = wgt.alloc(n, "sample weights");
    if (rc == VH_OK && h_gradient) rc = grd.alloc(n * 3, "sample gradients");
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemcpyAsync(pts, h_points, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    rc = vh_sample_sdf(c, mode, n, pts, sdf, h_weight ? wgt.get() : nullptr, h_gradient ? grd.get() : nullptr);
    if (rc != VH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    VH_HIP(hipMemcpyAsync(h_sdf, sdf, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (h_weight) VH_HIP(hipMemcpyAsync(h_weight, wgt, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (h_gradient) VH_HIP(hipMemcpyAsync(h_gradient, grd, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));           // (before the device buffers go)
    return VH_OK;
}

extern "C" int vh_sample_lattice(vh_context *c, const int32_t lo[3], const int32_t dims[3], float *d_sdf, float *d_weight)
{
    VH_TRACE("vh_sample_lattice");
    if (!c || !lo || !dims) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    LatticeBox box;
    bool empty = false;
    unsigned long long bricks = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 0) return fail(VH_ERR_INVALID_ARGUMENT, "negative lattice dimension");
        if ((int64_t)lo[a] + (int64_t)dims[a] > (int64_t)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "lo + dims beyond int32");
        empty = empty || dims[a] == 0;
        box.lo[a] = lo[a];
        box.dims[a] = dims[a];
        box.brick0[a] = lo[a] >> 3;
        box.bricks[a] = dims[a] ? ((lo[a] + dims[a] - 1) >> 3) - box.brick0[a] + 1 : 0;
    }
    if (empty) return VH_OK;
    if (!d_sdf) return fail(VH_ERR_INVALID_ARGUMENT, "a lattice needs an sdf buffer");
    bricks = (unsigned long long)box.bricks[0] * (unsigned long long)box.bricks[1];       // at most 2^58
    if (bricks > (~0ull >> 30)) return fail(VH_ERR_INVALID_ARGUMENT, "lattice too large");
    bricks *= (unsigned long long)box.bricks[2];
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }

    FrameParams fp = c->fp;
    DevPtrs dp = model_ptrs(c);
    const unsigned grid = (unsigned)std::min<unsigned long long>(bricks, 1ull << 20);
    hipLaunchKernelGGL(sample_lattice_kernel, dim3(grid), dim3(256), 0, c->stream, fp, dp, box, bricks, d_sdf, d_weight);
    VH_HIP(hipGetLastError());
    return VH_OK;
}
