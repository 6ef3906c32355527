// vh_api_rays.hip -- C-ABI, the DDA raycast for arbitrary ray batches: vh_cast_rays (kernel: vh_rays.hip).
// Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard, flush_pending()).
// The device call only enqueues: no scratch, no read-back, no synchronisation.

static_assert(sizeof(vh_ray) == 32, "vh_ray is two 16-byte loads");

extern "C" int vh_cast_rays(vh_context *c, uint64_t n, const vh_ray *d_rays, const float depth_plane[4], float *d_t,
                            float *d_normals, int32_t *d_voxels)
{
    VH_TRACE("vh_cast_rays");
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (n > (uint64_t)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 rays: cast in parts");
    RayPlane plane = {{0.0f, 0.0f, 0.0f, 0.0f}, 0};
    if (depth_plane) {
        for (int i = 0; i < 4; ++i)
            if (!std::isfinite(depth_plane[i])) return fail(VH_ERR_INVALID_ARGUMENT, "depth_plane is not finite");
        for (int i = 0; i < 3; ++i) plane.w[i] = depth_plane[i] * c->fp.voxelSize;       // RaycastArgs::zrow's arithmetic
        plane.w[3] = depth_plane[3];
        plane.shared = 1;
    }
    if (n == 0) return VH_OK;
    if (!d_rays || !d_t) return fail(VH_ERR_INVALID_ARGUMENT, "rays need a ray and a t buffer");
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return fail(VH_ERR_INVALID_ARGUMENT, "d_rays is not 16-byte aligned");
    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // the frames queued so far are part of the model

    FrameParams fp = c->fp;
    DevPtrs dp = model_ptrs(c);
    const unsigned grid = ((unsigned)grid_for((size_t)n, kRaysBlock) + 7u) & ~7u;      // (cast_rays_kernel: a multiple of the 8 XCDs)
    hipLaunchKernelGGL(cast_rays_kernel, dim3(grid), dim3(kRaysBlock), 0, c->stream, fp, dp, plane, (uint32_t)n,
                       reinterpret_cast<const float4 *>(d_rays), d_t, d_normals, d_voxels);
    VH_HIP(hipGetLastError());
    return VH_OK;
}

// The same with HOST buffers, for callers without a HIP runtime of their own (the C++ facade): device buffers for the call's
// lifetime, one copy each way.  Not a hot path.
extern "C" int vh_cast_rays_host(vh_context *c, uint64_t n, const vh_ray *h_rays, const float depth_plane[4], float *h_t,
                                 float *h_normals, int32_t *h_voxels)
{
    if (!c) return fail(VH_ERR_INVALID_ARGUMENT, "null context");
    if (n == 0 || n > (uint64_t)INT32_MAX || !h_rays || !h_t)
        return vh_cast_rays(c, n, nullptr, depth_plane, nullptr, nullptr, nullptr);      // nothing to copy: its answer
    DeviceGuard guard(c->device);
    DevBuf<float> rays, t, nrm;
    DevBuf<int32_t> vox;
    int rc = rays.alloc(n * 8, "rays");
    if (rc == VH_OK) rc = t.alloc(n, "ray hits");
    if (rc == VH_OK && h_normals) rc = nrm.alloc(n * 3, "ray normals");
    if (rc == VH_OK && h_voxels) rc = vox.alloc(n * 4, "ray voxels");
    if (rc != VH_OK) return rc;
    VH_HIP(hipMemcpyAsync(rays, h_rays, sizeof(vh_ray) * n, hipMemcpyHostToDevice, c->stream));
    rc = vh_cast_rays(c, n, reinterpret_cast<const vh_ray *>(rays.get()), depth_plane, t, h_normals ? nrm.get() : nullptr,
                      h_voxels ? vox.get() : nullptr);
    if (rc != VH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    VH_HIP(hipMemcpyAsync(h_t, t, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (h_normals) VH_HIP(hipMemcpyAsync(h_normals, nrm, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    if (h_voxels) VH_HIP(hipMemcpyAsync(h_voxels, vox, sizeof(int32_t) * 4 * n, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));           // (before the device buffers go)
    return VH_OK;
}
