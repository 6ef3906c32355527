// vh_api_deintegrate.hip -- C-ABI, taking a frame back out: vh_deintegrate, vh_deintegrate_depth, vh_reintegrate_depth
// (kernel: vh_integrate.hip).  Included by vh_api.hip (same translation unit: shares fail(), VH_HIP, DeviceGuard,
// launch(), flush_pending(), vh_set_pose(), vh_flatten()).
// The calls only enqueue: no scratch, no read-back, no synchronisation.

// pose -> the step-level flatten, called as it is -> one launch of the removal over the list it left.  The lock
// epoch, the heap and the hash table are not touched; the compact list and `occupied` are the flatten's.
template <class Depth>
static int deintegrate_impl(vh_context *c, const float pose[16], const Depth &depth)
{
    if (c->viewBlocks) return fail(VH_ERR_INVALID_ARGUMENT, "a view table owns no blocks: its voxels live in the caller's records");
    DeviceGuard guard(c->device);
    int rc = flush_pending(c);                       // the frames queued so far are part of the model
    if (rc == VH_OK) rc = vh_set_pose(c, pose);
    if (rc == VH_OK) rc = vh_flatten(c, nullptr);    // (no occupied_out: the count stays on the device)
    if (rc != VH_OK) return rc;
    // (counted with the TSDF update in vh_kernel_times: integrate_ms; the layout stays)
    rc = launch(c, kPhaseIntegrate, deintegrate_kernel<Depth>, dim3((unsigned)c->integrateGrid), dim3(256), c->fp, c->dp, depth);
    if (rc != VH_OK) return rc;
    VH_HIP(hipGetLastError());
    return VH_OK;
}

extern "C" int vh_deintegrate(vh_context *c, const float pose[16], const vh_float4 *d_verts)
{
    VH_TRACE("vh_deintegrate");
    if (!c || !pose || !d_verts) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return deintegrate_impl(c, pose, vertex_depth(reinterpret_cast<const float4 *>(d_verts)));
}

// Straight from the uint16 sensor image, with DepthSensor's arithmetic: the bits of vh_preprocess + vh_deintegrate.
extern "C" int vh_deintegrate_depth(vh_context *c, const float pose[16], const uint16_t *d_depth, const float k_inv[9])
{
    VH_TRACE("vh_deintegrate_depth");
    if (!c || !pose || !d_depth || !k_inv) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    return deintegrate_impl(c, pose, DepthSensor{d_depth, k_inv[6], k_inv[7], k_inv[8], 5000.0f});   // (unit: CameraTrackingUtils.cu:64)
}

// A composition, not a frame form of its own: out at the old pose, in again at the new one.
extern "C" int vh_reintegrate_depth(vh_context *c, const float old_pose[16], const float new_pose[16], const uint16_t *d_depth,
                                    const float k_inv[9])
{
    VH_TRACE("vh_reintegrate_depth");
    if (!c || !old_pose || !new_pose || !d_depth || !k_inv) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    const int rc = vh_deintegrate_depth(c, old_pose, d_depth, k_inv);
    return rc != VH_OK ? rc : vh_integrate_depth(c, new_pose, d_depth, k_inv);
}
