// vh_api_esdf.hip -- C-ABI, the Euclidean distance to the surface on the lattice: vh_esdf_workspace_bytes, vh_esdf_lattice,
// vh_esdf_lattice_host (kernels: vh_esdf.hip).  Included by vh_api.hip (same translation unit: shares fail(), VH_HIP,
// DeviceGuard, DevBuf, flush_pending()).  The device call only enqueues: the caller brings the workspace.

// What a box of `dims` at `radius` needs, whatever its lo: the sizes of the grown box and of the workspace's six arrays.
struct EsdfPlan {
    bool empty = false;
    unsigned long long gy = 0, gz = 0, words = 0;
    unsigned long long planeBytes = 0, rowsBytes = 0, colsBytes = 0;      // one array of each kind, rounded up to 16 bytes
    unsigned long long total = 0;
};

static int esdf_plan(const int32_t dims[3], int32_t radius, EsdfPlan *p)
{
    if (!dims) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (radius < 1 || radius > VH_ESDF_MAX_RADIUS) return fail(VH_ERR_INVALID_ARGUMENT, "esdf radius outside 1 .. VH_ESDF_MAX_RADIUS");
    unsigned long long voxels = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 0) return fail(VH_ERR_INVALID_ARGUMENT, "negative lattice dimension");
        p->empty = p->empty || dims[a] == 0;
    }
    if (p->empty) return VH_OK;
    for (int a = 0; a < 3; ++a) {
        voxels *= (unsigned long long)dims[a];                             // (at most 2^31 * 2^31 before the check)
        if (voxels > (unsigned long long)INT32_MAX) return fail(VH_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 lattice voxels: ask in parts");
    }
    const unsigned long long R = (unsigned long long)radius, dx = (unsigned long long)dims[0], dy = (unsigned long long)dims[1];
    const auto up16 = [](unsigned long long b) { return (b + 15ull) & ~15ull; };
    p->gy = dy + 2 * R;
    p->gz = (unsigned long long)dims[2] + 2 * R;
    p->words = (dx + 2 * R + 7 + 63) / 64;          // (+7: the row starts at a multiple of 8 at or below lo - R)
    // with at most 2^31 - 1 voxels and R <= 255 the largest array stays below 2^53 bytes
    p->planeBytes = up16(p->gz * p->gy * p->words * 8);
    p->rowsBytes = up16(p->gz * p->gy * dx * 2);
    p->colsBytes = up16(p->gz * dy * dx * 2);
    p->total = 2 * (p->planeBytes + p->rowsBytes + p->colsBytes);
    return VH_OK;
}

extern "C" int vh_esdf_workspace_bytes(const int32_t dims[3], int32_t radius, uint64_t *bytes)
{
    if (!bytes) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    EsdfPlan plan;
    const int rc = esdf_plan(dims, radius, &plan);
    if (rc != VH_OK) return rc;
    *bytes = plan.total;
    return VH_OK;
}

extern "C" int vh_esdf_lattice(vh_context *c, const int32_t lo[3], const int32_t dims[3], int32_t radius, int32_t unknown,
                               void *d_workspace, uint64_t workspace_bytes, int32_t *d_dist2, float *d_distance)
{
    VH_TRACE("vh_esdf_lattice");
    if (!c || !lo || !dims) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    if (unknown != VH_ESDF_UNKNOWN_KEEP && unknown != VH_ESDF_UNKNOWN_FREE && unknown != VH_ESDF_UNKNOWN_OCCUPIED)
        return fail(VH_ERR_INVALID_ARGUMENT, "unknown esdf treatment of unknown voxels");
    EsdfPlan plan;
    { const int rc = esdf_plan(dims, radius, &plan); if (rc != VH_OK) return rc; }
    for (int a = 0; a < 3; ++a) {
        if ((int64_t)lo[a] - radius < (int64_t)INT32_MIN || (int64_t)lo[a] + (int64_t)dims[a] + radius > (int64_t)INT32_MAX)
            return fail(VH_ERR_INVALID_ARGUMENT, "lo - radius or lo + dims + radius beyond int32");
    }
    if (plan.empty) return VH_OK;
    if (!d_dist2 && !d_distance) return fail(VH_ERR_INVALID_ARGUMENT, "an esdf needs an output buffer");
    if (!d_workspace || ((uintptr_t)d_workspace & 15u)) return fail(VH_ERR_INVALID_ARGUMENT, "esdf workspace NULL or not 16-byte aligned");
    if (workspace_bytes < plan.total) return fail(VH_ERR_INVALID_ARGUMENT, "esdf workspace smaller than vh_esdf_workspace_bytes reports");

    EsdfLayout L;
    for (int a = 0; a < 3; ++a) { L.lo[a] = lo[a]; L.dims[a] = dims[a]; }
    L.radius = radius;
    L.unknown = unknown;
    L.gx0 = (int)(((int64_t)lo[0] - radius) & ~(int64_t)7);               // (INT32_MIN is a multiple of 8)
    L.glo[0] = lo[1] - radius;
    L.glo[1] = lo[2] - radius;
    L.gy = plan.gy;
    L.gz = plan.gz;
    L.words = plan.words;
    L.brick0[0] = L.gx0 >> 3;
    L.bricks[0] = (int)(plan.words * 8);
    for (int a = 1; a < 3; ++a) {
        L.brick0[a] = L.glo[a - 1] >> 3;
        L.bricks[a] = (int)((((int64_t)lo[a] + dims[a] + radius - 1) >> 3) - L.brick0[a] + 1);
    }
    const unsigned long long bricks = (unsigned long long)L.bricks[0] * (unsigned long long)L.bricks[1] * (unsigned long long)L.bricks[2];

    DeviceGuard guard(c->device);
    { const int frc = flush_pending(c); if (frc != VH_OK) return frc; }      // the frames queued so far are part of the model
    FrameParams fp = c->fp;
    DevPtrs dp = model_ptrs(c);

    uint8_t *at = static_cast<uint8_t *>(d_workspace);
    unsigned long long *planeIn = reinterpret_cast<unsigned long long *>(at);
    unsigned long long *planeOut = reinterpret_cast<unsigned long long *>(at + plan.planeBytes);
    at += 2 * plan.planeBytes;
    uint16_t *rowsP = reinterpret_cast<uint16_t *>(at), *rowsN = reinterpret_cast<uint16_t *>(at + plan.rowsBytes);
    at += 2 * plan.rowsBytes;
    uint16_t *colsP = reinterpret_cast<uint16_t *>(at), *colsN = reinterpret_cast<uint16_t *>(at + plan.colsBytes);
    const auto grid_of = [](unsigned long long n) { return (unsigned)std::min<unsigned long long>(n, 1ull << 20); };

    const int launches = c->esdfLaunches ? c->esdfLaunches : 4;            // (fewer than four: a timing run, tools/esdf_time.py)
    hipLaunchKernelGGL(esdf_classify_kernel, dim3(grid_of(bricks)), dim3(256), 0, c->stream, fp, dp, L, bricks, planeIn, planeOut);
    VH_HIP(hipGetLastError());
    if (launches < 2) return VH_OK;

    const unsigned long long dx = (unsigned long long)dims[0], dy = (unsigned long long)dims[1], dz = (unsigned long long)dims[2];
    const unsigned long long tilesX = (dx + 255) / 256, rowTiles = tilesX * L.gy * L.gz;
    hipLaunchKernelGGL(esdf_row_kernel, dim3(grid_of(rowTiles)), dim3(256), 0, c->stream, L, rowTiles, tilesX, planeIn, planeOut, rowsP,
                       rowsN);
    VH_HIP(hipGetLastError());
    if (launches < 3) return VH_OK;

    const auto axis_of = [&](unsigned long long inner, unsigned long long lenOut, unsigned long long outer) {
        EsdfAxis A;
        A.inner = inner;
        A.lenOut = lenOut;
        A.tilesInner = (inner + 63) / 64;
        A.tilesAxis = (lenOut + kEsdfTileAxis - 1) / kEsdfTileAxis;
        A.numTiles = A.tilesInner * A.tilesAxis * outer;
        A.radius = radius;
        return A;
    };
    const EsdfAxis ay = axis_of(dx, dy, L.gz), az = axis_of(dx * dy, dz, 1);
    EsdfSelect none{};
    hipLaunchKernelGGL(esdf_axis_kernel<false>, dim3(grid_of(ay.numTiles)), dim3(256), 0, c->stream, ay, L, rowsP, rowsN, colsP, colsN, none);
    VH_HIP(hipGetLastError());
    if (launches < 4) return VH_OK;
    EsdfSelect sel;
    sel.planeIn = planeIn;
    sel.planeOut = planeOut;
    sel.dist2 = d_dist2;
    sel.distance = d_distance;
    sel.voxelSize = fp.voxelSize;
    hipLaunchKernelGGL(esdf_axis_kernel<true>, dim3(grid_of(az.numTiles)), dim3(256), 0, c->stream, az, L, colsP, colsN,
                       (uint16_t *)nullptr, (uint16_t *)nullptr, sel);
    VH_HIP(hipGetLastError());
    return VH_OK;
}

// The same with HOST outputs and a workspace of its own, for callers without a HIP runtime of their own (the C++ facade):
// device buffers for the call's lifetime, one copy back, synchronises.  Not a hot path.
extern "C" int vh_esdf_lattice_host(vh_context *c, const int32_t lo[3], const int32_t dims[3], int32_t radius, int32_t unknown,
                                    int32_t *h_dist2, float *h_distance)
{
    if (!c || !lo || !dims) return fail(VH_ERR_INVALID_ARGUMENT, "null argument");
    EsdfPlan plan;
    { const int rc = esdf_plan(dims, radius, &plan); if (rc != VH_OK) return rc; }
    if (plan.empty || (!h_dist2 && !h_distance))
        return vh_esdf_lattice(c, lo, dims, radius, unknown, nullptr, 0, h_dist2, h_distance);      // nothing to copy: its answer
    DeviceGuard guard(c->device);
    const size_t n = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
    DevBuf<uint4> work;                                                      // (16-byte elements: aligned)
    DevBuf<int32_t> d2;
    DevBuf<float> dist;
    int rc = work.alloc((size_t)(plan.total / 16), "esdf workspace");
    if (rc == VH_OK && h_dist2) rc = d2.alloc(n, "esdf dist2");
    if (rc == VH_OK && h_distance) rc = dist.alloc(n, "esdf distance");
    if (rc != VH_OK) return rc;
    const int timingOnly = c->esdfLaunches;            // (a truncated call writes nothing: never copy that to the caller)
    c->esdfLaunches = 0;
    rc = vh_esdf_lattice(c, lo, dims, radius, unknown, work.get(), plan.total, h_dist2 ? d2.get() : nullptr,
                         h_distance ? dist.get() : nullptr);
    c->esdfLaunches = timingOnly;
    if (rc != VH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (h_dist2) VH_HIP(hipMemcpyAsync(h_dist2, d2, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (h_distance) VH_HIP(hipMemcpyAsync(h_distance, dist, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    VH_HIP(hipStreamSynchronize(c->stream));           // (before the device buffers go)
    return VH_OK;
}
