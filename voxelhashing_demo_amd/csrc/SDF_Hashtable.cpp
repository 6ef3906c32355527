// SDF_Hashtable.cpp -- host facade over the C-ABI; mirrors SDF_Hashtable.cpp:11-40,60-90
// of the reference.  Errors follow the reference convention (checkCudaErrors,
// helper_cuda.h:966-977): message on stderr, then exit(EXIT_FAILURE).
#include "SDF_Hashtable.h"
#include "CameraTracking.h"

#include <cstdio>
#include <cstdlib>

static void check(int rc, const char *where)
{
    if (rc == VH_OK) return;
    std::fprintf(stderr, "SDF_Hashtable: %s failed: %s (%s)\n", where, vh_error_string(rc), vh_last_error());
    std::exit(EXIT_FAILURE);
}

SDF_Hashtable::SDF_Hashtable() : ctx_(nullptr), dist_(nullptr)
{
    vh_default_params(&h_hashtableParams);             // SDF_Hashtable.cpp:62-73
    vh_config cfg;
    cfg.params = h_hashtableParams;
    cfg.width = 640;                                   // common.h:17-18
    cfg.height = 480;
    cfg.semantics = VH_SEM_REFERENCE;
    cfg.device = -1;
    check(vh_create(&cfg, &ctx_), "deviceAllocate");   // :75-79
}

SDF_Hashtable::SDF_Hashtable(const HashTableParams &params, int width, int height, int semantics) : ctx_(nullptr), dist_(nullptr)
{
    h_hashtableParams = params;
    vh_config cfg;
    cfg.params = params;
    cfg.width = width;
    cfg.height = height;
    cfg.semantics = semantics;
    cfg.device = -1;
    check(vh_create(&cfg, &ctx_), "deviceAllocate");
}

// One rank of a table sharded over `world` GPUs (include/voxelhash_dist.h)
SDF_Hashtable::SDF_Hashtable(const HashTableParams &params, int width, int height, int semantics, int rank, int world, int batch,
                             const char uniqueId[VH_DIST_ID_BYTES], const float kInv[9], int device)
    : ctx_(nullptr), dist_(nullptr)
{
    h_hashtableParams = params;
    vh_dist_config cfg;
    cfg.table.params = params;
    cfg.table.width = width;
    cfg.table.height = height;
    cfg.table.semantics = semantics;
    cfg.table.device = device;
    cfg.rank = rank;
    cfg.world = world;
    cfg.batch = batch;
    cfg.key_capacity = 0;
    cfg.packet_format = VH_PACKET_U16;
    for (int i = 0; i < 9; ++i) cfg.k_inv[i] = kInv[i];
    check(vh_dist_create(&cfg, uniqueId, nullptr, &dist_), "vh_dist_create");
    ctx_ = vh_dist_shard(dist_);
}

void SDF_Hashtable::uniqueId(char id[VH_DIST_ID_BYTES]) { check(vh_dist_unique_id(id), "vh_dist_unique_id"); }
void SDF_Hashtable::loopbackId(char id[VH_DIST_ID_BYTES]) { check(vh_dist_loopback_id(id), "vh_dist_loopback_id"); }

void SDF_Hashtable::integrateExchange(const float *poses, const uint16_t *const *d_depth)
{
    check(dist_ ? vh_dist_step_batch(dist_, poses, reinterpret_cast<const void *const *>(d_depth)) : VH_ERR_INVALID_ARGUMENT,
          "integrateExchange");
}

SDF_Hashtable::~SDF_Hashtable()                          // :83-89
{
    if (dist_) vh_dist_destroy(dist_);                   // (owns the shard context)
    else vh_destroy(ctx_);
}

void SDF_Hashtable::integrate(const float4x4 &viewMat, const vh_float4 *verts, const vh_float4 *normals)
{
    // pose + inverse, mutex reset, allocBlocks, flattenIntoBuffer, integrateDepthMap
    // (:15-36) as one asynchronous submission
    check(vh_integrate(ctx_, viewMat.entries, verts, normals), "integrate");
}

void SDF_Hashtable::integrate(const float4x4 &viewMat, const uint16_t *d_depth, const float kInv[9])
{
    check(vh_integrate_depth(ctx_, viewMat.entries, d_depth, kInv), "integrate");
}

void SDF_Hashtable::raycast(const float4x4 &pose, float *d_depth_out, float zNear, float zFar)
{
    // sharded: through all shards, the record slots sized by the library until no view has holes (collective)
    if (dist_) check(vh_dist_raycast_auto(dist_, pose.entries, zNear, zFar, d_depth_out, nullptr, nullptr), "raycast");
    else check(vh_raycast(ctx_, pose.entries, zNear, zFar, d_depth_out), "raycast");
}

void SDF_Hashtable::raycast(const float4x4 &pose, float *d_depth_out, vh_float4 *d_normal_out, float zNear, float zFar)
{
    if (dist_) check(vh_dist_raycast_auto(dist_, pose.entries, zNear, zFar, d_depth_out, d_normal_out, nullptr), "raycast");
    else check(vh_raycast_normals(ctx_, pose.entries, zNear, zFar, d_depth_out, d_normal_out), "raycast");
}

void SDF_Hashtable::raycast(const float4x4 &pose, float *d_depth_out, vh_float4 *d_vertices_out, vh_float4 *d_normals_out,
                            float zNear, float zFar)
{
    // (a sharded table has no vertex-map form: the local shard alone would render a view full of holes)
    check(dist_ ? VH_ERR_INVALID_ARGUMENT : vh_raycast_maps(ctx_, pose.entries, zNear, zFar, d_depth_out, d_vertices_out, d_normals_out),
          dist_ ? "raycast with vertex maps is not available on a sharded table: use raycast(pose, depth, normals)" : "raycast");
}

void SDF_Hashtable::renderBlocks(const float4x4 &pose, float *d_front, float *d_back, float zNear, float zFar)
{
    check(vh_render_blocks(ctx_, pose.entries, zNear, zFar, d_front, d_back), "renderBlocks");
}

uint64_t SDF_Hashtable::extractMesh(std::vector<float> &positions, std::vector<float> *normals)
{
    uint64_t count = 0, got = 0;
    check(vh_extract_mesh_host(ctx_, nullptr, 0, nullptr, nullptr, &count), "extractMesh");
    positions.assign((size_t)count * 9, 0.0f);
    if (normals) normals->assign((size_t)count * 9, 0.0f);
    if (count)
        check(vh_extract_mesh_host(ctx_, nullptr, count, positions.data(), normals ? normals->data() : nullptr, &got), "extractMesh");
    return count;
}

uint64_t SDF_Hashtable::saveMeshPly(const char *path, bool withNormals)
{
    std::vector<float> pos, nrm;
    const uint64_t count = extractMesh(pos, withNormals ? &nrm : nullptr);
    FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "SDF_Hashtable: cannot write %s\n", path); std::exit(EXIT_FAILURE); }
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n",
                 (unsigned long long)(3 * count));
    if (withNormals) std::fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
    std::fprintf(f, "element face %llu\nproperty list uchar int vertex_indices\nend_header\n", (unsigned long long)count);
    for (uint64_t v = 0; v < 3 * count; ++v) {
        std::fwrite(&pos[3 * v], sizeof(float), 3, f);
        if (withNormals) std::fwrite(&nrm[3 * v], sizeof(float), 3, f);
    }
    for (uint64_t t = 0; t < count; ++t) {
        const unsigned char three = 3;
        const int32_t idx[3] = {(int32_t)(3 * t), (int32_t)(3 * t + 1), (int32_t)(3 * t + 2)};
        std::fwrite(&three, 1, 1, f);
        std::fwrite(idx, sizeof(int32_t), 3, f);
    }
    std::fclose(f);
    return count;
}

uint64_t SDF_Hashtable::extractMeshIndexed(std::vector<float> &vertices, std::vector<uint32_t> &indices, std::vector<float> *normals)
{
    uint64_t nv = 0, nt = 0, gv = 0, gt = 0;
    check(vh_extract_mesh_indexed_host(ctx_, nullptr, 0, 0, nullptr, nullptr, nullptr, &nv, &nt), "extractMeshIndexed");
    vertices.assign((size_t)nv * 3, 0.0f);
    indices.assign((size_t)nt * 3, 0u);
    if (normals) normals->assign((size_t)nv * 3, 0.0f);
    if (nv || nt)
        check(vh_extract_mesh_indexed_host(ctx_, nullptr, nv, nt, vertices.data(), normals ? normals->data() : nullptr, indices.data(),
                                           &gv, &gt), "extractMeshIndexed");
    return nt;
}

void SDF_Hashtable::sampleSdf(const std::vector<float> &points, int mode, std::vector<float> &sdf, std::vector<float> *weight,
                              std::vector<float> *gradient)
{
    const uint64_t n = points.size() / 3;
    sdf.assign((size_t)n, 0.0f);
    if (weight) weight->assign((size_t)n, 0.0f);
    if (gradient) gradient->assign((size_t)n * 3, 0.0f);
    check(vh_sample_sdf_host(ctx_, mode, n, points.data(), sdf.data(), weight ? weight->data() : nullptr,
                             gradient ? gradient->data() : nullptr), "sampleSdf");
}

void SDF_Hashtable::esdfLattice(const int32_t lo[3], const int32_t dims[3], int radius, int unknown, std::vector<int32_t> *dist2,
                                std::vector<float> *distance)
{
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) n = n > (uint64_t)INT32_MAX ? n : n * (dims[a] > 0 ? (uint64_t)dims[a] : 0);
    if (n > (uint64_t)INT32_MAX) n = 0;          // (the call refuses such a box)
    if (dist2) dist2->assign(n, 0);
    if (distance) distance->assign(n, 0.0f);
    check(vh_esdf_lattice_host(ctx_, lo, dims, radius, unknown, dist2 ? dist2->data() : nullptr, distance ? distance->data() : nullptr),
          "esdfLattice");
}

vh_component_stats SDF_Hashtable::components(const vh_mesh_region *region, int target, int connectivity,
                                             std::vector<vh_component> &components, const int32_t *lo, const int32_t *dims,
                                             std::vector<uint32_t> *labels)
{
    vh_component_stats st{};
    check(vh_components_host(ctx_, region, target, connectivity, 0, nullptr, nullptr, nullptr, nullptr, &st), "components (count)");
    components.assign((size_t)st.components, vh_component{});
    const bool box = lo && dims && labels;
    if (box) {
        uint64_t n = 1;
        for (int a = 0; a < 3; ++a) n = n > (uint64_t)INT32_MAX ? n : n * (dims[a] > 0 ? (uint64_t)dims[a] : 0);
        labels->assign(n > (uint64_t)INT32_MAX ? 0 : (size_t)n, VH_COMPONENT_NONE);
    }
    check(vh_components_host(ctx_, region, target, connectivity, components.size(), components.empty() ? nullptr : components.data(),
                             box ? lo : nullptr, box ? dims : nullptr, box ? labels->data() : nullptr, &st), "components");
    return st;
}

vh_component_stats SDF_Hashtable::removeComponents(uint64_t minSize, const vh_mesh_region *region, int target, int connectivity)
{
    vh_component_stats st{};
    check(vh_remove_components(ctx_, region, target, connectivity, minSize, &st), "removeComponents");
    return st;
}

void SDF_Hashtable::castRays(const std::vector<float> &rays, const float *depthPlane, std::vector<float> &t, std::vector<float> *normals,
                             std::vector<int32_t> *voxels)
{
    const uint64_t n = rays.size() / 8;
    t.assign((size_t)n, 0.0f);
    if (normals) normals->assign((size_t)n * 3, 0.0f);
    if (voxels) voxels->assign((size_t)n * 4, 0);
    check(vh_cast_rays_host(ctx_, n, reinterpret_cast<const vh_ray *>(rays.data()), depthPlane, t.data(),
                            normals ? normals->data() : nullptr, voxels ? voxels->data() : nullptr), "castRays");
}

void SDF_Hashtable::deintegrate(const float4x4 &oldPose, const vh_float4 *d_verts)
{
    check(vh_deintegrate(ctx_, oldPose.entries, d_verts), "deintegrate");
}

void SDF_Hashtable::deintegrateDepth(const float4x4 &oldPose, const uint16_t *d_depth, const float kInv[9])
{
    check(vh_deintegrate_depth(ctx_, oldPose.entries, d_depth, kInv), "deintegrateDepth");
}

void SDF_Hashtable::reintegrateDepth(const float4x4 &oldPose, const float4x4 &newPose, const uint16_t *d_depth, const float kInv[9])
{
    check(vh_reintegrate_depth(ctx_, oldPose.entries, newPose.entries, d_depth, kInv), "reintegrateDepth");
}

void SDF_Hashtable::merge(const SDF_Hashtable &src, const float srcToDst[16], int mode, vh_merge_stats *stats)
{
    check(vh_merge(ctx_, src.ctx_, srcToDst, mode, stats), "merge");      // (src is only read)
}

void SDF_Hashtable::integrateColor(const float4x4 &pose, const uint16_t *d_depth, const float kInv[9], const uint32_t *d_rgba, float band,
                                   int weightMax, bool withDepth)
{
    check(withDepth ? vh_integrate_depth_color(ctx_, pose.entries, d_depth, kInv, d_rgba, band, weightMax)
                    : vh_integrate_color(ctx_, pose.entries, d_depth, kInv, d_rgba, band, weightMax), "integrateColor");
}

void SDF_Hashtable::sampleColor(const std::vector<float> &points, int mode, std::vector<uint32_t> &rgba)
{
    const uint64_t n = points.size() / 3;
    rgba.assign((size_t)n, 0u);
    check(vh_sample_color_host(ctx_, mode, n, points.data(), rgba.data()), "sampleColor");
}

void SDF_Hashtable::mergeColor(const SDF_Hashtable &src, const float srcToDst[16], int mode, int weightMax, vh_merge_stats *stats)
{
    check(vh_merge_color(ctx_, src.ctx_, srcToDst, mode, weightMax, stats), "mergeColor");      // (src is only read)
}

void SDF_Hashtable::deintegrateDepthColor(const float4x4 &oldPose, const uint16_t *d_depth, const float kInv[9], const uint32_t *d_rgba,
                                          float band)
{
    check(vh_deintegrate_depth_color(ctx_, oldPose.entries, d_depth, kInv, d_rgba, band), "deintegrateDepthColor");
}

void SDF_Hashtable::reintegrateDepthColor(const float4x4 &oldPose, const float4x4 &newPose, const uint16_t *d_depth, const float kInv[9],
                                          const uint32_t *d_rgba, float band, int weightMax)
{
    check(vh_reintegrate_depth_color(ctx_, oldPose.entries, newPose.entries, d_depth, kInv, d_rgba, band, weightMax),
          "reintegrateDepthColor");
}

void SDF_Hashtable::saveColor(const char *path) { check(vh_save_color(ctx_, path), "saveColor"); }

void SDF_Hashtable::loadColor(const char *path) { check(vh_load_color(ctx_, path), "loadColor"); }

void SDF_Hashtable::integrateLabels(const float4x4 &pose, const uint16_t *d_depth, const float kInv[9], const uint16_t *d_labels,
                                    float band, int voteMax)
{
    check(vh_integrate_labels(ctx_, pose.entries, d_depth, kInv, d_labels, band, voteMax), "integrateLabels");
}

void SDF_Hashtable::sampleLabels(const std::vector<float> &points, std::vector<uint32_t> &words, int minVotes)
{
    const uint64_t n = points.size() / 3;
    words.assign((size_t)n, 0u);
    check(vh_sample_labels_host(ctx_, n, points.data(), minVotes, words.data()), "sampleLabels");
}

void SDF_Hashtable::labelCounts(int nBins, std::vector<uint32_t> &counts, const vh_mesh_region *region, int minVotes)
{
    counts.assign(nBins > 0 ? (size_t)nBins : 0, 0u);
    check(vh_label_counts_host(ctx_, region, minVotes, nBins, counts.data()), "labelCounts");
}

vh_label_stats SDF_Hashtable::removeLabel(int label, int minVotes, const vh_mesh_region *region)
{
    vh_label_stats st{};
    check(vh_remove_label(ctx_, region, label, minVotes, &st), "removeLabel");
    return st;
}

uint64_t SDF_Hashtable::streamOut(const vh_stream_region &region, std::vector<vh_view_record> &records, std::vector<uint32_t> *colors)
{
    uint64_t selected = 0, written = 0;
    check(vh_stream_out_host(ctx_, &region, 0, nullptr, nullptr, &selected, &written), "streamOut");
    records.resize((size_t)selected);
    if (colors) colors->assign((size_t)selected * 512, 0u);
    if (selected)
        check(vh_stream_out_host(ctx_, &region, selected, records.data(), colors ? colors->data() : nullptr, &selected, &written), "streamOut");
    records.resize((size_t)written);
    if (colors) colors->resize((size_t)written * 512);
    return written;
}

void SDF_Hashtable::streamIn(const std::vector<vh_view_record> &records, const std::vector<uint32_t> *colors, std::vector<int32_t> *status,
                             vh_stream_stats *stats)
{
    if (colors && colors->size() != records.size() * 512) {
        std::fprintf(stderr, "SDF_Hashtable: streamIn needs 512 colour words per record\n");
        std::exit(EXIT_FAILURE);
    }
    if (status) status->assign(records.size(), 0);
    check(vh_stream_in_host(ctx_, records.size(), records.data(), colors ? colors->data() : nullptr, status ? status->data() : nullptr,
                            stats), "streamIn");
}

uint64_t SDF_Hashtable::changesStateBytes()
{
    uint64_t bytes = 0;
    check(vh_changes_state_bytes(ctx_, &bytes), "changesStateBytes");
    return bytes;
}

uint64_t SDF_Hashtable::changedBlocks(void *d_state, std::vector<int32_t> &changed, std::vector<int32_t> &removed,
                                      const vh_mesh_region *region, int what, int halo)
{
    // a peek for the counts (it advances the state only when there is nothing to list), then the call that takes them
    uint64_t nc = 0, nr = 0;
    check(vh_changes_host(ctx_, d_state, region, what, halo, 0, nullptr, 0, nullptr, &nc, &nr), "changedBlocks");
    changed.assign((size_t)nc * 4, 0);
    removed.assign((size_t)nr * 4, 0);
    if (nc || nr)
        check(vh_changes_host(ctx_, d_state, region, what, halo, nc, nc ? changed.data() : nullptr, nr, nr ? removed.data() : nullptr,
                              &nc, &nr), "changedBlocks");
    if (changed.size() != (size_t)nc * 4 || removed.size() != (size_t)nr * 4) {
        std::fprintf(stderr, "SDF_Hashtable: the model changed between the two calls of changedBlocks\n");
        std::exit(EXIT_FAILURE);
    }
    return nc;
}

uint64_t SDF_Hashtable::extractMeshBlocks(const std::vector<int32_t> &keys, std::vector<float> &positions, std::vector<uint64_t> &first,
                                          std::vector<float> *normals)
{
    const uint64_t n = keys.size() / 4;
    uint64_t count = 0, got = 0;
    first.assign((size_t)n + 1, 0);
    check(vh_extract_mesh_blocks_host(ctx_, n, keys.data(), 0, nullptr, nullptr, first.data(), &count), "extractMeshBlocks");
    positions.assign((size_t)count * 9, 0.0f);
    if (normals) normals->assign((size_t)count * 9, 0.0f);
    if (count)
        check(vh_extract_mesh_blocks_host(ctx_, n, keys.data(), count, positions.data(), normals ? normals->data() : nullptr,
                                          first.data(), &got), "extractMeshBlocks");
    return count;
}

uint64_t SDF_Hashtable::saveMeshPlyIndexed(const char *path, bool withNormals)
{
    std::vector<float> pos, nrm;
    std::vector<uint32_t> idx;
    const uint64_t count = extractMeshIndexed(pos, idx, withNormals ? &nrm : nullptr);
    const uint64_t nv = pos.size() / 3;
    if (nv > (uint64_t)INT32_MAX) { std::fprintf(stderr, "SDF_Hashtable: %llu vertices do not fit a PLY int index\n", (unsigned long long)nv); std::exit(EXIT_FAILURE); }
    FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "SDF_Hashtable: cannot write %s\n", path); std::exit(EXIT_FAILURE); }
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n",
                 (unsigned long long)nv);
    if (withNormals) std::fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
    std::fprintf(f, "element face %llu\nproperty list uchar int vertex_indices\nend_header\n", (unsigned long long)count);
    for (uint64_t v = 0; v < nv; ++v) {
        std::fwrite(&pos[3 * v], sizeof(float), 3, f);
        if (withNormals) std::fwrite(&nrm[3 * v], sizeof(float), 3, f);
    }
    for (uint64_t t = 0; t < count; ++t) {
        const unsigned char three = 3;
        const int32_t tri[3] = {(int32_t)idx[3 * t], (int32_t)idx[3 * t + 1], (int32_t)idx[3 * t + 2]};
        std::fwrite(&three, 1, 1, f);
        std::fwrite(tri, sizeof(int32_t), 3, f);
    }
    std::fclose(f);
    return count;
}

void SDF_Hashtable::garbageCollect(float sdfThreshold)
{
    check(vh_garbage_collect(ctx_, sdfThreshold), "garbageCollect");
}

int SDF_Hashtable::occupiedBlockCount()
{
    vh_counters c;
    check(vh_get_counters(ctx_, &c), "get_counters");
    h_hashtableParams.numOccupiedBlocks = (uint32_t)c.occupied;   // :32
    return c.occupied;
}

void SDF_Hashtable::setStream(void *s) { check(vh_set_stream(ctx_, s), "set_stream"); }
void SDF_Hashtable::setOption(const char *name, int value) { check(vh_set_option(ctx_, name, value), "set_option"); }
void SDF_Hashtable::setAllocBand(float bandMetres) { check(vh_set_alloc_band(ctx_, bandMetres), "set_alloc_band"); }
void SDF_Hashtable::flush() { check(dist_ ? vh_dist_flush(dist_) : vh_flush(ctx_), "flush"); }
void SDF_Hashtable::integrateBatch(int count, const float *poses, const vh_float4 *const *d_verts,
                                   const vh_float4 *const *d_normals)
{
    check(vh_integrate_batch(ctx_, count, poses, d_verts, d_normals), "integrate_batch");
}

// ---------------------------------------------------------------------------
// CameraTracking (CameraTracking.cpp:27-69,118-145)
// ---------------------------------------------------------------------------
CameraTracking::CameraTracking(int w, int h) : icp_(nullptr), width(w), height(h)
{
    deltaTransform.setIdentity();
    // common.h:7-10 scaled with the resolution
    const float sx = (float)w / 640.0f, sy = (float)h / 480.0f;
    const float K[9] = {517.3f * sx, 0, 318.6f * sx, 0, 516.5f * sy, 255.3f * sy, 0, 0, 1};
    setIntrinsic(K);
    check(vh_icp_create(w, h, -1, &icp_), "CameraTracking");
}

CameraTracking::~CameraTracking() { vh_icp_destroy(icp_); }

void CameraTracking::setIntrinsic(const float K[9])
{
    for (int i = 0; i < 9; ++i) K_[i] = K[i];
}

void CameraTracking::setStream(void *hipStream) { check(vh_icp_set_stream(icp_, hipStream), "setStream"); }

void CameraTracking::Align(vh_float4 *d_input, vh_float4 *, vh_float4 *d_target, vh_float4 *d_targetNormals,
                           const uint16_t *, const uint16_t *)
{
    vh_icp_system last;
    int rounds = 0;
    check(vh_icp_align(icp_, d_input, d_target, d_targetNormals, K_, distThres_, maxIters, flags_,
                       deltaTransform.entries, &last, &rounds), "Align");
    globalCorrespondenceError = (float)last.error;
}

int CameraTracking::AlignToModel(SDF_Hashtable &table, const vh_float4 *d_input, float4x4 &pose, int rounds)
{
    vh_icp_system last;
    int steps = 0;
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = (double)pose.entries[i];
    check(vh_sdf_align(table.context(), icp_, d_input, distThres_, rounds, T, &last, &steps), "AlignToModel");
    for (int i = 0; i < 16; ++i) pose.entries[i] = (float)T[i];
    globalCorrespondenceError = (float)last.error;
    return steps;
}

int CameraTracking::AlignToModelColor(SDF_Hashtable &table, const vh_float4 *d_input, const uint32_t *d_rgba, float4x4 &pose, int rounds,
                                      float colorWeight, float colorThres)
{
    vh_icp_system last;
    int steps = 0;
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = (double)pose.entries[i];
    check(vh_sdf_color_align(table.context(), icp_, d_input, d_rgba, distThres_, colorWeight, colorThres, rounds, T, &last, &steps),
          "AlignToModelColor");
    for (int i = 0; i < 16; ++i) pose.entries[i] = (float)T[i];
    globalCorrespondenceError = (float)last.error;
    return steps;
}
