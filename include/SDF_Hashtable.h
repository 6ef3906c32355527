/*
 * SDF_Hashtable.h -- C++ host facade with the reference's class interface
 * (SDF_Hashtable.h:24-42 / SDF_Hashtable.cpp) on top of the C-ABI in
 * voxelhash.h.  Source-compatible for the hot path:
 *
 *     SDF_Hashtable table;                       // common.h defaults
 *     table.integrate(pose, d_verts, d_normals); // SDF_Hashtable.cpp:11-40
 *
 * The GL interop members (registerGLtoCUDA / unmapCUDApointers,
 * SDF_Hashtable.cpp:42-58) are kept as no-ops: the compact table, its counter
 * and the SDF volume are library-owned device buffers.  raycast() stands in
 * for SDFRenderer::render(const glm::mat4&) (SDFRenderer.h:38).
 */
#ifndef SDF_HASHTABLE_H
#define SDF_HASHTABLE_H

#include <cstdint>
#include <vector>

#include "voxelhash.h"
#include "voxelhash_dist.h"

/* row-major 4x4, the only part of cuda_SimpleMatrixUtil.h:800-1100 the path uses */
struct float4x4 {
    float entries[16];
    float4x4() {}
    explicit float4x4(const float values[16]) { for (int i = 0; i < 16; ++i) entries[i] = values[i]; }
    void setIdentity() { for (int i = 0; i < 16; ++i) entries[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
    float &operator()(int r, int c) { return entries[4 * r + c]; }
    float operator()(int r, int c) const { return entries[4 * r + c]; }
};

class SDFRenderer;   /* not part of this build; kept so signatures compile */

class SDF_Hashtable {
    vh_context *ctx_;
    vh_dist *dist_;                                    /* multi-GPU constructor: this rank of the sharded table (owns ctx_) */
    HashTableParams h_hashtableParams;

public:
    SDF_Hashtable();                                   /* common.h:39-50, 640x480, REFERENCE semantics */
    SDF_Hashtable(const HashTableParams &params, int width, int height, int semantics);
    /* One rank of ONE logical table sharded by bucket range over `world` GPUs, one camera per rank (voxelhash_dist.h):
     * params.numBuckets = all buckets, params.numVoxelBlocks = per rank; uniqueId: the 128 bytes of
     * SDF_Hashtable::uniqueId() drawn by one rank and handed to all (any out-of-band channel); `batch` frames per
     * camera travel in one exchange; kInv: K^-1 of the cameras (the frames are uint16 sensor images).  The frames enter
     * through integrateExchange(); raycast() renders this rank's view through the whole table. */
    SDF_Hashtable(const HashTableParams &params, int width, int height, int semantics, int rank, int world, int batch,
                  const char uniqueId[VH_DIST_ID_BYTES], const float kInv[9], int device = -1);
    static void uniqueId(char id[VH_DIST_ID_BYTES]);
    /* the id of an in-process loop-back group (vh_dist_loopback_id): `world` SDF_Hashtable ranks of ONE process, one host
     * thread per rank, exchange by device copies instead of RCCL -- the N > 1 host on a single-GPU box */
    static void loopbackId(char id[VH_DIST_ID_BYTES]);
    /* `batch` frames of this rank's camera (poses: batch*16 row-major floats; d_depth: batch device pointers): queues
     * this exchange and applies an earlier one (vh_dist_step_batch: the one before the previous by default); flush() completes
     * what is in flight.  Collective over the ranks. */
    void integrateExchange(const float *poses, const uint16_t *const *d_depth);
    bool sharded() const { return dist_ != nullptr; }
    ~SDF_Hashtable();
    SDF_Hashtable(const SDF_Hashtable &) = delete;
    SDF_Hashtable &operator=(const SDF_Hashtable &) = delete;

    void integrate(const float4x4 &deltaT, const vh_float4 *d_verts, const vh_float4 *d_normals);
    /* any 16-byte {x,y,z,w} float4 (HIP's float4 included) is accepted as is */
    template <class F4>
    void integrate(const float4x4 &deltaT, const F4 *d_verts, const F4 *d_normals)
    {
        static_assert(sizeof(F4) == sizeof(vh_float4), "vertex map elements must be 16-byte float4");
        integrate(deltaT, reinterpret_cast<const vh_float4 *>(d_verts), reinterpret_cast<const vh_float4 *>(d_normals));
    }
    /* the same frame straight from the uint16 sensor image (preProcess + integrate in one call, no vertex
     * map in memory; Application.cpp:73-74,84); kInv: row-major 3x3 */
    void integrate(const float4x4 &deltaT, const uint16_t *d_depth, const float kInv[9]);
    void raycast(const float4x4 &pose, float *d_depth_out, float zNear = 0.1f, float zFar = 5.0f);
    /* raycast(pose, d_depth_out, d_normal_out) -- depth and, from the same pass, the camera-frame
     * normal of every hit (TSDF gradient; vh_raycast_normals) */
    void raycast(const float4x4 &pose, float *d_depth_out, vh_float4 *d_normal_out, float zNear = 0.1f, float zFar = 5.0f);
    /* depth plus camera-frame vertex and normal maps of the view (what CameraTracking::Align takes as target) */
    void raycast(const float4x4 &pose, float *d_depth_out, vh_float4 *d_vertices_out, vh_float4 *d_normals_out,
                 float zNear = 0.1f, float zFar = 5.0f);
    /* SDFRenderer::drawToFrontAndBack (SDFRenderer.cpp:165-208): nearest front / farthest back face of the
     * allocated blocks' cubes per pixel, as two depth images (vh_render_blocks) */
    void renderBlocks(const float4x4 &pose, float *d_front, float *d_back, float zNear = 0.1f, float zFar = 5.0f);
    /* The model as geometry (vh_extract_mesh: marching tetrahedra, world frame, wound towards free space): positions =
     * 9 floats per triangle, normals (optional) one per vertex in the same layout.  Returns the triangle count.  Synchronises. */
    uint64_t extractMesh(std::vector<float> &positions, std::vector<float> *normals = nullptr);
    /* ... written as a binary little-endian PLY (three vertices per triangle, not welded); returns the triangle count */
    uint64_t saveMeshPly(const char *path, bool withNormals = true);
    /* The indexed form (vh_extract_mesh_indexed: one vertex per cell edge, never welded by position): vertices = 3 floats
     * per vertex, indices = 3 per triangle in extractMesh's order, normals (optional) one per vertex.  Returns the
     * triangle count.  Synchronises. */
    uint64_t extractMeshIndexed(std::vector<float> &vertices, std::vector<uint32_t> &indices, std::vector<float> *normals = nullptr);
    /* ... written as a binary little-endian PLY with shared vertices; returns the triangle count */
    uint64_t saveMeshPlyIndexed(const char *path, bool withNormals = true);
    /* The model as a distance field (vh_sample_sdf, through host buffers): points = 3 floats per point, world metres;
     * mode = VH_SAMPLE_NEAREST or VH_SAMPLE_TRILINEAR; sdf = one float per point, NaN where there is no valid sample;
     * weight (optional) one per point, gradient (optional) three per point, per world metre.  Synchronises. */
    void sampleSdf(const std::vector<float> &points, int mode, std::vector<float> &sdf, std::vector<float> *weight = nullptr,
                   std::vector<float> *gradient = nullptr);
    /* The Euclidean signed distance to the surface on the lattice (vh_esdf_lattice, through host buffers): for the voxels
     * lo <= g < lo + dims (x fastest) the exact signed squared distance, in voxels, to the nearest voxel of the other class up
     * to `radius` voxels (1 .. VH_ESDF_MAX_RADIUS) in dist2 (VH_ESDF_FAR, VH_ESDF_NONE), and / or the same in metres in distance
     * (+-inf, NaN); unknown = VH_ESDF_UNKNOWN_KEEP, _FREE or _OCCUPIED.  At least one of the two outputs.  Synchronises. */
    void esdfLattice(const int32_t lo[3], const int32_t dims[3], int radius, int unknown, std::vector<int32_t> *dist2,
                     std::vector<float> *distance);
    /* The connected pieces of the model (vh_components, through host buffers): target = VH_COMPONENT_INSIDE (the valid voxels
     * with sdf <= 0: what the mesh shows as closed pieces) or VH_COMPONENT_OUTSIDE, connectivity 6 or 14 (the mesh's own
     * tetrahedra); region nullptr = the whole model.  components: one record per piece (global voxel of its root, size) in
     * the rule's order; labels (optional, with lo and dims): for the voxels lo <= g < lo + dims, x fastest, the index of the
     * voxel's piece or VH_COMPONENT_NONE.  Returns the stats.  Synchronises. */
    vh_component_stats components(const vh_mesh_region *region, int target, int connectivity, std::vector<vh_component> &components,
                                  const int32_t *lo = nullptr, const int32_t *dims = nullptr, std::vector<uint32_t> *labels = nullptr);
    /* Takes every piece with fewer than minSize nodes out of the volume (vh_remove_components): voxels {0, 0}, colour 0, the
     * blocks that emptied freed.  Returns the stats.  Synchronises. */
    vh_component_stats removeComponents(uint64_t minSize, const vh_mesh_region *region = nullptr, int target = VH_COMPONENT_INSIDE,
                                        int connectivity = 14);
    /* Where rays meet the surface (vh_cast_rays, through host buffers): rays = 8 floats per ray (origin, t_min, direction, t_max,
     * the layout of vh_ray); depthPlane = four floats (one plane places the samples of all rays: row 2 of a pose's inverse gives
     * the raycast's depths) or nullptr (along each ray); t = one float per ray, NaN where there is no hit; normals (optional)
     * three per ray, world frame; voxels (optional) four per ray: the hit voxel and the status (1 hit, 0 miss, -1 refused).
     * Synchronises. */
    void castRays(const std::vector<float> &rays, const float *depthPlane, std::vector<float> &t, std::vector<float> *normals = nullptr,
                  std::vector<int32_t> *voxels = nullptr);
    /* Taking a fused frame back out (vh_deintegrate*, voxelhash.h "taking a frame back out"): the TSDF update run backwards
     * over the blocks `oldPose` sees, with the frame the pose went in with.  The exact inverse only below the weight cap, with
     * the options of the original frame, up to fp32 rounding; a voxel left with less than half a sample becomes {0, 0}.
     * garbageCollect() directly afterwards frees the blocks the removal emptied.  Asynchronous. */
    void deintegrate(const float4x4 &oldPose, const vh_float4 *d_verts);
    void deintegrateDepth(const float4x4 &oldPose, const uint16_t *d_depth, const float kInv[9]);
    /* ... and in again at the corrected pose: deintegrateDepth(oldPose) + integrate(newPose) */
    void reintegrateDepth(const float4x4 &oldPose, const float4x4 &newPose, const uint16_t *d_depth, const float kInv[9]);
    /* One model into another (vh_merge, voxelhash.h "one model into another"): the TSDF of `src` fused into this table under
     * the rigid row-major 4x4 srcToDst (src world metres -> this model's); mode = VH_SAMPLE_NEAREST or VH_SAMPLE_TRILINEAR; the
     * voxel sizes may differ.  src is only read.  garbageCollect() directly afterwards frees the candidate blocks that stayed
     * empty.  Synchronises. */
    void merge(const SDF_Hashtable &src, const float srcToDst[16], int mode, vh_merge_stats *stats = nullptr);
    /* The model in colour (vh_integrate_depth_color / vh_integrate_color, voxelhash.h "the model in colour"): d_rgba = W*H words
     * r | g << 8 | b << 16 registered to the depth image, averaged into the voxels within `band` metres of the surface with a
     * window of weightMax samples (1..255; 0 only sweeps the colour of voxels that hold nothing).  withDepth: the depth frame is
     * fused first (one RGB-D frame in one call).  Asynchronous. */
    void integrateColor(const float4x4 &pose, const uint16_t *d_depth, const float kInv[9], const uint32_t *d_rgba, float band,
                        int weightMax = 255, bool withDepth = false);
    /* ... and read back at world points through host buffers (vh_sample_color_host): points = 3 floats per point; rgba = one
     * word per point, r | g << 8 | b << 16 | 0xFF << 24, or 0 where there is no colour.  Synchronises. */
    void sampleColor(const std::vector<float> &points, int mode, std::vector<uint32_t> &rgba);
    /* Colour through merging, de-integration and saved models (voxelhash.h, the section of that name): merge() with src's colour
     * carried along in the same launch (vh_merge_color; weightMax 1..255), an RGB-D frame taken back out
     * (vh_deintegrate_depth_color) or moved to its corrected pose (vh_reintegrate_depth_color), and the colour words as a file
     * beside a snapshot (vh_save_color / vh_load_color; load after the snapshot). */
    void mergeColor(const SDF_Hashtable &src, const float srcToDst[16], int mode, int weightMax = 255, vh_merge_stats *stats = nullptr);
    void deintegrateDepthColor(const float4x4 &oldPose, const uint16_t *d_depth, const float kInv[9], const uint32_t *d_rgba, float band);
    void reintegrateDepthColor(const float4x4 &oldPose, const float4x4 &newPose, const uint16_t *d_depth, const float kInv[9],
                               const uint32_t *d_rgba, float band, int weightMax = 255);
    void saveColor(const char *path);
    void loadColor(const char *path);
    /* The model with labels (voxelhash.h, the section of that name): d_labels = W*H uint16 labels registered to the depth image
     * (0: not labelled), cast as one vote each into the voxels within `band` metres of the surface; voteMax 1..65535 caps a
     * voxel's vote count, 0 only sweeps the labels of voxels that hold nothing.  Asynchronous. */
    void integrateLabels(const float4x4 &pose, const uint16_t *d_depth, const float kInv[9], const uint16_t *d_labels, float band,
                         int voteMax = 65535);
    /* ... read back at world points through host buffers (vh_sample_labels_host): words = label | votes << 16 of the nearest
     * voxel per point, 0 where there is no label or fewer than minVotes votes.  Synchronises. */
    void sampleLabels(const std::vector<float> &points, std::vector<uint32_t> &words, int minVotes = 1);
    /* ... counted (vh_label_counts_host): counts[l] = the valid voxels of `region` (nullptr: the whole model) with label l for
     * 1 <= l < nBins, counts[0] = every other valid voxel.  Synchronises. */
    void labelCounts(int nBins, std::vector<uint32_t> &counts, const vh_mesh_region *region = nullptr, int minVotes = 1);
    /* ... and acted on (vh_remove_label): every voxel that carries `label` with at least minVotes votes cleared out of the
     * volume, the blocks that emptied freed.  Returns the stats.  Synchronises. */
    vh_label_stats removeLabel(int label, int minVotes = 1, const vh_mesh_region *region = nullptr);
    /* Block streaming (vh_stream_out_host / vh_stream_in_host, voxelhash.h "block streaming"): streamOut takes every allocated
     * block of `region` out of the model into `records` (key + 512 voxels each, in entry order) and, with `colors`, their 512
     * colour words each -- without it the colour of those blocks is dropped; returns the number of blocks moved.  streamIn puts
     * records back: colors (optional) 512 words per record, status (optional) one VH_STREAM_* per record.  Both synchronise. */
    uint64_t streamOut(const vh_stream_region &region, std::vector<vh_view_record> &records, std::vector<uint32_t> *colors = nullptr);
    void streamIn(const std::vector<vh_view_record> &records, const std::vector<uint32_t> *colors = nullptr,
                  std::vector<int32_t> *status = nullptr, vh_stream_stats *stats = nullptr);
    /* Incremental meshing (vh_changes_host / vh_extract_mesh_blocks_host, voxelhash.h "incremental meshing").  d_state: a DEVICE
     * buffer of changesStateBytes() bytes the caller owns, all zero at first.  changedBlocks lists the blocks of `region`
     * (nullptr: the whole model) that differ from what the state last saw -- changed: 4 int32 per block {x, y, z, flags =
     * VH_CHANGED_SELF | VH_CHANGED_HALO}, in entry order; removed: {x, y, z, 0} -- and advances the state; returns the number
     * of changed blocks.  extractMeshBlocks gives the triangles of a key list (4 int32 per key, the 4th ignored: `changed` as
     * it is): positions = 9 floats per triangle, first = keys + 1 offsets (key j's triangles are first[j] .. first[j + 1]),
     * normals optional; returns the triangle count.  Both synchronise. */
    uint64_t changesStateBytes();
    uint64_t changedBlocks(void *d_state, std::vector<int32_t> &changed, std::vector<int32_t> &removed,
                           const vh_mesh_region *region = nullptr, int what = VH_CHANGES_VOXELS, int halo = VH_CHANGES_HALO_MESH);
    uint64_t extractMeshBlocks(const std::vector<int32_t> &keys, std::vector<float> &positions, std::vector<uint64_t> &first,
                               std::vector<float> *normals = nullptr);
    void registerGLtoCUDA(SDFRenderer &) {}
    void unmapCUDApointers() {}

    int occupiedBlockCount();                          /* synchronises */
    /* README.md:15 lists deletion as a feature; the reference's deleteVoxelEntry
     * (VoxelUtils.cu:544-604) is never called.  Frees every block the last frame saw that holds
     * nothing within sdfThreshold of a surface (vh_garbage_collect). */
    void garbageCollect(float sdfThreshold);
    /* Opt-in extensions (voxelhash.h, vh_set_option): "pipeline" (one launch per frame, the commit and
     * TSDF update of a frame ride in the launch of the next; flush() launches the pending half),
     * "overflow_list", "band_mode", "depth_truncation", "weight_sample", "flatten_variant" (4: the walk-free frame -- the
     * occupancy-index walk in place of flattenKernel's scan of every entry: same results, 2-10x the frame rate on large tables), ... */
    void setOption(const char *name, int value);
    void setAllocBand(float bandMetres);
    void flush();
    /* count frames in count + 1 launches (vh_integrate_batch): poses = count * 16 row-major floats */
    void integrateBatch(int count, const float *poses, const vh_float4 *const *d_verts, const vh_float4 *const *d_normals);
    void setStream(void *hipStream);
    vh_context *context() { return ctx_; }
    const HashTableParams &params() const { return h_hashtableParams; }
};

#endif
