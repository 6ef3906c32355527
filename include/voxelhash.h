/*
 * voxelhash.h -- C-ABI of libvoxelhash_hip.so: the MI355X (gfx950) voxel-hashing
 * TSDF fusion path.  Plain C, plain pointers and sizes; no torch / C++ types.
 *
 * The library replaces the CUDA launcher layer of nilspin/VoxelHashing_demo
 * (VoxelUtils.h:5-13, implemented in VoxelUtils.cu) that SDF_Hashtable.cpp
 * binds to.  Two surfaces are exported:
 *
 *   1. vh_*  -- the explicit-context API (one table per context, one context
 *      per GPU, explicit stream, int status returns).  Everything else is
 *      built on it.
 *   2. the reference's own nine names (section "drop-in names" below) acting
 *      on a process-global default context, so that SDF_Hashtable.cpp links
 *      against this library unchanged apart from passing params by pointer.
 *
 * Device pointers are `hipMalloc`-class addresses (torch CUDA tensors'
 * data_ptr() qualify).  All device work is enqueued on the context's stream
 * and is asynchronous unless a function says it synchronises.  The usual
 * stream contract applies: a buffer handed to a call must be ready ON THAT
 * STREAM (produced there, or ordered before it with an event / a
 * synchronisation), and results are ready on that stream; the library adds
 * no synchronisation between streams.
 *
 * Paths in citations are relative to the reference checkout.
 */
#ifndef VOXELHASH_H
#define VOXELHASH_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* records -- layout identical to VoxelDataStructures.h                */
/* ------------------------------------------------------------------ */

/* VoxelDataStructures.h:12-17; 8 bytes */
typedef struct Voxel { float sdf; float weight; } Voxel;

/* VoxelDataStructures.h:20-26; 20 bytes, 4-byte aligned (the __align__(16)
 * placed before `struct` is ignored by the compilers) */
typedef struct VoxelEntry {
    int32_t pos[3];   /* int3 pos: block coordinate */
    int32_t ptr;      /* first voxel index of the block in the volume, -1 = free */
    int32_t offset;   /* overflow chain link, measured from the home bucket's last slot; 0 = none (always 0
                         unless the option "overflow_list" is on: the list code is dead in the reference) */
} VoxelEntry;

/* VoxelDataStructures.h:29-52; 176 bytes.  Matrices are row-major float4x4. */
typedef struct HashTableParams {
    float    global_transform[16];
    float    inv_global_transform[16];
    uint32_t numBuckets;
    uint32_t bucketSize;
    uint32_t attachedLinkedListSize;   /* iterations of the chain lookup loop (option "overflow_list"; dead code in the reference) */
    uint32_t numVoxelBlocks;
    int32_t  voxelBlockSize;           /* must be 8 */
    float    voxelSize;
    uint32_t numOccupiedBlocks;
    float    maxIntegrationDistance;   /* unused by the reference kernels */
    float    truncScale;               /* unused by the reference kernels (option "depth_truncation") */
    float    truncation;
    uint32_t integrationWeightSample;  /* unused by the reference kernels (option "weight_sample") */
    float    integrationWeightMax;
} HashTableParams;

/* float4 as CUDA/HIP lay it out */
typedef struct vh_float4 { float x, y, z, w; } vh_float4;

/* VoxelDataStructures.h:54-63 -- raw device pointers of one table.  The bucket
 * lock is an 8-byte epoch-stamped claim word per bucket instead of the
 * reference's memset-per-frame int (see DESIGN.md "bucket lock"): epoch in the
 * top 10 bits, then the winner's inverted launch rank, slot and record index. */
typedef struct PtrContainer {
    uint32_t   *d_heap;
    VoxelEntry *d_hashTable;
    VoxelEntry *d_compactifiedHashTable;
    uint64_t   *d_hashTableBucketMutex;
    Voxel      *d_SDFBlocks;
    int32_t    *d_heapCounter;
    int32_t    *d_compactifiedHashCounter;
} PtrContainer;

#define VH_FREE_BLOCK   (-1)          /* VoxelUtils.cu:19 */
#define VH_POS_SENTINEL 0x7fffffff    /* free-slot pos, VoxelUtils.cu:157 on a saturating cvt */

/* ------------------------------------------------------------------ */
/* status codes (the reference exits the process on any CUDA error,    */
/* helper_cuda.h:966-977; this ABI returns a code instead)             */
/* ------------------------------------------------------------------ */
enum {
    VH_OK = 0,
    VH_ERR_INVALID_ARGUMENT = 1,
    VH_ERR_NO_DEVICE = 2,        /* no usable HIP device */
    VH_ERR_OUT_OF_MEMORY = 3,
    VH_ERR_HIP = 4,              /* any other HIP runtime failure; see vh_last_error() */
    VH_ERR_NOT_INITIALISED = 5,  /* drop-in call before deviceAllocate() */
    VH_ERR_SINGULAR = 6,         /* vh_icp_solve: J^T J is not positive definite */
    VH_ERR_TIMEOUT = 7           /* vh_icp_align: a workgroup of the one-launch Align gave up waiting for the others (the call may be
                                  * repeated).  Frames: workgroups of a serialised one-launch frame (overflow list, option "pipeline_overflow") gave up waiting
                                  * for the pending frame's commit phase (option "spin_limit"): frames queued since the last successful
                                  * synchronisation have lost work.  Returned ONCE, by the first call that synchronises with the host and
                                  * sees the counter (vh_synchronize, vh_download*, vh_dist_flush); vh_get_counters reports the count
                                  * (spin_timeouts) without failing.  From then on the context runs such frames as two launches. */
};

/* projection / transform semantics */
enum {
    VH_SEM_REFERENCE = 0,  /* bit-faithful to the reference, quirks included: the projection
                              matrix is K transposed (common.h:16 through
                              cuda_SimpleMatrixUtil.h:316-320), blockInFrustum uses
                              global_transform (VoxelUtils.cu:348), the inverse pose is applied
                              to voxel indices and truncated (VoxelUtils.cu:797-800) */
    VH_SEM_PINHOLE = 1     /* physically meaningful variant used for benchmarks: K, inverse
                              pose in the frustum test plus z > 0, inverse pose in metres */
};

typedef struct vh_config {
    HashTableParams params;   /* as filled by SDF_Hashtable.cpp:62-73 */
    int32_t width;            /* depth image size; the reference hard-wires 640x480 */
    int32_t height;
    int32_t semantics;        /* VH_SEM_* */
    int32_t device;           /* HIP device ordinal, -1 = current device */
} vh_config;

typedef struct vh_counters {
    int32_t  occupied;          /* entries in the compact table (last flatten) */
    int32_t  heap_counter;      /* index of the top free heap slot; -1 = heap empty */
    uint32_t allocated_total;   /* blocks handed out since creation */
    uint32_t heap_exhausted;    /* insertions refused because the heap was empty */
    uint32_t candidates;        /* contenders of the last allocBlocks (demanded, even if the list was full) */
    uint32_t epoch;             /* bucket-lock epoch (= frames since creation) */
    uint32_t bin_overflow;      /* received key bins that exceeded their capacity (keys lost) */
    uint32_t freed_total;       /* blocks returned to the heap since creation (deletion / GC) */
    uint32_t last_freed;        /* ... by the last vh_delete_blocks / vh_garbage_collect */
    uint32_t cand_overflow;     /* contenders dropped since creation because the candidate list of their
                                   frame was full (their keys retry next frame; see "cand_capacity") */
    uint32_t spin_timeouts;     /* ERROR REPORT: workgroups of a serialised one-launch frame (option "overflow_list" with
                                   "pipeline" / vh_integrate_batch / vh_apply_frames_batch) that gave up waiting for the
                                   pending frame's commit phase after "spin_limit" polls (default 2^20, ~1.5 s): that frame
                                   is incomplete; once this is seen here the context runs its overflow-list frames as two
                                   launches each.  0 in every run so far. */
} vh_counters;

/* per-kernel device time, accumulated while profiling is on (HIP events on
 * the context's stream) */
typedef struct vh_kernel_times {
    uint64_t launches;          /* frames accumulated */
    double   alloc_claim_ms;
    double   alloc_commit_ms;
    double   flatten_ms;
    double   integrate_ms;
    double   raycast_ms;
    uint64_t raycast_launches;
    double   frame_scan_claim_ms;        /* fused vh_integrate, launch 1: claim || table walk */
    double   frame_commit_integrate_ms;  /* fused vh_integrate, launch 2: commit + TSDF update */
    double   view_export_ms;             /* vh_export_views: select walk + record packing; vh_stream_out: its pack launch */
    double   view_import_ms;             /* vh_import_view: clear + insert; vh_stream_in: its place launch */
    double   gc_ms;                      /* vh_delete_blocks / vh_garbage_collect, all launches */
    uint64_t gc_calls;
    double   render_blocks_ms;           /* vh_render_blocks, all launches */
    double   frame_pipelined_ms;         /* pipelined frames: the one launch per frame */
} vh_kernel_times;

typedef struct vh_context vh_context;

/* what vh_download copies */
enum {
    VH_BUF_HASH_TABLE = 0,   /* numBuckets*bucketSize VoxelEntry */
    VH_BUF_COMPACT = 1,      /* numBuckets*bucketSize VoxelEntry (first `occupied` valid) */
    VH_BUF_SDF_BLOCKS = 2,   /* numVoxelBlocks*512 Voxel */
    VH_BUF_HEAP = 3          /* numVoxelBlocks uint32 */
};

/* ------------------------------------------------------------------ */
/* explicit-context API                                                */
/* ------------------------------------------------------------------ */

void vh_default_params(HashTableParams *p);          /* common.h:39-50 */
const char *vh_error_string(int code);
const char *vh_last_error(void);                     /* text of the last failure on this thread */
int  vh_device_count(void);                          /* 0 when no GPU is present */

/* SDF_Hashtable::SDF_Hashtable + deviceAllocate + calculateKinectProjectionMatrix
 * (SDF_Hashtable.cpp:60-81, VoxelUtils.cu:169-231).  Also owns the compact
 * table, its counter and the zero-initialised SDF volume, which the reference
 * borrows from OpenGL (SDFRenderer.cpp:34-61). */
int vh_create(const vh_config *cfg, vh_context **out);
int vh_destroy(vh_context *ctx);                     /* deviceFree, VoxelUtils.cu:213-222 */

int vh_set_stream(vh_context *ctx, void *hip_stream);   /* NULL = default stream */
int vh_set_projection(vh_context *ctx, const float m[9]);            /* row-major 3x3 */
int vh_set_raycast_intrinsics(vh_context *ctx, float fx, float fy, float cx, float cy);

/* Opt-in truncation-band allocation (the reference has it commented
 * out, VoxelUtils.cu:632-703): with band > 0 every valid pixel demands the blocks of
 * 2*ceil(band/step)+1 points on its viewing ray at camera depths z + (k-half)*step, step =
 * 4 voxels; the middle sample is the surface point itself.  0 (default) = the reference's
 * surface-block-only allocation.  One insertion per bucket per frame still holds. */
int vh_set_alloc_band(vh_context *ctx, float band_metres);

/* Opt-in extensions, all off by default (= the live reference path), chosen with vh_set_option:
 *   "overflow_list" 1   the bucket overflow list the reference carries as dead code (#ifdef LINKED_LIST_ENABLED,
 *                       VoxelUtils.cu:384-411 lookup, :458-539 insert, :578-602 delete): a key whose home bucket is
 *                       full goes to a free slot among the 9 slots behind the bucket (never another bucket's last
 *                       slot) and is chained from the home bucket's last slot through VoxelEntry::offset, at most
 *                       params.attachedLinkedListSize - 1 chained entries per bucket; both buckets are locked for
 *                       the frame; deletion leaves holes instead of compacting.  Must be set before the first
 *                       frame.  A shard's chains stay inside the shard.  With the list on, vh_alloc_blocks may run
 *                       once per lock epoch (several cameras per epoch: vh_insert_bins / vh_apply_frames_batch).
 *   "pipeline_overflow" one-launch frames ("pipeline", vh_integrate_batch, vh_apply_frames_batch) with the overflow list on are
 *                       serialised inside the launch, and every waiting workgroup pays a cache invalidate: 1 (default) =
 *                       taken only for small launches (up to 512 claim + walk workgroups), larger ones run as two launches
 *                       (C2: 21 us against 53 us); 0 = never; 2 = always.  Results are the same bits either way.
 *   "band_mode"         VH_BAND_RAY (default: vh_set_alloc_band's samples along the viewing ray) or
 *                       VH_BAND_NORMAL_DDA: every block the segment from p - band*n to p + band*n crosses, by a
 *                       block DDA (commented out in the reference, VoxelUtils.cu:632-703); n comes from the
 *                       d_normals argument of vh_alloc_blocks / vh_integrate (preProcess's normal map, camera
 *                       frame), pixels without a normal demand their surface block only.  Not offered by
 *                       vh_integrate_depth and the key-generation calls (they carry no normal map).
 *                       VH_BAND_RAY_DDA: the same block DDA along the pixel's VIEWING RAY -- every block the segment
 *                       from the ray's point at camera depth z - band to its point at z + band crosses (a band that
 *                       would begin behind the camera begins at the surface point): the exact set the samples of
 *                       VH_BAND_RAY approximate, at one transform per segment end and the DDA's divisions per pixel
 *                       instead of a transform and four divisions per sample; needs no normals, offered by every
 *                       entry point.
 *   "depth_truncation" 1   truncation + truncScale * depth in the TSDF update (VoxelUtils.cu:815, getTruncation)
 *   "weight_sample" 1      sample weight max(integrationWeightSample * 1.5 * (1 - (depth - 0.5) / 4.5), 1) instead of
 *                          0.1 (VoxelUtils.cu:808-811, :827) */
#define VH_BAND_RAY        0
#define VH_BAND_NORMAL_DDA 1
#define VH_BAND_RAY_DDA    2

/* SDF_Hashtable.cpp:15-21: stores the pose and its cofactor inverse
 * (cuda_SimpleMatrixUtil.h:944-1069, same summation order, fp32, on the host) */
int vh_set_pose(vh_context *ctx, const float pose[16]);

/* resetHashTableMutexes (VoxelUtils.cu:146-149): bumps the lock epoch instead of clearing 4*numBuckets bytes */
int vh_reset_mutexes(vh_context *ctx);
/* allocBlocks (VoxelUtils.cu:708-716, kernel :606-705): W*H float4 each, d_normals unused as in the reference (:631) */
int vh_alloc_blocks(vh_context *ctx, const vh_float4 *d_verts, const vh_float4 *d_normals);
/* flattenIntoBuffer (VoxelUtils.cu:751-768, kernel :719-749): with occupied_out != NULL it
 * synchronises the stream and returns the count like the reference does; with NULL it stays
 * asynchronous */
int vh_flatten(vh_context *ctx, int32_t *occupied_out);
/* integrateDepthMap (VoxelUtils.cu:844-852, kernel :790-842) over the compact list of the last flatten */
int vh_integrate_depth_map(vh_context *ctx, const vh_float4 *d_verts);

/* SDF_Hashtable::integrate (SDF_Hashtable.cpp:11-40) as one asynchronous call:
 * pose -> epoch bump -> allocBlocks -> flatten -> integrateDepthMap, no host
 * synchronisation and no device->host copy. */
int vh_integrate(vh_context *ctx, const float pose[16],
                 const vh_float4 *d_verts, const vh_float4 *d_normals);

/* The same frame straight from the uint16 sensor image (5000 units = 1 m, 0 = no measurement):
 * preProcess's vertex computation (CameraTrackingUtils.cu:63-73) runs inside the claim phase and the
 * TSDF update reads the image, so no vertex map exists in memory: 2 bytes per pixel in instead of
 * 16.  Equals vh_preprocess + vh_integrate bit for bit.  k_inv: row-major 3x3. */
int vh_integrate_depth(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9]);

/* Pipelined frames.  With vh_set_option(ctx, "pipeline", 1) a frame is ONE launch: vh_integrate enqueues
 * {claim || walk} of its frame together with the {commit + TSDF update} of the PREVIOUS frame, whose
 * results it leaves pending; the pending half is launched by the next vh_integrate / vh_integrate_depth,
 * by vh_flush, and by every call that reads or changes the model (counters, download, raycast, collection,
 * snapshot, step-level calls, vh_set_stream, vh_synchronize ...), so the library's own entry points always
 * see completed frames.  Code that reads the model through raw device pointers (vh_get_device_pointers)
 * calls vh_flush first.  The caller's depth / vertex buffer is only read by the launch of its own frame
 * (the deferred half works from a private copy of the camera-z plane), so buffers may be reused as with
 * the unpipelined calls.  Results equal the unpipelined frames bit for bit, with one documented
 * difference: a frame whose new blocks outnumber the free blocks of the heap allocates none of them
 * (they count as heap_exhausted and retry), where vh_integrate serves as many as there are blocks.
 * With "overflow_list" the frames are still one launch each, but serialised inside it: the claim and walk workgroups of
 * the new frame start when the commit phase of the pending one has finished (and that phase serves as many winners as the
 * heap has blocks, like the unpipelined frame).  bucketSize > 16 runs unpipelined.  vh_integrate_batch / vh_integrate_depth_batch: `count` frames (poses: count*16 host
 * floats; d_verts / d_normals / d_depth: host arrays of `count` device pointers, d_normals may be NULL)
 * in count + 1 launches -- the pipeline switched on for the call and flushed at its end. */
int vh_flush(vh_context *ctx);
int vh_integrate_batch(vh_context *ctx, int32_t count, const float *poses, const vh_float4 *const *d_verts,
                       const vh_float4 *const *d_normals);
int vh_integrate_depth_batch(vh_context *ctx, int32_t count, const float *poses, const uint16_t *const *d_depth,
                             const float k_inv[9]);

/* Stand-in for SDFRenderer::render (SDFRenderer.cpp:210-255): one ray per pixel
 * from `pose`, camera depth of the first +/- zero crossing into d_depth_out
 * (width*height floats, 0 = no hit).  Spec: DESIGN.md "raycast".
 * Two traversals, chosen with vh_set_option(ctx, "raycast_mode", ...):
 *   VH_RAYCAST_DDA (default)  the voxel DDA the reference's shader intends (raycastSDF.frag:121-177,
 *       Amanatides-Woo between the ray's two ends): every voxel the ray passes through between t_min and
 *       t_max, in order, each a sample with the voxel's own {sdf, weight} placed at the camera depth of the
 *       voxel's centre; crossing times are functions of the integer voxel coordinate (no accumulated tMax),
 *       ties as at :156-170; absent blocks and empty 4x4x4-block cells are left in one exact step.
 *   VH_RAYCAST_FIXED_STEP     rounds 1-2: samples at camera depth t_min + i*voxelSize, nearest voxel each.
 * Both: first pair of consecutive valid samples (block allocated, weight > 0) with sdf_prev > 0 >= sdf_cur,
 * linear interpolation.  The DDA refuses views of more than 2^22 voxel steps per ray.
 * vh_raycast_normals (DDA only) also writes, in the same pass, the normal of every hit: the TSDF gradient at
 * the second voxel of the pair (central differences where both neighbours are valid, one-sided otherwise),
 * normalised, in the CAMERA frame with w = 0 (the convention of calculateNormals, CameraTrackingUtils.cu:
 * 75-113); zeros for a miss or when an axis has no valid neighbour.
 * How the DDA is executed does not change a bit of the image; option "raycast_beam" picks the form: 2 = one block
 * list per 8x8-pixel wave, 1 = a walk per ray behind a per-wave beam front end, 0 = a walk per ray from t_min,
 * 3 (default) = by the view: 2 when 64 half-block slabs span [t_min, t_max] (coarse voxels), else 1. */
#define VH_RAYCAST_FIXED_STEP 0
#define VH_RAYCAST_DDA        1
int vh_raycast(vh_context *ctx, const float pose[16], float t_min, float t_max,
               float *d_depth_out);
int vh_raycast_normals(vh_context *ctx, const float pose[16], float t_min, float t_max,
                       float *d_depth_out, vh_float4 *d_normals_out);

/* Block silhouettes: the reference's one working render pass (SDFRenderer::drawToFrontAndBack,
 * SDFRenderer.cpp:165-208: one cube per entry -- block k covers world [8k, 8k+8]*voxelSize,
 * Application.cpp:130-132 -- nearest front face per pixel; notes.md:3-16 adds the back faces).  Per
 * pixel the camera depth at which its ray enters the nearest and leaves the farthest cube of ANY
 * allocated block, clipped to [t_min, t_max], by an exact ray/box test; 0 = no block.  Two W*H float
 * images.  Uses the raycast intrinsics. */
int vh_render_blocks(vh_context *ctx, const float pose[16], float t_min, float t_max, float *d_front,
                     float *d_back);

/* The compact table (d_compactifiedHashTable, VH_BUF_COMPACT) as the reference leaves it -- `occupied` dense
 * entries from index 0 -- is what vh_download, vh_get_device_pointers, vh_flush and vh_synchronize hand over:
 * inside a fused frame the list is kept with two ends (two counters instead of one hot word) and these calls
 * fold it first.  The addresses in a PtrContainer never change during the life of a context (fetch it once, as
 * the reference does, VoxelUtils.cu:141-148): pipelined frames alternate between two compact buffers and two
 * claim arrays internally, and vh_flush / vh_synchronize leave the dense list in the buffer
 * d_compactifiedHashTable names; d_hashTableBucketMutex names the first of the two claim arrays (consecutive lock
 * epochs of pipelined frames stake their claims in the two arrays alternately; every word carries its epoch). */
int vh_synchronize(vh_context *ctx);
int vh_get_counters(vh_context *ctx, vh_counters *out);              /* synchronises */
int vh_get_params(vh_context *ctx, HashTableParams *out);
int vh_get_device_pointers(vh_context *ctx, PtrContainer *out);
int vh_download(vh_context *ctx, int which, void *host_dst, size_t bytes);  /* synchronises */
/* the same for `bytes` bytes starting `offset_bytes` into the buffer (one 4 KiB block of a
 * multi-gigabyte volume: offset = 8 * entry.ptr) */
int vh_download_range(vh_context *ctx, int which, size_t offset_bytes, void *host_dst, size_t bytes);

/* DIAGNOSTICS AND TEST FACILITIES.  They are part of the library a deployment loads -- the tests and the profiles run on the
 * product, not on a build of their own -- and are supported as documented here; none of them changes a result:
 *   vh_debug_eval, vh_debug_set_raycast_stamps, vh_debug_occupy, vh_debug_icp_layout (below); the loop-back transport of voxelhash_dist.h
 *   (vh_dist_loopback_id: the N-rank exchange inside one process); vh_set_profiling / vh_get_kernel_times; the options
 *   "spin_limit"; environment: VOXELHASH_ROCTX=1 (roctx ranges named after the entry points -- vh_integrate, vh_integrate_depth,
 *   vh_flush, vh_raycast, vh_render_blocks, vh_icp_align, vh_garbage_collect, vh_preprocess, vh_dist_step_batch, vh_dist_raycast --
 *   for `rocprofv3 --marker-trace`; libroctx64 is loaded at run time, nothing is linked), VOXELHASH_LOOPBACK_TIMEOUT_S (how long a
 *   loop-back rank waits for its peers), VH_ICP_BLOCKS
 *   (workgroups of an ICP round), VOXELHASH_SEMANTICS (the drop-in names' semantics).
 * Code that exists only in diagnostics BUILDS (make EXTRA=-D...) and in no shipped library: VH_DEBUG_SKIP_ROLES (roles of the
 * pipelined launch return at once), VH_CLAIM_STAMPS, VH_DEBUG_DIST_* (per-phase time stamps and switch-offs). */
/* test hook: evaluates the device scalar helpers on n points; writes 8 int32 per
 * point: block x,y,z, hash, blockInFrustum, project() x,y, float->int of .w */
int vh_debug_eval(vh_context *ctx, const vh_float4 *d_points, int32_t n, int32_t *d_out);
/* diagnostics hook: the DDA raycast records per wave {start, end (100 MHz clock), voxel steps + jumps of lane 0,
 * pixel patch x | y << 16} in d_stamps (4 uint64 per wave, workgroups in launch order); NULL = off */
int vh_debug_set_raycast_stamps(vh_context *ctx, void *d_stamps);
/* test hook: `workgroups` x 256 lanes that stay resident for `microseconds` on `stream` (a device busy with another kernel) */
int vh_debug_occupy(vh_context *ctx, void *stream, int32_t workgroups, int32_t microseconds);
/* test hook: the grids vh_icp_create chose -- out[0] workgroups of an ICP round (VH_ICP_BLOCKS), out[1] workgroups of the
 * one-launch Align, out[2] its input pixels per lane held in registers (1..6; 0: read again every round; -1: Align runs as a
 * chain of one-launch rounds, VH_ICP_PERSISTENT=0 or a grid the chip cannot hold at once) */
struct vh_icp;
int vh_debug_icp_layout(const struct vh_icp *icp, int32_t out[3]);

/* Options (18 names; anything else is rejected with VH_ERR_INVALID_ARGUMENT).  Results never depend on the tuning ones.
 *   semantics of the model (extensions of the reference, each with its oracle counterpart):
 *     "overflow_list" (0 | 1, before the first frame), "band_mode" (VH_BAND_*), "depth_truncation", "weight_sample" (0 | 1)
 *   the frame:
 *     "flatten_variant"  3 = the reference's walk over every VoxelEntry (flattenKernel, VoxelUtils.cu:719-749), 4 = the walk
 *                        over the bucket-occupancy bitmap and the non-empty buckets (same compact SET, the list's order is free
 *                        in the reference too: an atomic race, VoxelUtils.cu:737-746) -- the default: 2-11 x the frames/s of the
 *                        reference's walk at every table size measured
 *     "pipeline"         1: one launch per frame (a frame's commit + TSDF update ride in the next frame's launch)
 *     "pipeline_overflow" 0 | 1 | 2: one-launch frames with the overflow list never / by the launch's size / always
 *     "pipeline_shards"  0 | 1 | 2: the same for a shard's multi-camera frames (vh_apply_frames_batch)
 *     "fused_frame"      1 (default): vh_integrate as two launches; 0: the four step kernels of the step-level entry points
 *     "walk_nt"          non-temporal loads in the reference walk (default: on when the table exceeds the 256 MiB Infinity Cache)
 *     "walk_reverse"     1 (default): the reference walk sweeps the table forward in one launch and backward in the next, each tile on
 *                        the same XCD, so that the tail of a sweep is still in that XCD's L2; 0: always forward (same compact SET)
 *     "claim_lead"       groups of 8 walk workgroups that run ahead of a launch's first claim tile (the head of the sweep is read while
 *                        the L2s still hold it); -1 (default): by the host's rule in the pipelined launch, none in the two-launch
 *                        frame; >= 0: that many in both, clamped to the launch (same table, voxels and compact SET)
 *     "integrate_grid", "commit_blocks"   workgroups of the TSDF update / of the commit phase in the two-launch frame
 *     "gen_frames_per_launch"  1..8 (default 4): frames of a batch one key-generation launch of vh_generate_keys*_batch takes
 *     "spin_limit"       polls a workgroup of a serialised one-launch frame waits for the pending commit phase (0: default)
 *   the raycast:
 *     "raycast_mode" (VH_RAYCAST_DDA | VH_RAYCAST_FIXED_STEP), "raycast_beam" (0 | 1 | 2 | 3 = by the view, default)
 *   formats / test hooks:
 *     "packet_format" (VH_PACKET_F32 / VH_PACKET_U16, below), "cand_capacity" (a smaller candidate list: vh_counters.cand_overflow),
 *     "walk_short" (1, what every table gets: walk tiles of 1024 entries; 0: of 2048, the generic build -- tests/test_gpu_walk_order.py)
 * Variants that were measured and lost (the persistent walk, 8 entries per lane in the frame's walk, the generic build where a
 * lean one exists, the raycast as three launches, 16x4 ray patches, LDS staging of the TSDF update and of the raycast's
 * blocks ...) are not in the library: DESIGN_LOG.md names the commit that last held each. */
int vh_set_option(vh_context *ctx, const char *name, int value);
int vh_set_profiling(vh_context *ctx, int enabled);
int vh_get_kernel_times(vh_context *ctx, vh_kernel_times *out, int reset);  /* synchronises */

/* ---- bucket-range sharding (multi-GPU; DESIGN.md "sharding") ---- */

/* A "multi-camera frame" generalises SDF_Hashtable::integrate to R cameras whose
 * frames enter one logical table together: one lock epoch, all cameras'
 * allocations first (camera order, then launch order, decides who wins a
 * bucket), then flatten + TSDF update camera by camera.  With R = 1 it is the
 * reference's integrate().  The table is cut into bucket ranges, one per GPU. */
#define VH_MAX_CAMERAS 32
#define VH_BIN_PER_BATCH (-1)      /* frame_stride of the batched shard calls: one key bin per shard for the whole batch */
#define VH_PACKET_HEADER_FLOATS 32   /* camera packet: pose[16], inverse[16], then W*H camera-z */

/* Restrict this context to the buckets [lo, hi) of a logical table of
 * params.numBuckets buckets; only those buckets' storage is allocated. */
int vh_create_shard(const vh_config *cfg, uint32_t bucket_lo, uint32_t bucket_hi,
                    vh_context **out);
/* Key generation half of allocBlocks for the pose set with vh_set_pose: per valid
 * pixel the block key of the surface point, frustum-tested, runs of equal keys
 * collapsed per wavefront.  Records are int4 {x,y,z,rank}, rank = camera_id<<27 |
 * launch rank<<6 | band sample, binned by owning shard (owner = hash / ceil(numBuckets/num_shards)):
 * bin s = d_bins[s*bin_stride*4 ...], record 0 = {count,0,0,0}, records 1..count the
 * keys (count > capacity-1 = overflow).  d_packet (nullable) receives the camera
 * packet: pose, inverse pose, camera-z plane (VH_PACKET_HEADER_FLOATS + W*H floats). */
int vh_generate_keys(vh_context *ctx, const vh_float4 *d_verts, uint32_t camera_id,
                     int32_t num_shards, int32_t *d_bins, int32_t capacity, int32_t bin_stride,
                     float *d_packet);
/* Insert the keys of num_bins received bins (same layout) into this shard under the
 * current lock epoch (call vh_reset_mutexes first).  bin_stride / packet_stride: distance
 * between consecutive bins (in records) / packets (in floats); 0 = dense.  Strides let
 * several frames per camera travel in one collective (bins[src][frame], packets[cam][frame]). */
int vh_insert_bins(vh_context *ctx, const int32_t *d_bins, int32_t num_bins, int32_t capacity,
                   int32_t bin_stride);
/* flatten + TSDF update of this shard for num_cams camera packets (contiguous,
 * camera order): one walk over the shard's entries for all cameras, then one
 * pass per visible block applying the cameras that see it in order. */
int vh_integrate_packets(vh_context *ctx, int32_t num_cams, const float *d_packets,
                         size_t packet_stride);
/* Batched forms (one host call, fewest launches) for `batch` frames per camera and exchange.
 * Layouts: bin of shard/source s, frame b at d_bins[(s*bin_stride + b*frame_stride)*4];
 * packet of camera c, frame b at d_packets[c*packet_stride + b*packet_frame_stride].
 * A stride of 0 means dense (frame_stride = capacity, bin_stride = batch*frame_stride,
 * packet_frame_stride = 32 + W*H, packet_stride = batch*packet_frame_stride).
 * vh_generate_keys_batch: poses = batch*16 host floats, d_verts = host array of `batch`
 * device pointers; the packets written are this camera's (d_packets[b*packet_frame_stride]).
 * frame_stride = VH_BIN_PER_BATCH: ONE bin per shard/source for the whole batch (at d_bins[s*bin_stride*4], capacity
 * records for all `batch` frames together, batch <= 32): a record carries its frame index in the rank's camera bits
 * (the camera is the source of the bin), and the launch of frame b claims the records of frame b.  Same tables as
 * per-frame bins; the point is the exchange: a fixed-size bin must hold the worst case of what it may receive, and
 * the worst case of a batch is much closer to its mean than the worst case of a single frame is (vh_dist_* sizes a
 * per-batch bin at 1.5 x batch x W*H/16 / shards records: 3.7 MB of bins per rank and exchange at 8 ranks, batch 8,
 * 640x480, against 19.7 MB with per-frame bins of W*H/16).
 * vh_apply_frames_batch: for b = 0..batch-1: new lock epoch, insert the num_bins bins of
 * frame b, walk + TSDF update for the num_cams packets of frame b; equals vh_reset_mutexes +
 * vh_insert_bins + vh_integrate_packets per frame.  Launches, option "pipeline_shards":
 *   1 (default) one launch per frame ({claim || walk} of frame b with {commit + TSDF update} of frame
 *               b-1) plus one for the batch's last frame: batch + 1;
 *   2           that last half stays pending and rides in the first launch of the NEXT call (batch
 *               launches per call); it is launched by vh_flush and by every call that reads or changes the
 *               model, like a pipelined single-camera frame.  The packets of the batch's LAST frame must
 *               stay valid and unchanged until then (vh_dist_* keeps three buffer sets for this);
 *   0           two launches per frame ({claim || walk}, {commit + integrate}).
 * Tables with bucketSize > 16 and view tables always take two launches per frame; with "overflow_list" the frames of
 * options 1 and 2 are serialised inside their launch (see the pipelined single-camera frame). */
int vh_generate_keys_batch(vh_context *ctx, int32_t batch, const float *poses,
                           const vh_float4 *const *d_verts, uint32_t camera_id, int32_t num_shards,
                           int32_t *d_bins, int32_t capacity, int32_t bin_stride, int32_t frame_stride,
                           float *d_packets, size_t packet_frame_stride);
int vh_apply_frames_batch(vh_context *ctx, int32_t batch, const int32_t *d_bins, int32_t num_bins,
                          int32_t capacity, int32_t bin_stride, int32_t frame_stride, int32_t num_cams,
                          const float *d_packets, size_t packet_stride, size_t packet_frame_stride);
/* Camera packet formats (what vh_integrate_packets / vh_apply_frames_batch read; chosen per context
 * with vh_set_option(ctx, "packet_format", ...)).  Strides stay in 4-byte units.
 *   VH_PACKET_F32: 32 floats {pose, inverse pose} + W*H float camera-z plane (written by
 *                  vh_generate_keys / vh_generate_keys_batch when d_packet(s) is given)
 *   VH_PACKET_U16: 36 floats {pose, inverse pose, K_inv row 2, depth unit 5000} + the W*H uint16
 *                  sensor image (W*H even): half the bytes on the wire; the owner recomputes the
 *                  camera z as preProcess does, (K_inv row 2 . (x,y,1)) * (d / 5000), so the result
 *                  equals the float path on vertex maps made by vh_preprocess from the same image. */
#define VH_PACKET_F32 0
#define VH_PACKET_U16 1
/* Sensor-depth packets of `batch` frames of this camera (poses: batch*16 host floats; d_depth: host
 * array of `batch` device pointers to W*H uint16; packet of frame b at d_packets[b*packet_frame_stride],
 * 0 = dense = 36 + W*H/2).  Keys for the same frames: vh_generate_keys_batch with d_packets = NULL on
 * the vertex maps vh_preprocess made from these images. */
int vh_write_packets_u16_batch(vh_context *ctx, int32_t batch, const float *poses,
                               const uint16_t *const *d_depth, const float k_inv[9], float *d_packets,
                               size_t packet_frame_stride);

/* Keys AND sensor-depth packets of `batch` frames of this camera from the uint16 images alone (one
 * launch per 8 frames: vertices are computed in place, the packet is the header plus the image).
 * Layouts and strides as in vh_generate_keys_batch; d_packets may be NULL (keys only). */
int vh_generate_keys_depth_batch(vh_context *ctx, int32_t batch, const float *poses,
                                 const uint16_t *const *d_depth, const float k_inv[9], uint32_t camera_id,
                                 int32_t num_shards, int32_t *d_bins, int32_t capacity, int32_t bin_stride,
                                 int32_t frame_stride, float *d_packets, size_t packet_frame_stride);

/* ------------------------------------------------------------------ */
/* raycast over shards ("replicate the compact table +   */
/* visible blocks"; DESIGN.md section 6 "raycast")                      */
/* ------------------------------------------------------------------ */
/* A ray samples blocks of every shard, so the rank that renders a view first gathers the
 * blocks the view can touch: each shard exports them as records, the records travel
 * (all-to-all with per-destination counts), the renderer imports them into a private view
 * table and calls vh_raycast on it.  The selection is a conservative superset of the blocks
 * the rays of the view sample, so the result equals vh_raycast on the unsharded table bit
 * for bit. */
typedef struct vh_view_record {
    int32_t  pos[3];
    int32_t  reserved;
    Voxel    voxels[512];
} vh_view_record;                /* 4112 bytes */

/* One walk over this table (shard) for n_views views (poses: n_views*16 host floats,
 * camera->world; the pyramid is that of the raycast intrinsics, t_min..t_max): the allocated
 * entries view v can touch are written to d_records, view 0's records first, then view 1's
 * ... without gaps; d_counts[v] (device) receives the number view v selected.  At most
 * `capacity` records are written per view (a count above capacity reports the loss).
 * d_records must hold n_views*capacity records, 16-byte aligned.  n_views <= VH_MAX_CAMERAS. */
int vh_export_views(vh_context *ctx, const float *poses, int32_t n_views, float t_min, float t_max,
                    vh_view_record *d_records, int32_t capacity, int32_t *d_counts);
/* `view`: an unsharded context of the same numBuckets / bucketSize that never integrated a
 * frame (numVoxelBlocks may be 1).  Its table is emptied and then holds exactly the `count`
 * records; the voxels stay in d_records, which must stay valid and unchanged until the next
 * import.  vh_raycast(view, ...) then renders them.  Records that find their bucket full
 * are dropped and counted in vh_counters.bin_overflow (never happens for records exported
 * from one logical table of the same geometry). */
int vh_import_view(vh_context *view, const vh_view_record *d_records, int32_t count);

/* The same round without any host synchronisation.  vh_export_views_fixed: the view poses are DEVICE
 * memory (n_views*16 floats, e.g. straight out of an all-gather; n_views <= 16) and view v's records go
 * to the fixed slot range [v*capacity, (v+1)*capacity) of d_records, so the exchange has equal sizes known
 * to the host; d_counts[v] = records selected (above capacity: the excess was not written).
 * The count also travels inside the payload: the spare header word (`reserved`) of the first record of a
 * view's slot range holds it.  vh_import_views: `num_sources` slot ranges of `capacity` records each,
 * source s holding min(count_s, capacity) records, count_s = d_counts[s] (device) or, with d_counts =
 * NULL, that header word; what the sources selected beyond the
 * capacity is added to vh_counters.bin_overflow of the view context.  Costs bandwidth instead of
 * latency: the exchange moves num_sources*capacity records whatever the counts are. */
int vh_export_views_fixed(vh_context *ctx, const float *d_poses, int32_t n_views, float t_min, float t_max,
                          vh_view_record *d_records, int32_t capacity, int32_t *d_counts);
int vh_import_views(vh_context *view, const vh_view_record *d_records, int32_t num_sources, int32_t capacity,
                    const int32_t *d_counts);

/* ------------------------------------------------------------------ */
/* block deletion / garbage collection         */
/* ------------------------------------------------------------------ */
/* The reference lists deletion as a feature (README.md:15) but deleteVoxelEntry
 * (VoxelUtils.cu:544-604) is never called and frees the block of the first FREE slot it
 * meets.  Built as the paper does it (Niessner et al. 2013, 4.4), asynchronous on the context's
 * stream, in its own lock epoch:
 *   vh_delete_blocks: for each key {x,y,z,_} (device, n records of 4 int32) present in this
 *     table (shard): the 512 voxels are zeroed, ptr/512 goes back on the heap
 *     (removeSingleBlockInHeap, :336-341), the entry is removed and the later entries of its
 *     bucket move down in order (a bucket's entries stay a prefix of its slots, which
 *     insertVoxelEntry :421-456 and every lookup rely on).  Absent keys, keys of another shard
 *     and repetitions of a key are skipped.
 *     With the option "overflow_list" there is no compaction: a freed slot simply becomes free.
 *     Two exceptions keep the chains whole.  A bucket's last slot heads its chain: when it is
 *     deleted while the chain is not empty it is refilled with its first follower (pos, ptr and
 *     the follower's link to the rest), so "last slot free" always means "no chain".  A chained
 *     entry is unlinked from its predecessor (prev.offset = curr.offset, :594).  The resulting
 *     table does not depend on the order of the keys.
 *   vh_garbage_collect: the same for every entry of the compact list (the blocks the last frame
 *     saw) whose voxels have max weight == 0, or min |sdf| over the voxels with weight > 0
 *     >= sdf_threshold.  The max weight is floored at 0 and a NaN weight is no weight, so a block
 *     none of whose voxels has weight > 0 goes whatever the threshold.  A NaN |sdf| is no sample;
 *     a block with no sample has min = +inf.  A NaN threshold compares false: then only the
 *     blocks without an observed voxel go.
 * Both leave the compact list empty (occupied = 0 until the next frame); vh_counters.last_freed
 * / freed_total report what was freed. */
int vh_delete_blocks(vh_context *ctx, const int32_t *d_keys, int32_t n);
int vh_garbage_collect(vh_context *ctx, float sdf_threshold);

/* ------------------------------------------------------------------ */
/* the model as geometry: triangle mesh of the TSDF's zero level        */
/* ------------------------------------------------------------------ */
/* Marching tetrahedra on the Kuhn split (six tetrahedra around the diagonal of every cell, the same split in every cell:
 * no ambiguous cases, a closed 2-manifold wherever the volume is; DESIGN.md "mesh" has the full rule).  A voxel is valid
 * iff its block is allocated (in this table / shard) and its weight > 0, inside iff sdf <= 0.  A cell -- voxel (x,y,z)
 * and its +1 neighbours, owned by the block of (x,y,z) -- emits triangles iff all eight corners are valid.  A vertex
 * lies on a cell edge, face diagonal or the cell diagonal between voxels A <= B: t = sA / (sA - sB), position
 * (A + t on the axes where B = A + 1) * voxelSize, world frame, in both semantics; the arithmetic depends on the edge
 * alone, so triangles that share an edge share the vertex bit for bit and welding is an exact `unique`.  Triangles are
 * wound so that (v1 - v0) x (v2 - v0) points towards positive sdf (free space).  Zero-area triangles (a vertex on a
 * corner) are not filtered.
 *   region: the cells of the blocks block_lo <= key < block_hi per axis; NULL = the whole model.
 *   d_positions: capacity_triangles * 9 floats (device), three vertices per triangle; may be NULL when the capacity is 0.
 *   d_normals: NULL, or capacity_triangles * 9 floats: per vertex the TSDF gradients at A and B (the rule of
 *     vh_raycast_normals, not normalised) blended as gA + t * (gB - gA), then normalised; world frame; (0,0,0) where an
 *     end has no gradient.
 *   triangles_out (host): the triangles the region holds, also when that exceeds the capacity -- then the first
 *     `capacity_triangles` in output order are written and nothing beyond the buffers is touched (VH_OK).
 *     capacity 0 with NULL buffers is the count-only call.
 * Key domain: |key| < 2^28 on every axis (the voxel coordinate 8 * key + 0..7 must fit an int32; it is computed in wrapping
 * 32-bit arithmetic, so a key outside the domain gives unspecified positions).  Negative keys are fine.  From |8 * key| >= 2^24
 * on, the coordinate is rounded to the nearest float32 (the same bits as the specification, but vertices of a block coincide).
 * Region bounds may be any int32.
 * Output order is reproducible: blocks in ascending entry index of the hash table, cells in ascending voxel index
 * within the block, tetrahedra 0..5, triangles in table order -- the same table gives the same bytes.
 * Runs on the context's stream behind every frame queued so far (a pending pipelined frame is launched first) and
 * synchronises to return the count.  Works on shards (cells that need a block of another shard emit nothing) and on
 * view tables (vh_import_view(s)).  Scratch is allocated at the first call and kept; frames are not affected. */
typedef struct vh_mesh_region { int32_t block_lo[3], block_hi[3]; } vh_mesh_region; /* cells of blocks lo <= k < hi */
int vh_extract_mesh(vh_context *ctx, const vh_mesh_region *region /* NULL: whole model */,
                    uint64_t capacity_triangles,
                    float *d_positions   /* capacity*9 floats, may be NULL when capacity is 0 */,
                    float *d_normals     /* capacity*9 floats or NULL */,
                    uint64_t *triangles_out /* host: triangles the region holds, even if > capacity */);
/* The same with HOST output buffers (device buffers for the duration of the call, one copy back): for callers that have
 * no HIP runtime of their own, like the C++ facade.  Not a hot path. */
int vh_extract_mesh_host(vh_context *ctx, const vh_mesh_region *region, uint64_t capacity_triangles,
                         float *h_positions, float *h_normals, uint64_t *triangles_out);

/* The same surface in INDEXED form: one vertex buffer, three uint32 indices per triangle.  Everything vh_extract_mesh
 * specifies stays (which cells emit, the triangles, their order, the winding, the arithmetic of a position and a normal).
 *   A vertex is identified by its EDGE (A, d): A the global voxel coordinate of the lower end (the end t is measured
 *     from), d = 1..7 the bit set of axes (x = 1, y = 2, z = 4) on which the upper end is A + 1: three axis edges, three
 *     face diagonals and the cell diagonal are anchored at every voxel.  Two edges whose positions have equal bits (t = 0
 *     or 1 at an sdf of +-0, float32 rounding from |8 * key| >= 2^24 on) stay two vertices: sheets that only touch are
 *     not glued, which a weld by position would do.  Welded by edge the mesh is a closed 2-manifold wherever the volume
 *     is: no directed edge (i, j) occurs twice.
 *   Vertex (A, d) exists iff an emitted triangle of the region uses it: both ends valid with different inside flags, and
 *     one of the one, two or four cells that contain the edge (corner 0 at A - o, o a bit set disjoint from d) has eight
 *     valid corners and lies in a block of the region.
 *   Vertex order: ascending (entry index in the hash table of the block that holds voxel A, voxel index of A in that
 *     block, d).  A may lie in a +neighbour of the block that owns the cell, also one outside the region: the blocks
 *     that can hold vertices are the allocated ones with block_lo <= key < block_hi + 1 per axis (saturating).
 *   d_indices: three per triangle, triangles in the order of vh_extract_mesh.  d_vertices[d_indices[i]] has the bits
 *     vh_extract_mesh writes for corner i of the same table and region, and so has d_vertex_normals (one normal per
 *     vertex, the same rule: it depends on the edge alone).
 *   vertices_out, triangles_out (host): what the region holds, also when that exceeds a capacity -- then the first
 *     capacity_vertices vertices and the first capacity_triangles triangles in order are written and nothing beyond the
 *     buffers is touched (VH_OK).  Indices in a clipped index buffer may name vertices at or beyond capacity_vertices.
 *     Both capacities 0 with NULL buffers is the count-only call.
 *   A region with more than 2^32 - 1 vertices cannot be indexed: both counts are reported, nothing is written and the
 *     call returns VH_ERR_INVALID_ARGUMENT (extract by regions instead).
 * Key domain, stream order, the one synchronisation, shards (a cell that needs a block of another shard emits nothing,
 * and so do the vertices only such cells would use) and view tables as for vh_extract_mesh.  Scratch of the indexed call
 * (2 KB and a few words per block the table can hold) is allocated at its first use and kept; a context that never
 * calls it allocates nothing for it. */
int vh_extract_mesh_indexed(vh_context *ctx, const vh_mesh_region *region /* NULL: whole model */,
                            uint64_t capacity_vertices, uint64_t capacity_triangles,
                            float *d_vertices        /* capacity_vertices * 3 floats, may be NULL when that is 0 */,
                            float *d_vertex_normals  /* capacity_vertices * 3 floats or NULL */,
                            uint32_t *d_indices      /* capacity_triangles * 3, may be NULL when that is 0 */,
                            uint64_t *vertices_out, uint64_t *triangles_out /* host; what the region holds */);
/* The same with HOST output buffers, as vh_extract_mesh_host: for the C++ facade.  Not a hot path. */
int vh_extract_mesh_indexed_host(vh_context *ctx, const vh_mesh_region *region, uint64_t capacity_vertices,
                                 uint64_t capacity_triangles, float *h_vertices, float *h_vertex_normals,
                                 uint32_t *h_indices, uint64_t *vertices_out, uint64_t *triangles_out);

/* ------------------------------------------------------------------ */
/* the model as a distance field                                       */
/* ------------------------------------------------------------------ */
/* Signed distance, weight and gradient of the fused TSDF at world points, and dense boxes of the voxel lattice
 * (tests/sample_ref.py is the rule in executable form).  IEEE fp32, unfused multiply and add, in the order
 * written here: the same model gives the same bits.
 *   A voxel with integer coordinate g sits at g * voxelSize in the world frame (the mesh's convention, both semantics); it is
 *   valid iff its block is allocated in this table / shard, its weight > 0 and its sdf is not NaN (the mesh's rule).
 *   A point p has u = p / voxelSize per axis; a point with an axis failing |u| < 2^30 (NaN and +-inf among them) has no sample.
 *   No sample: sdf NaN, weight 0, gradient (NaN, NaN, NaN).
 *   VH_SAMPLE_NEAREST: the voxel (int)(u + copysign(0.5, u)), truncating (world2Voxel's rule); sdf and weight are its own
 *     when it is valid.  Gradient: the rule of the mesh normals at that voxel, per axis (s+ - s-) * 0.5 where both neighbours
 *     are valid, s+ - here or here - s- where one is, each divided by voxelSize; an axis with neither makes the whole
 *     gradient NaN.
 *   VH_SAMPLE_TRILINEAR: f = floor(u), i = (int)f, t = u - f; corner c (bit 0 = x, 1 = y, 2 = z) is voxel i + c.  A sample
 *     iff all eight corners are valid (also for a point exactly on the lattice).  With lerp(a, b, t) = a + t * (b - a):
 *       sdf = lerp(lerp(lerp(s0,s1,tx), lerp(s2,s3,tx), ty), lerp(lerp(s4,s5,tx), lerp(s6,s7,tx), ty), tz),
 *       weight the same on the eight weights,
 *       gx = lerp(lerp(s1-s0, s3-s2, ty), lerp(s5-s4, s7-s6, ty), tz) / voxelSize, gy and gz alike on their axes.
 *     A stored +-inf goes through the arithmetic as IEEE has it.
 * Both device calls only enqueue work on the context's stream, behind every frame queued so far (a pending pipelined frame
 * is launched first); they read nothing back, do not synchronise, allocate nothing and change nothing in the model.  They
 * work on shards (a block of another shard is absent: a sample that needs one is NaN) and on view tables, with or without
 * the overflow list.  n == 0 or a zero entry of dims: VH_OK, nothing is launched.  VH_ERR_INVALID_ARGUMENT: n > 2^31 - 1,
 * an unknown mode, NULL d_points or d_sdf with n > 0, a negative entry of dims, lo + dims beyond int32 on an axis. */
#define VH_SAMPLE_NEAREST   0
#define VH_SAMPLE_TRILINEAR 1
int vh_sample_sdf(vh_context *ctx, int32_t mode, uint64_t n,
                  const float *d_points   /* n*3 floats, world metres, packed xyz: the layout of d_vertices of vh_extract_mesh_indexed */,
                  float *d_sdf            /* n floats; NaN = no valid sample */,
                  float *d_weight         /* n floats or NULL */,
                  float *d_gradient       /* n*3 floats or NULL: d sdf / d world metres */);
/* The same with HOST buffers (device buffers for the duration of the call, one copy each way; synchronises): for the C++
 * facade, as vh_extract_mesh_host.  Not a hot path. */
int vh_sample_sdf_host(vh_context *ctx, int32_t mode, uint64_t n, const float *h_points, float *h_sdf, float *h_weight,
                       float *h_gradient);
/* The voxels lo <= g < lo + dims as dense arrays: element (k * dims[1] + j) * dims[0] + i is voxel lo + (i, j, k); the stored
 * sdf where the voxel is valid, else NaN; the stored weight where valid, else 0. */
int vh_sample_lattice(vh_context *ctx, const int32_t lo[3], const int32_t dims[3],
                      float *d_sdf        /* dims[0]*dims[1]*dims[2] floats, x fastest */,
                      float *d_weight     /* the same size or NULL */);

/* The Euclidean signed distance field (ESDF) on the lattice: for every voxel of a box the exact squared distance, in voxels,
 * to the nearest voxel of the other class, up to a radius (tests/esdf_ref.py is the rule in executable
 * form).  Integers throughout: the same model gives the same bits.
 *   Classes.  A voxel g is valid by the rule above (block allocated in this table / shard, weight > 0, sdf not NaN).  A
 *     valid voxel is INSIDE iff sdf < 0 (-inf is inside, -0.0 and +0.0 are not), every other valid voxel is OUTSIDE, every
 *     other voxel of the infinite lattice is UNKNOWN.  `unknown` remaps the unknown voxels before anything else happens:
 *     VH_ESDF_UNKNOWN_KEEP leaves them unknown, _FREE makes them outside and _OCCUPIED inside, in every respect.
 *   Distance.  With R = radius (1 .. VH_ESDF_MAX_RADIUS) and d2(g, s) = |g - s|^2: P(g) = the minimum of d2(g, s) over the
 *     inside voxels s with d2 <= R^2, N(g) the same over the outside voxels; either may be "none".  The result D(g) is
 *       for an outside voxel  P(g), or VH_ESDF_FAR where there is none;
 *       for an inside voxel  -N(g), or -VH_ESDF_FAR where there is none;
 *       for an unknown voxel (under KEEP only)  VH_ESDF_NONE.
 *     The sites are voxel centres: across a surface the values go ..., 4, 1, -1, -4, ... and never 0.
 *   The sites are those of the whole model, not of the box: D(g) depends on the voxels within R of g only, so two calls
 *     agree wherever their boxes overlap.
 *   d_distance, in metres: sign(D) * (sqrtf((float)|D|) * voxelSize), each operation rounded to fp32 on its own and the
 *     square root correctly rounded; +-inf for +-VH_ESDF_FAR, NaN for VH_ESDF_NONE.
 * The layout of both outputs is vh_sample_lattice's.  The call only enqueues work on the context's stream, behind every
 * frame queued so far (a pending pipelined frame is launched first); it reads nothing back, does not synchronise, allocates
 * nothing (the caller brings the workspace, of at least vh_esdf_workspace_bytes(dims, radius) bytes, 16-byte aligned; nothing
 * beyond that size is written) and changes nothing in the model.  It works on shards (a block of another shard is unknown)
 * and on view tables, with or without the overflow list.  A zero entry of dims: VH_OK, nothing is launched, no workspace
 * is needed (vh_esdf_workspace_bytes reports 0).  VH_ERR_INVALID_ARGUMENT: a radius outside 1 .. VH_ESDF_MAX_RADIUS, an
 * unknown `unknown`, a negative entry of dims, lo - radius or lo + dims + radius beyond int32 on an axis, both outputs
 * NULL, a NULL or not 16-byte aligned workspace, workspace_bytes below what vh_esdf_workspace_bytes reports, more than
 * 2^31 - 1 voxels.
 * Diagnostics: vh_set_option(ctx, "esdf_launches", k) with k = 1..3 makes vh_esdf_lattice stop behind its first k launches,
 * for timing (tools/esdf_time.py): it still returns VH_OK and then writes NO output.  The setting stays on the context until
 * it is set back to 0; vh_esdf_lattice_host ignores it. */
#define VH_ESDF_MAX_RADIUS       255
#define VH_ESDF_UNKNOWN_KEEP     0
#define VH_ESDF_UNKNOWN_FREE     1
#define VH_ESDF_UNKNOWN_OCCUPIED 2
#define VH_ESDF_FAR  INT32_MAX
#define VH_ESDF_NONE INT32_MIN
int vh_esdf_workspace_bytes(const int32_t dims[3], int32_t radius, uint64_t *bytes);
int vh_esdf_lattice(vh_context *ctx, const int32_t lo[3], const int32_t dims[3], int32_t radius, int32_t unknown,
                    void *d_workspace, uint64_t workspace_bytes,
                    int32_t *d_dist2    /* dims[0]*dims[1]*dims[2], x fastest, the layout of vh_sample_lattice; or NULL */,
                    float *d_distance   /* the same size, metres; or NULL (not both NULL) */);
/* The same with HOST outputs and a workspace of its own for the duration of the call (synchronises): for the C++ facade, as
 * vh_sample_sdf_host.  Not a hot path. */
int vh_esdf_lattice_host(vh_context *ctx, const int32_t lo[3], const int32_t dims[3], int32_t radius, int32_t unknown,
                         int32_t *h_dist2, float *h_distance);

/* ------------------------------------------------------------------ */
/* the model met by rays                                               */
/* ------------------------------------------------------------------ */
/* Where does this ray meet the surface: the DDA of vh_raycast with the camera taken out, for any batch of rays (DESIGN.md
 * 4.10; tests/rays_ref.py is the rule in executable form).  IEEE fp32, every multiply and add rounded on its own, in the
 * order written here: the same model and rays give the same bits.
 *   A ray is O + t * D for t_min <= t, crossings taken while t < t_max; D need not be normalised.  Per axis a:
 *     G_a = O_a / voxelSize + 0.5, E_a = D_a / voxelSize; the axis is active iff |E_a| > 1e-20, steps by s_a = +1 iff E_a > 0,
 *     else -1; Gs_a = G_a - 1 for an axis that steps up, G_a otherwise.  The first voxel is floor(G + E * t_min).  The
 *     crossing out of integer coordinate c happens at t_a(c) = ((float)c - Gs_a) * (1 / E_a), never for an inactive axis.  The
 *     walk takes, again and again, the first pending crossing in the order (t, priority y < z < x); a crossing with
 *     t >= t_max is not taken and ends the ray.  With O = a pose's translation and D_a = (T[a,0] * dx + T[a,1] * dy) + T[a,2]
 *     these are the rays of vh_raycast, bit for bit.
 *   Samples: a visited voxel (cx, cy, cz) of an allocated block with weight > 0, at parameter
 *     t(c) = ((w0 * cx + w1 * cy) + w2 * cz) + w3.  With depth_plane = P one plane serves all rays:
 *     w = (P0 * voxelSize, P1 * voxelSize, P2 * voxelSize, P3); row 2 of a pose's inverse makes t the camera depth, and the
 *     results are then the bits of vh_raycast for the same rays.  With depth_plane = NULL the sample sits at the projection
 *     of the voxel centre onto its own ray: dd = (Dx * Dx + Dy * Dy) + Dz * Dz, k = 1 / dd, w_a = (D_a * k) * voxelSize,
 *     w3 = -(((Ox * Dx + Oy * Dy) + Oz * Dz) * k).
 *   Hit: the first pair of consecutive visited voxels that are both samples with sdf_prev > 0 >= sdf_cur;
 *     t = t_prev + ((t_cur - t_prev) * sdf_prev) / (sdf_prev - sdf_cur).
 *   d_t: the hit's t, NaN where there is none.  d_voxels: {x, y, z, 1} of the pair's second voxel for a hit, {0, 0, 0, 0}
 *     for a miss (the status word tells a miss from a hit whose arithmetic gives NaN, stored +-inf for instance).
 *     d_normals: the gradient rule of vh_raycast_normals at that voxel, divided by its length when that is > 0 and every
 *     axis has a neighbour, NOT rotated (world frame, towards positive sdf); zeros otherwise.
 *   A refused ray has status -1, t = NaN, normal zeros and costs no walk.  Refused: a ray with a float that is not finite;
 *     one for which t_max > t_min does not hold; dd == 0; one whose step bound
 *     16 + sum_a (1.01 * (t_max - t_min) * |D_a| / voxelSize + 2) is not < 2^22 (the bound is also the ray's hang-guard
 *     budget); one with |G_a| + (|t_max| + |t_min|) * |D_a| / voxelSize not < 2^23 on some axis.  The last two are the
 *     bounds vh_raycast applies to a view, evaluated per ray on the device in double.
 * The device call only enqueues work on the context's stream, behind every frame queued so far (a pending pipelined frame
 * is launched first); it reads nothing back, does not synchronise, allocates nothing and changes nothing in the model.  It
 * works on shards (a block of another shard is absent) and on view tables, with or without the overflow list.  n == 0:
 * VH_OK, nothing is launched.  VH_ERR_INVALID_ARGUMENT: a null context, n > 2^31 - 1, NULL d_rays or d_t with n > 0, d_rays
 * not 16-byte aligned, an entry of depth_plane that is not finite. */
typedef struct vh_ray { float origin[3]; float t_min; float dir[3]; float t_max; } vh_ray;   /* 32 bytes */
int vh_cast_rays(vh_context *ctx, uint64_t n,
                 const vh_ray *d_rays            /* n rays, device, 16-byte aligned */,
                 const float depth_plane[4]      /* host; NULL: samples are placed along each ray */,
                 float *d_t                      /* n floats: ray parameter of the hit, NaN = none */,
                 float *d_normals                /* n*3 floats or NULL: world-frame normal of the hit, zeros otherwise */,
                 int32_t *d_voxels               /* n*4 int32 or NULL: hit voxel x, y, z and status */);
/* The same with HOST buffers (device buffers for the duration of the call, one copy each way; synchronises): for the C++
 * facade, as vh_sample_sdf_host.  Not a hot path. */
int vh_cast_rays_host(vh_context *ctx, uint64_t n, const vh_ray *h_rays, const float depth_plane[4], float *h_t,
                      float *h_normals, int32_t *h_voxels);

/* ------------------------------------------------------------------ */
/* taking a frame back out                                             */
/* ------------------------------------------------------------------ */
/* De-integration: the TSDF update of a fused frame run backwards, so that a frame whose pose was corrected after the fact can
 * be removed at its OLD pose and fused again at the new one without rebuilding the model (BundleFusion's deIntegrate on this
 * data structure; tests/deintegrate_ref.py is the rule in executable form).  IEEE fp32, every multiply and add
 * rounded on its own, in the order written here: the same model, frame and options give the same bits.
 *   Block set: every allocated entry of this table (or shard) that passes blockInFrustum for `pose` -- exactly the compact
 *     set vh_set_pose(pose) + vh_flatten produce, chained overflow entries included.  No block is allocated or freed.
 *   Sample: for each of a block's 512 voxels the frame's sample (s, cw) is computed exactly as vh_integrate's update does:
 *     the camera point by the context's semantics, project, the image bounds test, depth <= 0 rejects, s = depth - cz,
 *     trunc = truncation (+ truncScale * depth with the option depth_truncation AS IT IS SET NOW), !(s > -trunc) rejects,
 *     s clamped to [-trunc, trunc], cw = 0.1f (or max((float)(integrationWeightSample * 1.5 * (1 - (depth - 0.5f) / 4.5f)), 1)
 *     with the option weight_sample, the product in double).  A voxel the update would have skipped is untouched.
 *   Stored weight: with the stored voxel {os, ow}, a voxel with !(ow > 0) is untouched.
 *   Removal: nw = ow - cw.  floor = half the smallest weight a sample can have: 0.05f, or 0.5f with weight_sample.
 *     !(nw >= floor): the voxel becomes {+0.0f, +0.0f}, the zero-initialised state, which the mesh, the sampler and the raycasts
 *     treat as invalid.  Otherwise sdf = ((os * ow) - (s * cw)) / nw and weight = nw.  (k additions of 0.1f followed by k
 *     subtractions leave a rounding residue, not 0: a residue is far below half a sample, a sample that genuinely remains is
 *     never below a whole one.)
 *   Exactness: this is the algebraic inverse of the update only for voxels whose weight never reached integrationWeightMax
 *     (the cap forgets how much was added), only when the options are those the frame went in with, and even then only up to
 *     fp32 rounding: sdf and weight of the remaining frames come back to within rounding, not to the bit.  Blocks that were
 *     allocated AFTER the original frame and that the old view sees receive a subtraction they never got an addition for, as
 *     in BundleFusion.  One case is exact: a frame integrated into an empty model and then taken out leaves every voxel {0, 0}.
 * vh_deintegrate is the counterpart of vh_integrate's update for a float4 vertex map (it reads .z).  vh_deintegrate_depth is
 * the counterpart of vh_integrate_depth, straight from the uint16 image: the bits of vh_preprocess + vh_deintegrate.
 * vh_reintegrate_depth is exactly vh_deintegrate_depth(old_pose) followed by vh_integrate_depth(new_pose).
 * The calls only enqueue work on the context's stream, behind every frame queued so far (a pending pipelined frame is
 * launched first); they read nothing back and do not synchronise.  The context's pose becomes `pose`; afterwards the compact
 * list and vh_counters.occupied are those of vh_set_pose(pose) + vh_flatten -- the blocks the call touched -- so a
 * vh_garbage_collect directly after the call frees the blocks the removal emptied (the pairing to use).  The lock epoch, the
 * heap and the hash table are unchanged.  Both semantics; with or without the overflow list; on shards (vh_create_shard) every
 * shard is called with the same pose and image and removes from its own blocks.  In vh_kernel_times the launch counts as a
 * TSDF update (integrate_ms), its flatten as flatten_ms.
 * VH_ERR_INVALID_ARGUMENT: a NULL context, pose, image or k_inv; a context that holds an imported view (vh_import_view(s)):
 * its voxels live in the caller's records.  A refused call changes nothing. */
int vh_deintegrate(vh_context *ctx, const float pose[16], const vh_float4 *d_verts);
int vh_deintegrate_depth(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9]);
int vh_reintegrate_depth(vh_context *ctx, const float old_pose[16], const float new_pose[16],
                         const uint16_t *d_depth, const float k_inv[9]);

/* ------------------------------------------------------------------ */
/* tracking against the model itself                                   */
/* ------------------------------------------------------------------ */
/* Point-to-SDF alignment: the camera is tracked against the fused distance field directly, with no raycast and no projective
 * pairing (Bylow et al., RSS 2013; tests/sdf_track_ref.py is the rule in executable form).  IEEE fp32, every
 * multiply and add rounded on its own, in the order written here: the same model, image and pose give the same per-pixel bits.
 *   Point: pixel idx of the W x H input vertex map (camera frame, what vh_preprocess writes) holds p.  p.z == 0: no point
 *     (vh_icp_*'s rule).  Otherwise q_r = ((T[r][0] * p.x + T[r][1] * p.y) + T[r][2] * p.z) + T[r][3] for r = 0..2, with T the
 *     fp32 copy of the camera -> world pose.
 *   Sample: (s, g) = the VH_SAMPLE_TRILINEAR sdf and gradient of vh_sample_sdf at q ("the model as a distance field" above):
 *     all eight corners of q's cell valid, on shards and view tables, with or without the overflow list.
 *   Kept: the pixel has a point, the point a sample, |s| < dist_thres, and g.x, g.y, g.z are all finite.
 *   System: over the kept pixels, with J = [g, q x g] (6 floats) and residual s: JTJ = sum J J^T (the 21 products of the upper
 *     triangle, mirrored), JTr = sum J s, error = sum s, count.  The products are fp32; they are added in fp32 in a fixed
 *     order (per lane, per workgroup, then over the workgroups of vh_icp's grid): reproducible run to run, and equal to the
 *     exact sums to fp32 summation error only.
 *   Step: T <- exp(-(JTJ^-1 JTr)) T, in double, a left perturbation of the camera -> world pose by the twist (v, w) of
 *     vh_se3_exp; the next round uses (float)T.  vh_sdf_align runs max_iters such rounds from `pose` (typically the pose of
 *     the frame before) and stops early when the summed residual is exactly 0 or JTJ is not positive definite; `pose` is
 *     used as given, it does not go through log / exp first.  *iterations = the rounds that took a step, *last = the system
 *     of the last round built.  A model in which no pixel is kept gives count 0 and JTJ = 0: the pose comes back as given
 *     and *iterations = 0.
 *   Maps (vh_sdf_residuals), per pixel: d_points = q, or (0, 0, 0) where the pixel has no point; d_sdf = s where the pixel
 *     is kept, else NaN; d_gradient = g where the pixel is kept, else (0, 0, 0).
 * `icp` is the workspace (its partial sums, state, grid and image size W x H, which need not be the context's): it must be
 * bound to the context's stream (vh_icp_set_stream) and live on its device.  The calls enqueue on that stream behind every
 * frame queued so far (a pending pipelined frame is launched first), change nothing in the model, and synchronise once, for
 * the read-back that returns the system or the pose.  vh_fusion_step_sdf is one tracked frame: vh_preprocess ->
 * vh_sdf_align(start = pose) -> vh_integrate_depth((float)pose); it needs the workspace to have the context's image size.
 * WHAT IT IS FOR: models fused with a truncation of a few voxels.  Far from a surface a TSDF with a wide truncation is an
 * average over unrelated surfaces, and the tracker follows that average.  Measured with the numpy rule on the CPU (float64
 * sums; synthetic room, 320 x 240, 12 frames over 14 cm of travel, 2 cm voxels, frame 0 given, the others tracked): worst
 * translation error 9.2 mm with truncation = 0.06, dist_thres = 0.08, 10 rounds; with the reference's default truncation =
 * 1.0, 49 mm at dist_thres = 0.08 and 15 mm at dist_thres = 0.03 (20 rounds).  Not GPU results.
 * VH_ERR_INVALID_ARGUMENT, and nothing is changed or launched: a NULL argument (last and iterations may be NULL); an entry
 * of pose or dist_thres that is not finite, or dist_thres <= 0; max_iters outside 0..65536; a workspace of another device or
 * stream; for vh_fusion_step_sdf a workspace of another image size. */
struct vh_icp;
struct vh_icp_system;
int vh_sdf_build_system(vh_context *ctx, struct vh_icp *icp, const vh_float4 *d_input, const float pose[16],
                        float dist_thres, struct vh_icp_system *out);                       /* synchronises */
int vh_sdf_residuals(vh_context *ctx, struct vh_icp *icp, const vh_float4 *d_input, const float pose[16], float dist_thres,
                     float *d_points /* W*H*3 */, float *d_sdf /* W*H */, float *d_gradient /* W*H*3 */,
                     struct vh_icp_system *out);                                            /* the same + the maps */
int vh_sdf_align(vh_context *ctx, struct vh_icp *icp, const vh_float4 *d_input, float dist_thres, int32_t max_iters,
                 double pose[16] /* in: start (e.g. the previous frame's pose); out: result */,
                 struct vh_icp_system *last, int32_t *iterations);
int vh_fusion_step_sdf(vh_context *ctx, struct vh_icp *icp, const uint16_t *d_depth, const float k_inv[9], float dist_thres,
                       int32_t max_iters, vh_float4 *d_input_vertices, vh_float4 *d_input_normals, double pose[16],
                       struct vh_icp_system *last, int32_t *iterations);

/* ------------------------------------------------------------------ */
/* tracking against the model's colour and shape                       */
/* ------------------------------------------------------------------ */
/* vh_sdf_align with a photometric row beside the geometric one: where the model holds colour ("the model in colour" below),
 * the luminance it has at the moved point is compared with the luminance of the input pixel (Kerl et al., IROS 2013, against
 * the fused colour volume instead of a key frame; tests/sdf_color_track_ref.py is the rule in executable
 * form).  A flat wall, a floor or a table top leaves the geometric system singular in the plane; the texture on it does not.
 * IEEE fp32, every multiply, add and divide rounded on its own, in the order written here.
 *   Point, sample, geometric kept, geometric row: vh_sdf_align's -- q, (s, g), |s| < dist_thres and g finite, J = [g, q x g]
 *     with residual s.
 *   Luminance of a colour word w = r | g << 8 | b << 16 | ...: Y(w) = (float)(77 * r + 150 * g + 29 * b) / 65280.0f (the sum
 *     is an integer; Y lies in 0..1).
 *   Input intensity: I = Y(d_rgba[idx]), d_rgba the W x H colour image registered to the depth image (vh_integrate_color's
 *     layout, one word per pixel; its top byte is ignored).
 *   Model intensity at q: there is one iff vh_sample_color's VH_SAMPLE_TRILINEAR rule has a sample at q -- eight valid corners,
 *     all eight words with a count > 0, a colour volume present.  C = the lerp nest of vh_sample_sdf (x innermost, then y,
 *     then z) over the eight Y values; gC = the gradient vh_sample_sdf forms from corner differences, over those eight values,
 *     divided by voxelSize.
 *   Photometric residual e = C - I.  Photometric kept: the pixel is geometrically kept, q has a model intensity,
 *     |e| < color_thres, and color_weight != 0.
 *   Photometric row: h_a = color_weight * gC_a, J = [h, q x h], residual color_weight * e.
 *   System: the sums of "tracking against the model itself" over all rows, geometric and photometric; count = the number of
 *     rows, error = the sum of the rows' residuals.  Step, stop conditions, *iterations and *last as vh_sdf_align.
 *   Maps (vh_sdf_color_residuals): d_points, d_sdf, d_gradient as vh_sdf_residuals; d_color_residual = e where the pixel has
 *     a photometric row, else NaN; d_color_gradient = gC where it has one, else (0, 0, 0).
 * Consequences: with color_weight == 0, on a context without a colour volume, or on a context that holds an imported view,
 * every call returns the bits of the vh_sdf_* call -- pose, system, maps (d_color_residual all NaN, d_color_gradient all 0).
 * On a shard the blocks of other shards are absent, as for vh_sample_color: a cell that reaches into one has no sample.
 * color_weight: 0.1 is the value of the numpy prototype and of the literature (intensity in 0..1 against metres); it has not
 * been tuned on this model.
 * Stream, workspace, the one synchronising read-back and a pending pipelined frame: as vh_sdf_*.  vh_fusion_step_sdf_color is
 * one tracked colour frame: vh_preprocess -> vh_sdf_color_align(start = pose) -> vh_integrate_depth_color((float)pose, ...,
 * band, weight_max).
 * VH_ERR_INVALID_ARGUMENT, and nothing is changed or launched: what vh_sdf_* refuses; a NULL d_rgba; a color_weight that is
 * not finite or below 0; a color_thres that is not finite or not above 0; for vh_fusion_step_sdf_color what
 * vh_integrate_depth_color refuses (band, weight_max, a view table). */
int vh_sdf_color_build_system(vh_context *ctx, struct vh_icp *icp, const vh_float4 *d_input, const uint32_t *d_rgba,
                              const float pose[16], float dist_thres, float color_weight, float color_thres,
                              struct vh_icp_system *out);                                   /* synchronises */
int vh_sdf_color_residuals(vh_context *ctx, struct vh_icp *icp, const vh_float4 *d_input, const uint32_t *d_rgba,
                           const float pose[16], float dist_thres, float color_weight, float color_thres,
                           float *d_points /* W*H*3 */, float *d_sdf /* W*H */, float *d_gradient /* W*H*3 */,
                           float *d_color_residual /* W*H */, float *d_color_gradient /* W*H*3 */,
                           struct vh_icp_system *out);                                      /* the same + the maps */
int vh_sdf_color_align(vh_context *ctx, struct vh_icp *icp, const vh_float4 *d_input, const uint32_t *d_rgba, float dist_thres,
                       float color_weight, float color_thres, int32_t max_iters,
                       double pose[16] /* in: start; out: result */, struct vh_icp_system *last, int32_t *iterations);
int vh_fusion_step_sdf_color(vh_context *ctx, struct vh_icp *icp, const uint16_t *d_depth, const float k_inv[9],
                             const uint32_t *d_rgba, float dist_thres, float color_weight, float color_thres, int32_t max_iters,
                             float band, int32_t weight_max, vh_float4 *d_input_vertices, vh_float4 *d_input_normals,
                             double pose[16], struct vh_icp_system *last, int32_t *iterations);

/* ------------------------------------------------------------------ */
/* one model into another                                              */
/* ------------------------------------------------------------------ */
/* Merging: the TSDF held by src is fused into dst under the rigid transform src_to_dst -- submaps whose relative pose a loop
 * closure has corrected, a second session joined to a first, a model re-anchored in another frame or re-gridded to another voxel
 * size, a bucket-range shard pulled into one table (tests/merge_ref.py is the rule in executable form; the
 * reference has none).  IEEE fp32, every multiply and add rounded on its own, in the order written here: the same two models
 * and transform give the same voxel bits.
 *   T = src_to_dst as fp32, row-major: src world metres -> dst world metres; the caller guarantees it is rigid.  Tinv = the
 *   library's cofactor inverse of T (the routine of vh_set_pose).  vs_s, vs_d: the two voxel sizes, which may differ.  trunc,
 *   wmax: DST's truncation and integrationWeightMax.
 *   1. Candidates.  For every allocated entry of src with key k (chained overflow entries included) the eight corners e of the
 *     box [8k - 0.5, 8k + 8] per axis in src voxel units -- a low corner is (float)(8k) - 0.5f, a high one (float)(8k + 8) -- are
 *     transformed: x = e * vs_s, q_r = ((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3], u_r = q_r / vs_d.  Per axis lo / hi
 *     = the minimum / maximum over the corners, gmin = (int)ceilf(lo), gmax = (int)ceilf(hi) - 1; the entry's candidates are all
 *     block keys gmin >> 3 .. gmax >> 3 per axis.  A block with any u failing |u| < 2^30 (NaN included) is skipped
 *     (skipped_blocks) and contributes nothing.  The box holds every point whose trilinear cell or nearest voxel lies in block
 *     k, so the candidates are a superset of the dst blocks that can receive a sample (up to rounding at the rim, where this
 *     rule is the rule): with T = I and equal voxel sizes the candidate of k is k (and, for voxel sizes that are not powers of
 *     two, now and then k + 1, which stays empty); under a rotation about 3.3 x the source's blocks, a third to a half of
 *     which stay empty.
 *   2. Allocation.  The candidate keys are inserted into dst through the claim + commit path of vh_insert_bins, one lock epoch
 *     (vh_reset_mutexes) per round, until no candidate is missing or a round allocates nothing (buckets full, heap empty);
 *     with the overflow list, too.  Which slot and heap block a key gets is free, as for frames.  dst may be a shard: keys of
 *     other bucket ranges are not its business and are not counted as unplaced.  The call holds at most 2^24 candidate records
 *     (duplicates counted; 256 MiB of scratch, allocated by the first call into a context and kept): more is refused with
 *     VH_ERR_OUT_OF_MEMORY before dst changes.
 *   3. Update, over the distinct candidate blocks present in dst, each once.  For dst voxel g: p_a = (float)g_a * vs_d,
 *     q = Tinv . p (rows summed as above), (s, w) = the `mode` sample of SRC at q by the rule of vh_sample_sdf ("the model as a
 *     distance field" above: u = q / vs_s, domain, validity, nearest or trilinear sdf and weight; blocks of another shard are
 *     absent; view tables and the overflow list as there).  No sample (s is NaN) or !(w > 0): the voxel is untouched.
 *     Otherwise s = s >= 0 ? fminf(trunc, s) : fmaxf(-trunc, s) and, with the stored voxel {os, ow}:
 *       !(ow > 0): the voxel becomes {s, fminf(wmax, w)} -- a voxel that holds nothing contributes nothing, so a nearest-voxel
 *         identity merge into an empty model is an exact copy;
 *       otherwise sdf = ((os * ow) + (s * w)) / (ow + w), weight = fminf(wmax, ow + w).
 *   4. Afterwards dst's compact list and vh_counters.occupied are the blocks the update ran over, so vh_garbage_collect(dst, ..)
 *     directly after the call frees the candidate blocks that stayed empty (the pairing to use).  allocated_total and
 *     heap_exhausted move as the commit path moves them; the epoch advances by `rounds`; dst's pose is unchanged; src is only
 *     read.  A src without candidates (empty, or wholly outside the domain): VH_OK, nothing changes.
 * Ordering: a pending pipelined frame of either context is launched first; the call orders itself behind src's stream with an
 * event (recorded there, awaited on dst's stream), its kernels run on dst's stream, and it synchronises dst's stream (round
 * counters, stats).  In vh_kernel_times the key generation and the bin claim count as alloc_claim_ms, the commit and the
 * missing-key count as alloc_commit_ms, the list as flatten_ms, the update as integrate_ms.
 * VH_ERR_INVALID_ARGUMENT, and nothing is changed or launched: a NULL context or matrix; src == dst; contexts on different
 * devices; dst holding an imported view; an unknown mode; an entry of T or of its inverse that is not finite. */
typedef struct vh_merge_stats {
    uint32_t source_blocks;   /* allocated entries of src that were walked */
    uint32_t skipped_blocks;  /* of those, outside the domain: they contribute nothing */
    uint64_t candidates;      /* candidate records generated, duplicates counted */
    uint32_t allocated;       /* blocks this call allocated in dst */
    uint32_t blocks;          /* distinct blocks of dst that received the update (= occupied afterwards) */
    uint64_t unplaced;        /* candidate records (duplicates counted) whose key is not in dst after the last round */
    uint32_t rounds;          /* lock epochs the allocation used */
} vh_merge_stats;
int vh_merge(vh_context *dst, vh_context *src, const float src_to_dst[16], int32_t mode /* VH_SAMPLE_NEAREST | VH_SAMPLE_TRILINEAR */,
             vh_merge_stats *stats /* host, may be NULL */);

/* ------------------------------------------------------------------ */
/* the model in colour                                                 */
/* ------------------------------------------------------------------ */
/* The registered colour image of an RGB-D frame fused into the voxels near the surface, and read back at points, at mesh
 * vertices or per pixel of a raycast (tests/color_ref.py is the rule in executable form; the reference has
 * none).  Voxel stays {sdf, weight}: colour lives in a second volume of one uint32 per voxel, numVoxelBlocks * 512 words, the
 * voxel at volume index ptr + i having its word at ptr + i.  IEEE fp32, every operation rounded on its own, in the order
 * written here: the same model and images give the same words.
 *   Word: r | g << 8 | b << 16 | w << 24, w = the colour sample count, 1..255.  The word 0 means "no colour".
 *   The volume is allocated, zeroed, by the first colour-fusing call into a context and kept: half the bytes of the SDF volume.
 *   A failed allocation returns VH_ERR_OUT_OF_MEMORY and nothing changes.  A context that never fuses colour allocates nothing
 *   and behaves exactly as before.
 * FUSING.  d_rgba is W*H pixels registered to the depth image, one little-endian word per pixel: byte 0 red, byte 1 green,
 * byte 2 blue, byte 3 ignored.
 *   Block set: every allocated entry of this table (or shard) that passes blockInFrustum for `pose` -- the compact set of
 *     vh_set_pose(pose) + vh_flatten, as for vh_deintegrate, chained overflow entries included.  No block is allocated or freed.
 *   Per voxel of a listed block, with the stored voxel {os, ow} and its colour word c:
 *     1. !(ow > 0): the word becomes 0 and nothing else happens to this voxel -- a voxel that holds nothing has no colour,
 *        which also sweeps out the colour a de-integration orphaned.
 *     2. The camera point by the context's semantics, project, the image bounds test, the depth read, depth <= 0 rejects:
 *        all exactly as in vh_integrate's update.  s = depth - cz; no truncation is involved.
 *     3. !(fabsf(s) <= band) rejects: colour belongs to the surface (the reference's default truncation of 1 m would paint
 *        a metre of free space).
 *     4. A rejected voxel is untouched.
 *     5. weight_max == 0: no sample is added; the call is the sweep of step 1 only.
 *     6. Otherwise, with (R, G, B) the pixel at (sx, sy) and w = c >> 24, per channel
 *          f = ((float)old * (float)w + (float)in) / (float)(w + 1),  new = (uint32_t)(f + 0.5f), truncating.
 *     7. w' = min(w + 1, weight_max): at the cap the average keeps moving, with window weight_max.
 *   vh_integrate_color reads the uint16 sensor image with vh_integrate_depth's arithmetic, vh_integrate_color_map the .z of a
 *   float4 vertex map.  vh_integrate_depth_color is exactly vh_integrate_depth followed by vh_integrate_color.
 *   Afterwards the context's pose is `pose`, the compact list and vh_counters.occupied are the flatten's; the lock epoch, the
 *   heap, the hash table and the SDF volume are unchanged.  A pending pipelined frame is launched first.  The calls only
 *   enqueue: they read nothing back and do not synchronise.  In vh_kernel_times the launch counts as integrate_ms, its flatten
 *   as flatten_ms.  Both semantics; with or without the overflow list; on shards every shard is called with the same arguments
 *   and colours its own blocks.
 *   VH_ERR_INVALID_ARGUMENT, with nothing changed: a NULL argument; band not finite or <= 0; weight_max outside 0..255; a
 *   context that holds an imported view.
 * KEEPING IT CONSISTENT.  vh_delete_blocks and vh_garbage_collect zero the colour words of the blocks they free (blocks are
 * handed out zeroed).  vh_load_snapshot clears the colour volume: ptrs are re-dealt and snapshots do not carry colour (the
 * file format is unchanged); vh_save_color / vh_load_color keep the words in a file beside the snapshot.  vh_deintegrate*,
 * vh_merge, view records and the text dump neither carry nor remove colour; the pairing after a plain de-integration is
 * vh_integrate_color(old_pose, ..., weight_max = 0), which sweeps the emptied voxels.  The calls that do carry colour through
 * those steps are vh_merge_color, vh_deintegrate_color / vh_deintegrate_depth_color / vh_reintegrate_depth_color and
 * vh_save_color / vh_load_color: "colour through merging, de-integration and saved models" below.
 * vh_has_color: 0 or 1.  vh_clear_color zeroes the volume if there is one (enqueues only).  vh_download_color synchronises;
 * VH_ERR_INVALID_ARGUMENT when there is no volume or the range is beyond it.
 * READING.  Output word: r | g << 8 | b << 16 | 0xFF << 24; 0 = no colour (real black is 0xFF000000).  The domain,
 * u = p / voxelSize, which voxel or cell, and voxel validity are those of vh_sample_sdf ("the model as a distance field").
 *   VH_SAMPLE_NEAREST: the nearest voxel's colour, if that voxel is valid and its word has w > 0.
 *   VH_SAMPLE_TRILINEAR: a sample iff the sdf rule has one (eight valid corners) and all eight words have w > 0; per channel
 *     the lerp nest of vh_sample_sdf's sdf on the eight (float) channel values, out = (uint32_t)(f + 0.5f).
 *   No volume yet (or a context that holds an imported view, whose records carry no colour): every output is 0, VH_OK.
 *   vh_sample_color_map: points in the camera frame; a point with .z == 0 has no colour, otherwise
 *     q_r = ((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3] (vh_sdf_align's formula) and the rule above at q.
 *   vh_raycast_color is exactly vh_raycast_maps followed by vh_sample_color_map over its vertex map.
 *   The device calls only enqueue, behind every queued frame; they allocate nothing and change nothing; on shards the blocks
 *   of other shards are absent.  Argument checks are vh_sample_sdf's (plus a NULL pose); vh_sample_color_host takes host
 *   buffers and synchronises, as vh_sample_sdf_host. */
int vh_integrate_color(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                       const uint32_t *d_rgba, float band, int32_t weight_max);
int vh_integrate_color_map(vh_context *ctx, const float pose[16], const vh_float4 *d_verts, const uint32_t *d_rgba,
                           float band, int32_t weight_max);
int vh_integrate_depth_color(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                             const uint32_t *d_rgba, float band, int32_t weight_max);
int vh_has_color(vh_context *ctx);
int vh_clear_color(vh_context *ctx);
int vh_download_color(vh_context *ctx, size_t first_voxel, uint32_t *host_dst, size_t count);   /* synchronises */
int vh_sample_color(vh_context *ctx, int32_t mode, uint64_t n, const float *d_points /* n*3, world metres */,
                    uint32_t *d_rgba_out /* n words */);
int vh_sample_color_host(vh_context *ctx, int32_t mode, uint64_t n, const float *h_points, uint32_t *h_rgba_out);
int vh_sample_color_map(vh_context *ctx, int32_t mode, const float pose[16], uint64_t n,
                        const vh_float4 *d_points /* camera frame */, uint32_t *d_rgba_out);
int vh_raycast_color(vh_context *ctx, const float pose[16], float t_min, float t_max, float *d_depth_out,
                     vh_float4 *d_vertices_out, vh_float4 *d_normals_out, int32_t mode, uint32_t *d_rgba_out);

/* ------------------------------------------------------------------ */
/* colour through merging, de-integration and saved models             */
/* ------------------------------------------------------------------ */
/* The calls above composed with colour (tests/merge_color_ref.py is the rule in executable form).  Every call
 * above keeps its behaviour.  IEEE fp32, every operation rounded on its own, in the order written; words as in "the model in
 * colour".
 * MERGING.  vh_merge_color is vh_merge -- its candidates, allocation, ordering, stats, refusals and what it leaves afterwards,
 * and for every dst voxel its TSDF update with the same bits -- with a colour step in the same update launch, at the same point
 * u = (Tinv . g * vs_d) / vs_s, through the source blocks the TSDF sample resolved (the table is not walked a second time).
 *   Colour sample of src, (rgb_s, w_s):
 *     VH_SAMPLE_NEAREST: the nearest voxel's word, if its count w_s = word >> 24 is > 0.
 *     VH_SAMPLE_TRILINEAR: a sample iff all eight corner words have a count > 0 (the corners are valid: the TSDF sample
 *       exists); per channel vh_sample_color's lerp nest and (uint32_t)(f + 0.5f); w_s = the minimum of the eight counts.
 *   Colour step, only where the TSDF step happened (the sample is not NaN and w > 0) and a colour sample exists.  With dst's
 *   word c and w_d = c >> 24:
 *     w_d == 0: the word becomes rgb_s | min(w_s, weight_max) << 24;
 *     otherwise per channel f = ((float)old * (float)w_d + (float)in * (float)w_s) / (float)(w_d + w_s),
 *       new = (uint32_t)(f + 0.5f), and the count becomes min(w_d + w_s, weight_max).
 *   So a nearest-voxel identity merge into an empty model with weight_max = 255 copies every colour word of a valid voxel
 *   exactly, as it copies the TSDF.
 *   A src without a colour volume, or a view table as src: the call is exactly vh_merge and allocates nothing in dst.  A src
 *   with a volume and a dst without: dst's is allocated and zeroed before anything else changes (VH_ERR_OUT_OF_MEMORY, nothing
 *   changed, when that fails).  src's two volumes are only read.  Refusals: vh_merge's, and weight_max outside 1..255.
 * TAKING A FRAME'S COLOUR BACK OUT.  vh_deintegrate_color is one launch in vh_integrate_color's shape behind the step-level
 * flatten for `pose`: block set and steps 1 to 4 of FUSING exactly (the !(ow > 0) sweep included).  For a voxel that passes,
 * with w = c >> 24:
 *     w == 0: untouched.  w == 1: the word becomes 0.
 *     otherwise per channel f = ((float)old * (float)w - (float)in) / (float)(w - 1), f = fminf(fmaxf(f, 0.0f), 255.0f),
 *       new = (uint32_t)(f + 0.5f); the count becomes w - 1.
 *   Exactness is as for the TSDF: the inverse holds only below the colour cap (a word at weight_max has forgotten how many
 *   samples it averaged) and only up to byte rounding.  Removing the frame that was added last brings each channel back to
 *   within 1 of its value before that frame: the add rounds by at most 0.5, and the inverse scales that by w / (w - 1) <= 2
 *   before it rounds to the nearest byte.  Removing an older frame, or several, lets these errors add up.
 *   vh_deintegrate_depth_color is exactly vh_deintegrate_color(pose, ..) -- first, because it reads the TSDF weights and the
 *   band as the frame left them -- then vh_deintegrate_depth(pose, ..), then vh_integrate_color(pose, .., weight_max = 0), the
 *   sweep of what emptied.  vh_reintegrate_depth_color is exactly vh_deintegrate_depth_color(old_pose, ..) followed by
 *   vh_integrate_depth_color(new_pose, .., weight_max).
 *   Enqueue only; shards, both semantics, the overflow list and vh_kernel_times as for vh_integrate_color.
 *   VH_ERR_INVALID_ARGUMENT, with nothing changed: a NULL argument; band not finite or <= 0; (vh_reintegrate_depth_color)
 *   weight_max outside 0..255; a context that holds an imported view; a context without a colour volume (nothing to remove).
 * SAVED MODELS.  vh_save_color writes the colour words to a file of its own: a header (magic, numEntries, numVoxelBlocks, the
 * allocated count), then per allocated entry in table order its pos[3] and its 512 words.  Written to path + ".partial" and
 * renamed, as the snapshot is; a context without a volume: VH_ERR_INVALID_ARGUMENT.  vh_load_color validates everything on
 * the host before a device byte changes -- the header against the context, the file size, and the file's sequence of pos
 * against the context's currently allocated entries in table order -- and a mismatch leaves the model and its colour
 * untouched.  Then it allocates the volume if needed, clears it, and writes each record at the entry's current ptr.  The
 * pairing is vh_save_snapshot + vh_save_color, and vh_load_snapshot followed by vh_load_color.  Both calls synchronise. */
int vh_merge_color(vh_context *dst, vh_context *src, const float src_to_dst[16], int32_t mode, int32_t weight_max /* 1..255 */,
                   vh_merge_stats *stats /* host, may be NULL */);
int vh_deintegrate_color(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                         const uint32_t *d_rgba, float band);
int vh_deintegrate_depth_color(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                               const uint32_t *d_rgba, float band);
int vh_reintegrate_depth_color(vh_context *ctx, const float old_pose[16], const float new_pose[16], const uint16_t *d_depth,
                               const float k_inv[9], const uint32_t *d_rgba, float band, int32_t weight_max);
int vh_save_color(vh_context *ctx, const char *path);
int vh_load_color(vh_context *ctx, const char *path);

/* ------------------------------------------------------------------ */
/* block streaming: a model larger than the block pool                 */
/* ------------------------------------------------------------------ */
/* Niessner et al. 2013, section 5: blocks that leave an active region around the camera move to the host and their pool slots
 * are freed; they move back when the camera returns.  Two exact, lossless calls: vh_stream_out takes the blocks of a region out
 * of the model as records, vh_stream_in puts records back.  The policy on top (which region, where the records are kept) is the
 * caller's; voxelhashing_demo_amd/streaming.py has one.  No counterpart in the reference.
 *
 * The region.  VH_STREAM_BOX: the blocks with block_lo <= key < block_hi on every axis (bounds may be any int32).
 * VH_STREAM_SPHERE: the blocks whose centre lies within `radius` of `centre` (world metres), float32, every operation rounded on
 * its own, in exactly this order:
 *     x_a = ((float)(8 * key_a) + 3.5f) * voxelSize - centre_a     for a = 0, 1, 2
 *     d2  = (x_0 * x_0 + x_1 * x_1) + x_2 * x_2
 *     inside iff d2 <= radius * radius
 * invert = 1 selects the complement: everything OUTSIDE the box or sphere (what leaves an active region).  Key domain: that of the
 * mesh, |key| < 2^28 on every axis.  radius must be finite and >= 0 and centre finite, kind one of the two: otherwise
 * VH_ERR_INVALID_ARGUMENT and nothing changes.  A box does not use centre and radius (they are still checked: zeros will do), a
 * sphere does not use block_lo and block_hi.
 *
 * vh_stream_out runs on the context's stream behind every frame queued so far (a pending pipelined frame is launched first) and
 * synchronises to return its two counts (host): *selected_out = the allocated blocks the region holds, *written_out =
 * min(selected, capacity).  The first `written` of them in ascending entry index of the hash table (the order of the mesh's block
 * list) are written to d_records (capacity records, 16-byte aligned): {pos, reserved = 0, voxels[512]}, exactly the bytes the
 * block held.  With d_colors (capacity * 512 words) record i's 512 colour words go to d_colors[512 * i ...], zeros if the context
 * has no colour volume; with d_colors == NULL THE COLOUR OF THE REMOVED BLOCKS IS DROPPED.  Exactly the written blocks are then
 * removed as vh_delete_blocks removes them: a lock epoch of its own, voxels and colour words zeroed, the blocks back on the heap,
 * the compact list left empty, vh_counters.last_freed / freed_total updated -- the table is what vh_delete_blocks on those keys
 * leaves, slot for slot.  Blocks selected beyond the capacity stay in the model: call again.  capacity == 0 (buffers may be NULL)
 * is the count-only call; it, and a call that selects nothing, change nothing.
 *
 * vh_stream_in puts n records (n <= 2^24; d_colors: n * 512 words or NULL = the blocks get no colour) into the model and reports
 * per record (d_status: n int32 on the device, or NULL) and in total (stats, host, may be NULL):
 *     VH_STREAM_FOREIGN   the key hashes outside this shard's bucket range
 *     VH_STREAM_PRESENT   the model already holds the key -- its block is NOT touched (fusing a record into a block that exists
 *                         is vh_import_view + vh_merge) -- or the key occurs more than once in the call and another record won
 *     VH_STREAM_PLACED    a block was allocated and holds the record's 512 voxels (and colour words), whole
 *     VH_STREAM_UNPLACED  bucket full or pool empty: nothing written for this record
 * Exactly one of the records of equal keys is placed; which one is unspecified.  No record is half-written or silently lost:
 * placed + present + unplaced + foreign == n.  With d_colors the colour volume is created first.  The keys that are neither
 * foreign nor present go through the insertion path of vh_insert_bins as one key bin, one lock epoch per round, until none is
 * missing or a round allocates nothing (stats->rounds; the call synchronises between rounds).  The compact list is left empty.
 * Which record is UNPLACED when room runs out is as free as the slot a key gets: with "overflow_list" a key whose home bucket is
 * full takes a free slot behind it, so in a crowded table whether the last keys of a call (here and in vh_merge's allocation)
 * still find one can depend on which keys the rounds served first.  Keys that each have a free slot in their own home bucket,
 * the other keys of the call counted, are all placed whatever the order.
 *
 * Both calls work on shards and with "overflow_list"; view tables are refused (they own no blocks).  The _host forms take host
 * buffers, stage through device scratch the context keeps, and copy once each way; vh_stream_out_host sizes the scratch from the
 * count, so `capacity` may be generous. */
#define VH_STREAM_BOX    0
#define VH_STREAM_SPHERE 1
typedef struct vh_stream_region {
    int32_t kind;                       /* VH_STREAM_BOX | VH_STREAM_SPHERE */
    int32_t invert;                     /* 1: the complement */
    int32_t block_lo[3], block_hi[3];
    float   centre[3], radius;          /* world metres */
} vh_stream_region;

#define VH_STREAM_PLACED   0
#define VH_STREAM_PRESENT  1
#define VH_STREAM_UNPLACED 2
#define VH_STREAM_FOREIGN  3
typedef struct vh_stream_stats { uint64_t placed, present, unplaced, foreign; uint32_t rounds; } vh_stream_stats;

int vh_stream_out(vh_context *ctx, const vh_stream_region *region, uint64_t capacity, vh_view_record *d_records,
                  uint32_t *d_colors /* capacity * 512 words or NULL */, uint64_t *selected_out, uint64_t *written_out);
int vh_stream_in(vh_context *ctx, uint64_t n, const vh_view_record *d_records, const uint32_t *d_colors /* n * 512 words or NULL */,
                 int32_t *d_status /* n or NULL */, vh_stream_stats *stats /* host, may be NULL */);
int vh_stream_out_host(vh_context *ctx, const vh_stream_region *region, uint64_t capacity, vh_view_record *h_records,
                       uint32_t *h_colors, uint64_t *selected_out, uint64_t *written_out);
int vh_stream_in_host(vh_context *ctx, uint64_t n, const vh_view_record *h_records, const uint32_t *h_colors, int32_t *h_status,
                      vh_stream_stats *stats);

/* ------------------------------------------------------------------ */
/* connected pieces of the model                       */
/* ------------------------------------------------------------------ */
/* vh_components labels the connected pieces of the fused model; vh_remove_components takes the small ones out of the volume,
 * so that every later vh_extract_mesh*, vh_raycast, vh_cast_rays and vh_esdf_lattice is free of them.  The rule is in
 * integers: the GPU gives the bits of tests/components_ref.py.
 *   Valid voxel.  vh_sample_sdf's rule: its block is allocated in this table (or shard), weight > 0, and its sdf is not NaN.
 *   Nodes.  target VH_COMPONENT_INSIDE: the valid voxels with sdf <= 0 (the mesh's inside rule: -0.0, +0.0 and -inf are
 *     inside), so a component is what the mesh shows as one closed piece.  VH_COMPONENT_OUTSIDE: the other valid voxels
 *     (pockets and bubbles).  Only voxels of blocks inside `region` (NULL: the whole model) are nodes: a region boundary, an
 *     absent block and a block of another shard all cut the graph.
 *   Edges.  connectivity 6: nodes A and B are joined iff B - A = +-e for an axis unit vector e.  connectivity 14: iff
 *     B - A = +-o for o in {0,1}^3 \ {0}: exactly the edges (A, d), d = 1..7, of the Kuhn split vh_extract_mesh_indexed
 *     anchors at every voxel, so two inside voxels are joined iff the mesh's own tetrahedra join them.  (1, -1, 0) and its
 *     kin are not edges.  There is no other connectivity, in particular no 26.
 *   Identity and order.  A node's id is rank * 512 + voxel index: rank = the position of its block in the ordered block list
 *     (ascending entry index, the mesh's order), voxel index = ((z&7)<<6)|((y&7)<<3)|(x&7).  A component's root is its node
 *     of least id; components are output in ascending root id.  The same table gives the same bytes; the partition and the
 *     multiset of sizes do not depend on the table at all.
 *   Limit.  Ids fit a uint32 with VH_COMPONENT_NONE reserved: a region with more than 2^23 - 1 listed blocks returns
 *     VH_ERR_INVALID_ARGUMENT; stats->blocks is reported, the other counts are 0 and nothing is written.
 *
 * vh_components writes the first `capacity` records, in order, and reports what the region holds even when that exceeds the
 * capacity, as vh_extract_mesh does (capacity 0 with NULL buffers: the count-only call).  d_labels has vh_sample_lattice's
 * layout over lo, dims: the index of the voxel's component in output order (it may be at or beyond `capacity`), or
 * VH_COMPONENT_NONE where the voxel is no node.  stats: blocks listed, nodes, components and the largest component's size; the
 * removal fields are 0.  The call runs on the context's stream behind every queued frame (a pending pipelined frame is
 * launched first), synchronises once to return the stats, and changes nothing in the model.  It works on shards, on view
 * tables and with or without "overflow_list".  Its scratch (one uint32 per voxel of the listed blocks, one word per pool block,
 * eight words and a count per listed block) is allocated at the first call, grown on demand and kept; a context that never
 * calls it allocates nothing for it.  VH_ERR_INVALID_ARGUMENT: an unknown target or connectivity, a capacity without a
 * buffer, a box given in part (lo, dims and d_labels: all three or none), a box vh_sample_lattice refuses.
 *
 * vh_remove_components labels in the same way, then every node of a component with size < min_size becomes {0, 0}, as a
 * de-integrated voxel does, and its colour word 0 where a colour volume exists.  A block in which the call cleared at least
 * one voxel and whose 512 weights are then all 0 is freed through the deletion path of vh_delete_blocks, in a lock epoch of
 * its own (vh_counters.last_freed / freed_total say what was freed; the compact list is left as vh_delete_blocks leaves it);
 * blocks that were empty before are left alone.  min_size 0 or 1 removes nothing.  Removing is idempotent, and clearing
 * whole components never splits another.  stats as above, of the labelling before the removal, plus the components and
 * voxels removed and the blocks freed.  View tables are refused (they own no blocks).  The call synchronises.
 * Diagnostics: vh_set_option(ctx, "components_launches", k) with k = 1..6 makes both calls stop behind the first k stages of
 * the labelling (block list, local pass, seam pass, flatten, count, scan + records), for tools/components_time.py: such a
 * call returns no result and removes nothing.  0 or 7: the whole call (the default). */
#define VH_COMPONENT_INSIDE  0
#define VH_COMPONENT_OUTSIDE 1
#define VH_COMPONENT_NONE    0xFFFFFFFFu
typedef struct vh_component { int32_t voxel[3]; uint32_t size; } vh_component;        /* 16 B: global voxel of the root, nodes */
typedef struct vh_component_stats { uint64_t blocks, nodes, components, largest,      /* of the labelling */
                                    removed_components, removed_voxels, freed_blocks; } vh_component_stats;

int vh_components(vh_context *ctx, const vh_mesh_region *region /* NULL: whole model */, int32_t target, int32_t connectivity,
                  uint64_t capacity, vh_component *d_components /* may be NULL when capacity is 0 */,
                  const int32_t lo[3], const int32_t dims[3], uint32_t *d_labels /* all three NULL, or a lattice box */,
                  vh_component_stats *stats /* host */);
int vh_components_host(vh_context *ctx, const vh_mesh_region *region, int32_t target, int32_t connectivity, uint64_t capacity,
                       vh_component *h_components, const int32_t lo[3], const int32_t dims[3], uint32_t *h_labels,
                       vh_component_stats *stats);
int vh_remove_components(vh_context *ctx, const vh_mesh_region *region, int32_t target, int32_t connectivity,
                         uint64_t min_size, vh_component_stats *stats /* host, may be NULL */);

/* ------------------------------------------------------------------ */
/* the model with labels                               */
/* ------------------------------------------------------------------ */
/* A per-pixel segmentation (the label image of a network, registered to the depth image) fused into the voxels near the
 * surface, read back at points, at mesh vertices or per pixel of a raycast, counted per class, and acted on: everything that
 * carries one label taken out of the volume.  tests/labels_ref.py is the rule in executable form; the reference has none.  The
 * rule is all integers: the same model and images give the same words.  (The d_labels of vh_components holds component
 * indices and has nothing to do with this section; "semantics" keeps meaning REFERENCE / PINHOLE.)
 *   Voxel stays {sdf, weight}: labels live in a third volume of one uint32 per voxel, numVoxelBlocks * 512 words, the voxel at
 *   volume index ptr + i having its word at ptr + i (the colour volume's layout).
 *   Word: label | votes << 16, label 1..65535, votes 1..65535.  The word 0 means "no label".
 *   The volume is allocated, zeroed, by the first label-fusing call into a context and kept.  A failed allocation returns
 *   VH_ERR_OUT_OF_MEMORY and nothing changes.  A context that never fuses labels allocates nothing and behaves exactly as
 *   before.  DevPtrs, Voxel, VoxelEntry, the snapshot format and vh_view_record are unchanged.
 * FUSING.  d_labels is W*H uint16 values registered to the depth image; the value 0 marks a pixel the segmentation did not label.
 *   Block set: vh_integrate_color's -- every allocated entry of this table (or shard) that passes blockInFrustum for `pose`,
 *     the compact set of vh_set_pose(pose) + vh_flatten, chained overflow entries included.  No block is allocated or freed.
 *   Per voxel of a listed block, with the stored voxel {os, ow} and its label word c = (l, n), l = c & 0xFFFF, n = c >> 16:
 *     1. !(ow > 0): the word becomes 0 and nothing else happens to this voxel -- the sweep: a voxel that holds nothing has no
 *        label, which also clears the labels a de-integration orphaned.
 *     2. The camera point by the context's semantics, project, the image bounds test, the depth read, depth <= 0 rejects and
 *        !(fabsf(depth - cz) <= band) rejects: all exactly as in vh_integrate_color.  A rejected voxel is untouched.
 *     3. vote_max == 0, or the pixel's label L == 0: the voxel is untouched.
 *     4. Otherwise one Boyer-Moore vote is cast:
 *          n == 0            -> (L, 1)
 *          l == L            -> (l, min(n + 1, vote_max))
 *          l != L, n > 1     -> (l, n - 1)
 *          l != L, n == 1    -> the word 0
 *        Below the cap the stored label is a label that holds a strict majority of the votes cast, if there is one; vote_max
 *        bounds how many opposing votes it takes to change a voxel's mind.
 *   vh_integrate_labels reads the uint16 sensor image with vh_integrate_depth's arithmetic, vh_integrate_labels_map the .z of a
 *   float4 vertex map.  Afterwards the context's pose is `pose`, the compact list and vh_counters.occupied are the flatten's;
 *   the lock epoch, the heap, the hash table, the SDF volume and the colour volume are unchanged.  A pending pipelined frame is
 *   launched first.  The calls only enqueue.  In vh_kernel_times the launch counts as integrate_ms, its flatten as flatten_ms.
 *   Both semantics; with or without the overflow list; on shards every shard is called with the same arguments and labels its
 *   own blocks.
 *   VH_ERR_INVALID_ARGUMENT, with nothing changed: a NULL argument; band not finite or <= 0; vote_max outside 0..65535; a
 *   context that holds an imported view.
 * READING.  The domain, u = p / voxelSize, the nearest-voxel choice and voxel validity are those of vh_sample_sdf, mode
 *   VH_SAMPLE_NEAREST ("the model as a distance field"); labels do not interpolate.  Output: the stored word (label |
 *   votes << 16) if the voxel is valid and votes >= max(min_votes, 1), else 0.
 *   vh_sample_labels_map: points in the camera frame; a point with .z == 0 gives 0, otherwise the point is moved by `pose`
 *   with vh_sample_color_map's arithmetic and the rule above applies.  vh_raycast_labels is exactly vh_raycast_maps followed by
 *   vh_sample_labels_map over its vertex map.
 *   No label volume (or a context that holds an imported view): every output is 0, VH_OK.  The device calls only enqueue,
 *   behind every queued frame; they allocate nothing and change nothing.  Argument checks are vh_sample_color's;
 *   vh_sample_labels_host takes host buffers and synchronises.
 * COUNTING.  vh_label_counts over the allocated blocks of `region` (NULL: the whole model; of this shard): for 1 <= l < n_bins
 *   d_counts[l] = the valid voxels whose word has label l and votes >= max(min_votes, 1); d_counts[0] = the valid voxels
 *   counted nowhere else (unlabelled, below min_votes, or a label >= n_bins), so the bins always sum to the valid voxels of
 *   the region.  n_bins 1..65536; the call zeroes d_counts itself.  No label volume: everything goes to bin 0.  The call only
 *   enqueues (its block list is the mesh's, whose scratch the first listing call allocates).
 * REMOVING.  vh_remove_label: every voxel of the region's blocks whose word has `label` (1..65535) and votes >=
 *   max(min_votes, 1) becomes {0, 0}, as a de-integrated voxel; its colour word, where a colour volume exists, becomes 0; its
 *   label word becomes 0.  A block in which this pass cleared a voxel and whose 512 weights are then all == 0 is freed through
 *   the deletion path of vh_delete_blocks, in a lock epoch of its own, exactly as vh_remove_components frees
 *   (vh_counters.last_freed / freed_total; the compact list is left as vh_delete_blocks leaves it).  stats: the blocks listed,
 *   the voxels cleared, the blocks freed.  The call synchronises.  VH_ERR_INVALID_ARGUMENT, with nothing changed: a context
 *   that holds an imported view; a context without a label volume; a label outside 1..65535.
 *   Limit: only voxels within `band` of the surface ever carry a label, so an object leaves the volume completely only if it
 *   was labelled with band >= the truncation; with a thinner band the voxels between band and truncation stay, as a shell
 *   without a zero crossing.
 * KEEPING IT CONSISTENT.  A pool block that is not allocated has 512 zero label words: vh_delete_blocks, vh_garbage_collect,
 *   vh_remove_components, vh_remove_label and vh_stream_out zero the label words of the blocks they free (so streaming a
 *   block out drops its labels); vh_load_snapshot clears the volume.  vh_merge, vh_stream_out / vh_stream_in, vh_deintegrate*,
 *   vh_changes' digest, snapshots, vh_save_color and view records neither carry nor read labels; carrying labels through them
 *   is future work, as it was for colour.  After a plain de-integration the pairing is
 *   vh_integrate_labels(old_pose, ..., vote_max = 0), which is the sweep.
 *   vh_has_labels: 0 or 1.  vh_clear_labels zeroes the volume if there is one (enqueues only).  vh_download_labels
 *   synchronises; VH_ERR_INVALID_ARGUMENT when there is no volume or the range is beyond it.
 * Measured: nothing is promised; DESIGN.md 4.25 says what tools/labels_time.py printed, or that it has not run yet. */
typedef struct vh_label_stats { uint64_t blocks, removed_voxels, freed_blocks; } vh_label_stats;

int vh_integrate_labels(vh_context *ctx, const float pose[16], const uint16_t *d_depth, const float k_inv[9],
                        const uint16_t *d_labels, float band, int32_t vote_max);
int vh_integrate_labels_map(vh_context *ctx, const float pose[16], const vh_float4 *d_verts, const uint16_t *d_labels,
                            float band, int32_t vote_max);
int vh_has_labels(vh_context *ctx);
int vh_clear_labels(vh_context *ctx);
int vh_download_labels(vh_context *ctx, size_t first_voxel, uint32_t *host_dst, size_t count);   /* synchronises */
int vh_sample_labels(vh_context *ctx, uint64_t n, const float *d_points /* n*3, world metres */, int32_t min_votes,
                     uint32_t *d_words_out /* n words */);
int vh_sample_labels_host(vh_context *ctx, uint64_t n, const float *h_points, int32_t min_votes, uint32_t *h_words_out);
int vh_sample_labels_map(vh_context *ctx, const float pose[16], uint64_t n, const vh_float4 *d_points /* camera frame */,
                         int32_t min_votes, uint32_t *d_words_out);
int vh_raycast_labels(vh_context *ctx, const float pose[16], float t_min, float t_max, float *d_depth_out,
                      vh_float4 *d_vertices_out, vh_float4 *d_normals_out, int32_t min_votes, uint32_t *d_words_out);
int vh_label_counts(vh_context *ctx, const vh_mesh_region *region /* NULL: whole model */, int32_t min_votes,
                    int32_t n_bins /* 1..65536 */, uint32_t *d_counts /* n_bins words */);
int vh_label_counts_host(vh_context *ctx, const vh_mesh_region *region, int32_t min_votes, int32_t n_bins,
                         uint32_t *h_counts);                                                    /* host buffer; synchronises */
int vh_remove_label(vh_context *ctx, const vh_mesh_region *region /* NULL: whole model */, int32_t label /* 1..65535 */,
                    int32_t min_votes, vh_label_stats *stats /* host, may be NULL */);

/* ------------------------------------------------------------------ */
/* incremental meshing: which blocks changed, and their triangles      */
/* (tests/changes_ref.py is the rule in executable form) */
/* ------------------------------------------------------------------ */
/* A live consumer of the model (a viewer, a remote client, a planner's map) keeps a mesh chunk per block and re-meshes only
 * the blocks a frame, a merge, a de-integration, a collection, a streaming call or a component removal touched.  No
 * model-changing call records what it touched: vh_changes finds out afterwards, by comparing a digest of every allocated
 * block's bits with a small STATE the caller keeps, so one streaming read of the allocated blocks serves every call that
 * changes the model, whichever and however many ran since the state last advanced.
 *
 * State.  A device buffer the caller owns, vh_changes_state_bytes() bytes (64 + 32 per block of the pool); all-zero bytes
 * is the empty state (nothing seen yet).  Layout (part of this specification): a 64-byte header whose first uint64 is the
 * EPOCH, the number of calls that advanced the state, the rest zero; then one 32-byte slot per pool block, indexed by the
 * block's ptr >> 9: {int32 key[3]; uint32 live; uint64 h0; uint64 h1}.  An empty slot is all zero.  One state serves one
 * `what` and one context.
 *
 * Digest of a block, in wrapping uint64 arithmetic.  For voxel i = 0..511: x_i = (uint64)bits(weight) << 32 | bits(sdf).
 *     mix(z):  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31   (splitmix64)
 *     G = 0x9e3779b97f4a7c15;   m_i = mix(x_i + (i + 1) * G + what);   h0 = sum m_i;   h1 = sum m_i * (2 i + 1)
 * With VH_CHANGES_COLOR the colour word c_i of every voxel (0 while the context has no colour volume) adds a term:
 *     m'_i = mix(c_i + (i + 513) * G + what), added to h0, and m'_i * (2 (i + 512) + 1), added to h1.
 * Bits are compared: -0.0 against +0.0 and two NaN payloads differ.  What the digest guarantees: mix is a bijection, so a
 * change confined to ONE voxel's {sdf, weight} pair, or to ONE colour word, of a block is ALWAYS detected.  Its limit: any
 * other change of a block goes unnoticed only if both 64-bit sums collide, heuristically with a probability of the order
 * of 2^-64 or less per block and comparison; the digest is NOT cryptographic, and bits chosen by an adversary can collide.
 *
 * Rule.  The allocated blocks of the region grown by one block on every side (saturating at the ends of int32) are listed
 * in ascending entry index of the hash table (the mesh's block list).
 *   A listed block INSIDE the region, key K, pool slot p = ptr >> 9, is SELF-CHANGED iff state slot p is not live, holds
 *     another key, or holds another digest.
 *   A live state slot whose key lies inside the region is STALE iff no listed block of this call has that slot and key.
 *   A stale slot's key is REMOVED iff the table holds no entry with that key now (the bucket probe, overflow list
 *     included).  A key that came back under another pool slot is not removed: it is self-changed at its new slot.
 *   Halo.  For every self-changed or removed key k the allocated blocks k + o, o != 0, are listed with the halo flag:
 *     VH_CHANGES_HALO_NONE none; VH_CHANGES_HALO_MESH o in {-1, 0}^3 (the cells of block j read the blocks j + {0, 1}^3:
 *     what vh_extract_mesh_blocks without normals depends on); VH_CHANGES_HALO_NORMALS o in {-1, 0, 1}^3 (the gradient at
 *     an apron voxel reaches one voxel further both ways: with normals).  Halo blocks one block outside the region are
 *     listed too.
 *   d_changed: 4 int32 per block, {x, y, z, flags}, flags = VH_CHANGED_SELF | VH_CHANGED_HALO (a block can carry both), in
 *     ascending entry index.  d_removed: {x, y, z, 0} in ascending state slot.  Both orders are reproducible.
 *   Commit, all or nothing, decided on the device: iff BOTH counts fit their capacities the lists are written and the state
 *     advances -- the slots of the self-changed blocks are written, the stale slots emptied, the epoch counted up (also
 *     when nothing changed).  Otherwise the counts are reported (VH_OK), nothing is written to the lists, the state is byte
 *     for byte what it was, and the caller calls again with larger buffers.  So capacity 0 with NULL buffers is a PEEK that
 *     consumes changes only when there are none.  Changes outside the region stay pending for a later call.
 * The call runs on the context's stream behind every frame queued so far (a pending pipelined frame is launched first),
 * reads the two counts back in one copy, synchronises once, and changes nothing in the model.  It works on shards (a block
 * of another shard is absent: never halo, never keeping a key from being removed) and with "overflow_list".  View tables
 * are refused with VH_ERR_INVALID_ARGUMENT: they are rebuilt by import, not edited.  VH_ERR_INVALID_ARGUMENT also for a
 * NULL state or count, a `what` without VH_CHANGES_VOXELS or with unknown bits, an unknown halo, a capacity without its
 * buffer.  Scratch beyond the block list's (a flag word and two digest words per listed block, three words per pool block)
 * is allocated at the first call and kept; a context that never calls this allocates nothing for it.  vh_changes_host
 * takes host lists (the state stays a device buffer). */
#define VH_CHANGES_VOXELS 1
#define VH_CHANGES_COLOR  2
#define VH_CHANGES_HALO_NONE    0
#define VH_CHANGES_HALO_MESH    1
#define VH_CHANGES_HALO_NORMALS 2
#define VH_CHANGED_SELF 1
#define VH_CHANGED_HALO 2
int vh_changes_state_bytes(vh_context *ctx, uint64_t *bytes);
int vh_changes(vh_context *ctx, void *d_state, const vh_mesh_region *region /* NULL: whole model */,
               int32_t what /* VH_CHANGES_VOXELS [| VH_CHANGES_COLOR] */, int32_t halo /* VH_CHANGES_HALO_* */,
               uint64_t capacity_changed, int32_t *d_changed /* 4 per block: x, y, z, flags */,
               uint64_t capacity_removed, int32_t *d_removed /* 4 per block: x, y, z, 0 */,
               uint64_t *changed_out, uint64_t *removed_out /* host */);
int vh_changes_host(vh_context *ctx, void *d_state, const vh_mesh_region *region, int32_t what, int32_t halo,
                    uint64_t capacity_changed, int32_t *h_changed, uint64_t capacity_removed, int32_t *h_removed,
                    uint64_t *changed_out, uint64_t *removed_out);

/* The triangles of a LIST of blocks, block by block.  d_keys: n keys, 4 int32 each, the 4th ignored (vh_changes' d_changed
 * feeds it directly).  For key j of the list the call writes the triangles of the cells block j owns: exactly the bytes
 * vh_extract_mesh writes for the region [j, j + 1), positions and normals, at triangles d_first[j] .. d_first[j + 1] of the
 * buffers, in the list's order.  An absent key has an empty range; a key that occurs twice gets its copy each time.
 * d_first (n + 1 uint64 on the device, or NULL) always holds the unclipped offsets; clipping at the capacity, the count-only
 * call and *triangles_out are as in vh_extract_mesh.  n == 0 returns VH_OK with 0 triangles and launches nothing; n above
 * the number of blocks the table can hold (numVoxelBlocks; the imported records of a view table) is
 * VH_ERR_INVALID_ARGUMENT.  Stream order, the one synchronisation, shards, view tables and "mesh_variant" as for
 * vh_extract_mesh.  There is no per-block indexed form (vertex ownership crosses blocks); per-vertex colour is
 * vh_sample_color over the positions. */
int vh_extract_mesh_blocks(vh_context *ctx, uint64_t n, const int32_t *d_keys /* 4 per block; the 4th is ignored */,
                           uint64_t capacity_triangles, float *d_positions, float *d_normals /* or NULL */,
                           uint64_t *d_first /* n + 1 offsets, device, or NULL */, uint64_t *triangles_out);
int vh_extract_mesh_blocks_host(vh_context *ctx, uint64_t n, const int32_t *h_keys, uint64_t capacity_triangles,
                                float *h_positions, float *h_normals, uint64_t *h_first, uint64_t *triangles_out);

/* ------------------------------------------------------------------ */
/* model dump / checkpoint                     */
/* ------------------------------------------------------------------ */
/* Text dump in the format of SDFRenderer::printSDFdata (SDFRenderer.cpp:71-110, written to
 * SDF_dump.txt by the reference): occupied count, then per compact entry pos / ptr / offset
 * and 512 sdf values at 4 decimals.  Like the original, entry i is followed by voxels
 * [512*i, 512*i+512) of the volume, not by the block its ptr names.  Synchronises. */
int vh_dump_sdf_text(vh_context *ctx, const char *path);
/* Binary snapshot of the model (hash table, heap, counters, the 4 KiB block of every
 * allocated entry) and its restore into a context created with the same configuration;
 * fusing can continue after vh_load_snapshot as if never interrupted.  Both synchronise.
 * Snapshots do not carry colour: vh_load_snapshot clears the colour volume ("the model in colour").  A coloured model is
 * saved as the pair vh_save_snapshot + vh_save_color and resumed with vh_load_snapshot followed by vh_load_color.
 * vh_counters after a load: heap_counter, allocated_total, heap_exhausted and epoch are the saved context's; freed_total is
 * allocated_total minus the allocated entries (the file does not carry it; that is its value at the save, so the pool accounting
 * allocated_total - freed_total == allocated entries holds on); the other counters are 0.  What the compact list holds after a
 * load, and after vh_clear_color, is not specified: the next frame or flatten makes it. */
int vh_save_snapshot(vh_context *ctx, const char *path);
int vh_load_snapshot(vh_context *ctx, const char *path);

/* ------------------------------------------------------------------ */
/* depth pre-processing                        */
/* ------------------------------------------------------------------ */
/* preProcess (CameraTrackingUtils.cu:115-120) = calculateVertexPositions (:50-73) +
 * calculateNormals (:75-113) as one kernel: uint16 depth (5000 units = 1 m, 0 = invalid)
 * -> float4 vertex map (K_inv*(x,y,1)*depth, w = 1; invalid -> (0,0,0,1)) and float4
 * normal map (central-difference cross product, normalised; 0 on the border or next to an
 * invalid pixel).  k_inv: the 3x3 the reference uploads with SetCameraIntrinsic, read
 * row-major.  The outputs are what vh_integrate takes as d_verts / d_normals. */
int vh_preprocess(const uint16_t *d_depth, const float k_inv[9], int32_t width, int32_t height,
                  vh_float4 *d_positions, vh_float4 *d_normals, void *hip_stream);
/* the reference's own names (CameraTrackingUtils.cu:218-222, 115-120): 640x480, default
 * stream, synchronous */
bool SetCameraIntrinsic(const float *intrinsic, const float *invIntrinsic);
void preProcess(vh_float4 *positions, vh_float4 *normals, const uint16_t *depth);

/* ------------------------------------------------------------------ */
/* camera tracking: frame-to-frame point-to-plane ICP                  */
/* (second half)                               */
/* ------------------------------------------------------------------ */
/* The reference's tracker (CameraTracking::Align, CameraTracking.cpp:27-69; never called,
 * Application.cpp:75) aligns the vertex map of one frame (input) to the vertex + normal maps of
 * another (target): per round FindCorrespondences (CameraTrackingUtils.cu:131-185) projects every
 * input point, moved by the current estimate, into the target image and keeps the pair when the
 * point-to-plane distance d = dot(q - t, n) is below the threshold; CalculateJacAndResKernel
 * (Solver.cu:40-54) writes the 6 x N Jacobian [n, t x n]; cublasSgemv / cublasSsyrk reduce it to
 * J^T r and J^T J (Solver.cpp:81-90); the host solves and composes in SE3 (Solver.cpp:104-106,
 * SE3.cpp).  Here one fused pass per round produces the 27 sums directly.  With the target maps
 * taken from vh_raycast + vh_depth_to_maps this is the frame-to-model tracking of KinectFusion. */
#define VH_ICP_ABS_DISTANCE 1   /* keep |d| < threshold (the reference keeps the signed d < threshold, :170) */
#define VH_ICP_NEED_TARGET  2   /* skip pixels whose target has no depth or no normal (the reference pairs them) */

typedef struct vh_icp vh_icp;    /* workspace for one image size on one device */
typedef struct vh_icp_system {
    double   JTJ[36];            /* row-major, symmetric; parameter order (v, w) = translation, rotation */
    double   JTr[6];
    double   error;              /* sum of d over the kept pairs (computeCorrespondences' return value) */
    uint32_t count;              /* kept pairs */
} vh_icp_system;

int vh_icp_create(int32_t width, int32_t height, int32_t device /* -1: current */, vh_icp **out);
int vh_icp_destroy(vh_icp *icp);
int vh_icp_set_stream(vh_icp *icp, void *hip_stream);
/* One round's linear system for the estimate `delta` (row-major 4x4 mapping input points into the
 * target's camera frame); K = row-major intrinsics.  Device maps are width*height float4.  fp32
 * sums in a fixed order (reproducible); synchronises to return the system. */
int vh_icp_build_system(vh_icp *icp, const vh_float4 *d_input, const vh_float4 *d_target,
                        const vh_float4 *d_target_normals, const float delta[16], const float K[9],
                        float dist_thres, int32_t flags, vh_icp_system *out);
/* The same, and also the three maps computeCorrespondences fills (zero where no pair is kept). */
int vh_icp_correspondences(vh_icp *icp, const vh_float4 *d_input, const vh_float4 *d_target,
                           const vh_float4 *d_target_normals, const float delta[16], const float K[9],
                           float dist_thres, int32_t flags, vh_float4 *d_corres, vh_float4 *d_corres_normals,
                           float *d_residuals, vh_icp_system *out);
/* Host only.  update = -(JTJ^-1 JTr) by an LDL^T factorisation, estimate = log(exp(update) exp(estimate)) with
 * twists (v, w) as in SE3.cpp:4-22.  VH_ERR_SINGULAR leaves the estimate untouched. */
int  vh_icp_solve(const vh_icp_system *sys, double estimate[6]);
void vh_se3_exp(const double twist[6], double T[16]);
void vh_se3_log(const double T[16], double twist[6]);
/* Up to max_iters rounds (the reference: 20; 0 <= max_iters <= 65536, else VH_ERR_INVALID_ARGUMENT) from the start value
 * in `delta`, which receives the result; stops early when the summed residual is exactly 0 (:52) or the system is singular.
 * All rounds run in ONE launch whose workgroups wait for each other between rounds
 * (VH_ICP_PERSISTENT=0 in the environment at vh_icp_create: one launch per round -- same result,
 * bit for bit).  The waits are bounded: VH_ERR_TIMEOUT when a
 * workgroup gave up (another kernel holding the chip for about a second), `delta` is then untouched. */
int vh_icp_align(vh_icp *icp, const vh_float4 *d_input, const vh_float4 *d_target,
                 const vh_float4 *d_target_normals, const float K[9], float dist_thres, int32_t max_iters,
                 int32_t flags, float delta[16], vh_icp_system *last, int32_t *iterations);
/* float depth image in metres (0 = nothing, e.g. vh_raycast's output) -> vertex + normal maps with
 * the arithmetic of preProcess; asynchronous on hip_stream. */
int vh_depth_to_maps(const float *d_depth, const float k_inv[9], int32_t width, int32_t height,
                     vh_float4 *d_positions, vh_float4 *d_normals, void *hip_stream);
/* vh_raycast, then vertex and normal maps (camera frame) of the same view, with the K^-1 of the
 * raycast intrinsics: the model as an ICP target (raycast(pose, depth, normals)). */
int vh_raycast_maps(vh_context *ctx, const float pose[16], float t_min, float t_max, float *d_depth_out,
                    vh_float4 *d_vertices_out, vh_float4 *d_normals_out);
/* One frame of the closed loop (the demo's frame order, Application.cpp:73-90, with the tracker switched on):
 * vh_preprocess(d_depth) -> vh_icp_align(input maps, model maps; start = identity) -> pose <- pose . delta (row-major
 * double 4x4, in / out) -> vh_integrate_depth(pose, d_depth) -> vh_raycast_maps(pose) into the model maps for the next
 * frame.  Everything runs on the context's stream (the tracker must be bound to it: vh_icp_set_stream); the one host
 * synchronisation is the one inside vh_icp_align.  The first frame of a sequence is vh_integrate_depth + vh_raycast_maps
 * at the start pose.  d_input_*: scratch maps the call fills. */
int vh_fusion_step(vh_context *ctx, vh_icp *icp, const uint16_t *d_depth, const float k_inv[9], const float K[9],
                   float dist_thres, int32_t max_iters, int32_t flags, float t_min, float t_max,
                   vh_float4 *d_input_vertices, vh_float4 *d_input_normals, float *d_model_depth,
                   vh_float4 *d_model_vertices, vh_float4 *d_model_normals, double pose[16],
                   vh_icp_system *last, int32_t *iterations);
/* the reference's own name (CameraTrackingUtils.cu:187-215; float4x4 by value there, a pointer to
 * its 16 row-major floats here): intrinsics from SetCameraIntrinsic, threshold 0.08 (common.h:12),
 * synchronous, returns the summed residual */
float computeCorrespondences(const vh_float4 *d_input, const vh_float4 *d_target,
                             const vh_float4 *d_targetNormals, vh_float4 *corres, vh_float4 *corresNormals,
                             float *residual, const float *deltaTransform, int width, int height);

/* ------------------------------------------------------------------ */
/* drop-in names (VoxelUtils.h:5-13); process-global default context    */
/* ------------------------------------------------------------------ */
/* The reference declares these with `const HashTableParams&`; a C++ reference
 * is a pointer at the ABI level, so the C declarations take a pointer.
 * Errors follow the reference convention: message on stderr + exit(1).
 * mapGLobjectsToCUDApointers (VoxelUtils.h:13) is not carried over: the
 * compact table / counter / volume are library-owned device buffers. */
void updateConstantHashTableParams(const HashTableParams *params);
void deviceAllocate(const HashTableParams *params);
void deviceFree(void);
void resetHashTableMutexes(const HashTableParams *params);
void allocBlocks(const vh_float4 *verts, const vh_float4 *normals);
int  flattenIntoBuffer(const HashTableParams *params);
void calculateKinectProjectionMatrix(void);
void integrateDepthMap(const HashTableParams *params, const vh_float4 *verts);
/* the default context behind the drop-in names (NULL before deviceAllocate) */
vh_context *vh_default_context(void);

#ifdef __cplusplus
}
#endif
#endif /* VOXELHASH_H */
