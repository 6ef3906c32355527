// vh_kernels.hip -- the hand-written gfx950 kernels of the voxel-hashing TSDF path, one file
// per stage of SDF_Hashtable::integrate (SDF_Hashtable.cpp:11-40) and its neighbours:
//
//   vh_alloc.hip       allocBlocks: per-pixel block key, wave-level run dedup, bucket probe,
//                      epoch-stamped claim (allocBlocksKernel + the locking half of
//                      insertVoxelEntry, VoxelUtils.cu:606-705, 418-456); commit of the winners
//                      (VoxelUtils.cu:447-453, 328-334); key generation for the multi-GPU exchange
//   vh_walk.hip        flattenIntoBuffer: the walk over the VoxelEntry array, wave-ballot
//                      compaction of allocated in-frustum entries (flattenKernel, :719-749),
//                      and the walk over the bucket-occupancy bitmap that replaces it by default
//   vh_integrate.hip   integrateDepthMap: one 8^3 block per workgroup pass, 16-byte-per-lane
//                      voxel read-modify-write (integrateDepthMapKernel, :790-842); de-integration, the same update
//                      run backwards for one frame (BundleFusion's deIntegrate; no counterpart in the reference)
//   vh_frame.hip       the fused frame: {claim || walk} and {commit + integrate} in two launches, or pipelined in one
//   vh_shard.hip       the multi-camera frame on a bucket-range shard
//   vh_raycast.hip     per-pixel march through the hash (stand-in for SDFRenderer::render,
//                      SDFRenderer.cpp:210-255)
//   vh_view.hip        raycast over shards: export of the blocks a view can touch, view table import
//   vh_blocks.hip      block silhouettes: per-pixel nearest front / farthest back face of the allocated
//                      blocks' cubes (SDFRenderer::drawToFrontAndBack, SDFRenderer.cpp:165-208)
//   vh_gc.hip          block deletion / garbage collection (deleteVoxelEntry :544-604 done correctly)
//   vh_blocklist.hip   the ordered block list of a region (count -> scan -> write over the bucket range) and the two-level
//                      scan: the front end of the mesh, the components and block streaming (no counterpart in the reference)
//   vh_mesh.hip        iso-surface extraction: ordered block list, marching tetrahedra per block behind a 9^3 apron in
//                      LDS, count -> scan -> emit (no counterpart in the reference)
//   vh_sample.hip      the model as a distance field: sdf / weight / gradient at world points (one point per lane),
//                      dense boxes of the voxel lattice (one workgroup pass per brick; no counterpart in the reference)
//   vh_esdf.hip        the Euclidean distance to the surface on the lattice: bit planes of the classes, an exact capped
//                      squared distance transform axis by axis (no counterpart in the reference)
//   vh_rays.hip        the DDA raycast for arbitrary ray batches: one ray per lane through vh_raycast.hip's per-lane walk
//                      (no counterpart in the reference)
//   vh_track.hip       camera tracking against the model itself: the ICP's round with the trilinear sample of the model as
//                      residual and its gradient as normal, and the joint form with a photometric row, the luminance of the
//                      cell's eight colour words against the input image (no counterpart in the reference)
//   vh_merge.hip       one model fused into another under a rigid transform: candidate keys from the source's blocks through the
//                      bin insertion path, then the TSDF update's launch shape with the distance-field sample as the measurement
//                      (no counterpart in the reference); the same launch with src's colour carried along (vh_merge_color)
//   vh_color.hip       the model in colour: a second volume of one word per voxel, the registered colour image fused into the
//                      voxels near the surface in the TSDF update's launch shape and taken back out of them, colour at world
//                      points with the sampler's shared look-ups (no counterpart in the reference)
//   vh_labels.hip      the model with labels: a third volume of one word per voxel, a segmentation's label image fused into the
//                      voxels near the surface as Boyer-Moore votes in colour's launch shape, labels at world points, valid voxels
//                      per label with wave-aggregated atomics, one label taken out of the volume through the deletion path (no
//                      counterpart in the reference)
//   vh_stream.hip     block streaming: the blocks of a region out of the model as records (ordered list, pack, the deletion
//                      path) and records back in (classification, the bin insertion path, one placed record per key); no
//                      counterpart in the reference
//   vh_components.hip  connected pieces of the model: a union-find over the sparse blocks (in LDS inside a block, atomicMin on the
//                      larger root across the seams), sizes, records and labels in root order, removal of the small pieces
//                      through the deletion path (no counterpart in the reference)
//   vh_changes.hip     incremental meshing: a digest per block against a caller-kept state says which blocks changed, were removed
//                      or read a changed neighbour; a list of keys in front of the mesh's per-block kernel (no counterpart in
//                      the reference)
//   vh_preprocess.hip  depth -> vertex / normal maps (preProcess, CameraTrackingUtils.cu:50-120),
//                      table set-up kernels (VoxelUtils.cu:151-166), device-side test hook
//   vh_icp.hip         frame-to-frame point-to-plane ICP: correspondences + Jacobian + J^T J / J^T r in one
//                      pass (CameraTrackingUtils.cu:131-185, Solver.cu:19-54, Solver.cpp:81-90)
//
// All of it is integer / fp32 scalar work bound by HBM traffic, latency or VALU issue; there is
// no contraction to hand to MFMA.  Built with -ffp-contract=off (see vh_device.h).
#include "vh_device.h"

#include "vh_alloc.hip"
#include "vh_walk.hip"
#include "vh_integrate.hip"
#include "vh_frame.hip"
#include "vh_shard.hip"
#include "vh_raycast.hip"
#include "vh_raycast_coop.hip"
#include "vh_view.hip"
#include "vh_gc.hip"
#include "vh_blocks.hip"
#include "vh_preprocess.hip"
#include "vh_icp.hip"
#include "vh_blocklist.hip"
#include "vh_mesh.hip"
#include "vh_sample.hip"
#include "vh_esdf.hip"
#include "vh_rays.hip"
#include "vh_track.hip"
#include "vh_merge.hip"
#include "vh_color.hip"
#include "vh_labels.hip"
#include "vh_stream.hip"
#include "vh_components.hip"
#include "vh_changes.hip"
