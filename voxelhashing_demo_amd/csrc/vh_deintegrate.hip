// vh_deintegrate.hip -- de-integration: the TSDF update of vh_integrate.hip run backwards for one frame.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_integrate.hip (DepthPlane, DepthSensor).
// No counterpart in the reference; BundleFusion's deIntegrate is the model (include/voxelhash.h states the rule,
// tests/deintegrate_ref.py is its executable form).
#pragma once

namespace vh {

// The frame's sample (s, cw) of voxel (vx, vy, vz): tsdf_update's computation up to, not including, combineVoxel.
// RESTATED from vh_integrate.hip on purpose -- the frame path's file stays byte-identical, and the two must agree bit
// for bit (tests/test_deintegrate_ref_cpu.py pins the numpy form of this text to the oracle's update with sign = +1,
// tests/test_gpu_deintegrate.py the kernel to the numpy form).  The line numbers are VoxelUtils.cu's, as there.
// false: the update would have returned false, the voxel stays untouched.
template <class Depth>
__device__ __forceinline__ bool frame_sample(const FrameParams &fp, const float *Tinv, const Depth &src, int vx, int vy,
                                             int vz, float &sOut, float &cwOut)
{
    float cx, cy, cz;
    if (fp.semantics == VH_SEM_REFERENCE) {
        const float4 r = mat4_mul(Tinv, (float)vx, (float)vy, (float)vz, 1.0f);          // :797-800
        cx = (float)f2i_rz(r.x) * fp.voxelSize;
        cy = (float)f2i_rz(r.y) * fp.voxelSize;
        cz = (float)f2i_rz(r.z) * fp.voxelSize;
    } else {
        const float4 r = mat4_mul(Tinv, (float)vx * fp.voxelSize, (float)vy * fp.voxelSize,
                                  (float)vz * fp.voxelSize, 1.0f);
        cx = r.x; cy = r.y; cz = r.z;
    }
    int sx, sy;
    project(fp.proj, cx, cy, cz, sx, sy);                                        // :801
    if (sx < 0 || sx >= fp.width || sy < 0 || sy >= fp.height) return false;     // :803
    const float depth = src.at(sx, sy, fp.width);                                 // :805
    if (depth <= 0.0f) return false;                                             // :806
    float sdf = depth - cz;                                                      // :813
    float trunc = fp.truncation;                                                 // :815
    if (fp.flags & kFlagDepthTruncation) trunc = fp.truncation + (fp.truncScale * depth);
    if (!(sdf > -trunc)) return false;                                           // :818
    sOut = (sdf >= 0.0f) ? __builtin_fminf(trunc, sdf) : __builtin_fmaxf(-trunc, sdf);
    float cw = 0.1f;                                                             // :829
    if (fp.flags & kFlagWeightSample) {
        const float zeroOne = (depth - 0.5f) / (5.0f - 0.5f);
        cw = __builtin_fmaxf((float)((double)fp.weightSample * 1.5 * (1.0 - (double)zeroOne)), 1.0f);
    }
    cwOut = cw;
    return true;
}

// Takes the frame's sample out of the stored voxel {sdfIO, wIO}; true: the voxel changed.
// A voxel that holds nothing (!(w > 0)) is left before its sample is computed: the outcome is the same, untouched.
// wFloor: half the smallest weight a sample can have -- what k additions followed by k subtractions of the same
// weights leave is a rounding residue far below it, a sample that genuinely remains is a whole one.
template <class Depth>
__device__ __forceinline__ bool tsdf_remove(const FrameParams &fp, const float *Tinv, const Depth &src, int vx, int vy,
                                            int vz, float &sdfIO, float &wIO)
{
    const float ow = wIO, os = sdfIO;
    if (!(ow > 0.0f)) return false;
    float s, cw;
    if (!frame_sample(fp, Tinv, src, vx, vy, vz, s, cw)) return false;
    const float wFloor = (fp.flags & kFlagWeightSample) ? 0.5f : 0.05f;
    const float nw = ow - cw;
    if (!(nw >= wFloor)) {
        sdfIO = 0.0f;                  // the zero-initialised state: invalid to the mesh, the sampler and the raycast
        wIO = 0.0f;
        return true;
    }
    sdfIO = ((os * ow) - (s * cw)) / nw;
    wIO = nw;
    return true;
}

// integrate_block's shape: the 256 lanes of a workgroup take the 8^3 block of entry e, lane t voxels 2t and 2t + 1
// (neighbours in x) as one 16-byte load and, when one of the two changed, one 16-byte store
template <class Depth>
__device__ __forceinline__ void deintegrate_block(const FrameParams &fp, const DevPtrs &dp, const VoxelEntry &e,
                                                  const Depth &src)
{
    const int lin = 2 * (int)threadIdx.x;
    const int tx = lin & 7, ty = (lin >> 3) & 7, tz = lin >> 6;
    const int bx = (int)((uint32_t)e.pos[0] * 8u) + tx;
    const int by = (int)((uint32_t)e.pos[1] * 8u) + ty;
    const int bz = (int)((uint32_t)e.pos[2] * 8u) + tz;
    float4 *cell = reinterpret_cast<float4 *>(dp.blocks + (size_t)e.ptr + lin);
    float4 v = *cell;                            // {sdf0, w0, sdf1, w1}
    const bool u0 = tsdf_remove(fp, fp.Tinv, src, bx, by, bz, v.x, v.y);
    const bool u1 = tsdf_remove(fp, fp.Tinv, src, bx + 1, by, bz, v.z, v.w);
    if (u0 || u1) *cell = v;
}

// A fixed grid strides over the dense compact list the step-level flatten left (the count stays on the device):
// entries of allocated blocks only, so every e.ptr names a whole block inside dp.blocks.
template <class Depth>
__global__ __launch_bounds__(256) void deintegrate_kernel(const FrameParams fp, const DevPtrs dp, const Depth src)
{
    const int count = dp.counters[kCompactCount];
    for (int k = (int)blockIdx.x; k < count; k += (int)gridDim.x) deintegrate_block(fp, dp, dp.compact[k], src);
}

}  // namespace vh
