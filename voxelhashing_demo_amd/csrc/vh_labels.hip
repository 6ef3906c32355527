// vh_labels.hip -- the model with labels: vh_integrate_labels, vh_sample_labels, vh_label_counts, vh_remove_label (DESIGN.md
// 4.25; the rule: include/voxelhash.h, "the model with labels", and tests/labels_ref.py).  No counterpart in the reference.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_color.hip (lane_cell comes from vh_integrate.hip,
// sample_nearest_block from vh_sample.hip, color_voxel / ColorPoints / color_release_kernel from vh_color.hip, the block list
// from vh_blocklist.hip).
//
// Labels are a third volume beside dp.blocks and the colour volume, one uint32 per voxel at the same index: label | votes << 16
// with label and votes both 1..65535; the word 0 is "no label".  Like the colour volume it is no member of DevPtrs: the pointer
// travels as a kernel argument of its own.  The rule is all integers.
//   label_integrate_kernel   color_integrate_kernel's launch shape: 256 lanes own one 8^3 block per pass, lane t voxels 2t and
//                            2t + 1; one 16-byte load of the TSDF pair (read only), one 8-byte load of the label pair, one
//                            2-byte gather per voxel from the label image, one 8-byte store when a word changed
//   (color_release_kernel    the label words of the blocks a deletion freed, zeroed: the colour launch with the label pointer)
//   label_points_kernel      one point per lane, the run-sharing look-up of color_points_kernel, nearest voxel only
//   label_counts_kernel      the listed blocks' valid voxels per label: equal lanes of a wave found with a ballot, one atomic
//                            per distinct label and wave, into a small LDS table first
//   label_remove_kernel      vh_remove_label: the voxels (and colour and label words) of one label cleared, the keys of the
//                            blocks that emptied listed for the deletion path (comp_remove_kernel's tail)
#pragma once

namespace vh {

// stats words of a vh_remove_label (unsigned long long each)
enum LabelWord : int { kLabelRemovedVoxels = 0, kLabelFreedBlocks, kLabelWords };

// One Boyer-Moore vote for the pixel's label of voxel (vx, vy, vz), cast on its word c = label | votes << 16; ow is the
// voxel's stored TSDF weight.  true: the word changed.  The camera point, the projection, the bounds test, the depth read and
// the band test are color_apply's (vh_color.hip), which has them from tsdf_apply (vh_integrate.hip): stated a third time so
// that the kernels of the TSDF update and of colour keep their code.
template <class Depth>
__device__ __forceinline__ bool label_apply(const FrameParams &fp, const Depth &src, const uint16_t *__restrict__ image, float band,
                                            uint32_t voteMax, int vx, int vy, int vz, float ow, uint32_t &c)
{
    if (!(ow > 0.0f)) {                     // a voxel that holds nothing has no label (also what a de-integration orphaned)
        const bool had = c != 0u;
        c = 0u;
        return had;
    }
    float cx, cy, cz;
    if (fp.semantics == VH_SEM_REFERENCE) {
        const float4 r = mat4_mul(fp.Tinv, (float)vx, (float)vy, (float)vz, 1.0f);
        cx = (float)f2i_rz(r.x) * fp.voxelSize;
        cy = (float)f2i_rz(r.y) * fp.voxelSize;
        cz = (float)f2i_rz(r.z) * fp.voxelSize;
    } else {
        const float4 r = mat4_mul(fp.Tinv, (float)vx * fp.voxelSize, (float)vy * fp.voxelSize, (float)vz * fp.voxelSize, 1.0f);
        cx = r.x; cy = r.y; cz = r.z;
    }
    int sx, sy;
    project(fp.proj, cx, cy, cz, sx, sy);
    if (sx < 0 || sx >= fp.width || sy < 0 || sy >= fp.height) return false;
    const float depth = src.at(sx, sy, fp.width);
    if (depth <= 0.0f) return false;
    const float s = depth - cz;             // no truncation: a label belongs to the surface
    if (!(__builtin_fabsf(s) <= band)) return false;
    if (voteMax == 0u) return false;        // the sweep only
    const uint32_t in = image[(size_t)sy * fp.width + sx];
    if (in == 0u) return false;             // a pixel the segmentation did not label
    const uint32_t l = c & 0xffffu, n = c >> 16;
    uint32_t out;
    if (n == 0u) out = in | (1u << 16);                         // fresh
    else if (l == in) out = l | (min(n + 1u, voteMax) << 16);   // one more vote, or held at the cap
    else if (n > 1u) out = l | ((n - 1u) << 16);                // one vote less
    else out = 0u;                                              // the last vote went: no label
    const bool changed = out != c;
    c = out;
    return changed;
}

// The fixed grid of the TSDF update over the dense compact list the step-level flatten left for `pose` (entries of allocated
// blocks only, so every e.ptr names a whole block inside dp.blocks and inside the label volume, which has a word per voxel).
template <class Depth>
__global__ __launch_bounds__(256) void label_integrate_kernel(const FrameParams fp, const DevPtrs dp, const Depth src,
                                                              uint32_t *__restrict__ labels, const uint16_t *__restrict__ image,
                                                              float band, uint32_t voteMax)
{
    const int count = dp.counters[kCompactCount];
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        const VoxelEntry e = dp.compact[k];
        const LaneCell cell = lane_cell(dp, e);
        const float4 v = *cell.cell;                                                        // {sdf0, w0, sdf1, w1}
        uint2 *words = reinterpret_cast<uint2 *>(labels + (size_t)e.ptr + 2 * threadIdx.x);
        uint2 c = *words;
        const bool u0 = label_apply(fp, src, image, band, voteMax, cell.bx, cell.by, cell.bz, v.y, c.x);
        const bool u1 = label_apply(fp, src, image, band, voteMax, cell.bx + 1, cell.by, cell.bz, v.w, c.y);
        if (u0 || u1) *words = c;
    }
}

// the word as a reader with `minVotes` (at least 1) sees it
__device__ __forceinline__ uint32_t label_read(uint32_t word, uint32_t minVotes) { return (word >> 16) >= minVotes ? word : 0u; }

// color_points_kernel's nearest half: lanes without a point stay in for the cross-lane reads of sample_nearest_block.
__global__ __launch_bounds__(256) void label_points_kernel(const FrameParams fp, const DevPtrs dp, const uint32_t *__restrict__ labels,
                                                           uint32_t minVotes, uint32_t n, const ColorPoints in,
                                                           uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    const bool have = at < n;
    const float nan = __builtin_nanf("");
    float u[3] = {nan, nan, nan};
    if (have) {
        if (in.toWorld) {
            const float4 p = reinterpret_cast<const float4 *>(in.points)[at];
            if (p.z != 0.0f) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    u[r] = (((in.T[4 * r + 0] * p.x + in.T[4 * r + 1] * p.y) + in.T[4 * r + 2] * p.z) + in.T[4 * r + 3]) / fp.voxelSize;
            }
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) u[a] = in.points[(size_t)at * 3u + a] / fp.voxelSize;
        }
    }
    const bool inDomain = __builtin_fabsf(u[0]) < kSampleDomain && __builtin_fabsf(u[1]) < kSampleDomain &&
                          __builtin_fabsf(u[2]) < kSampleDomain;          // false for NaN
    const SampleNearest near = sample_nearest_block(fp, dp, lane, u, inDomain);
    const uint32_t word = color_voxel(dp, labels, near.ptr, sample_index(near.r[0], near.r[1], near.r[2]));
    if (have) out[at] = label_read(word, minVotes);
}

__device__ __forceinline__ uint32_t label_list_count(const unsigned long long *numItems, uint32_t listCapacity)
{
    const unsigned long long n = *numItems;
    return n < (unsigned long long)listCapacity ? (uint32_t)n : listCapacity;
}

constexpr int kLabelSlots = 64;         // label_counts_kernel's LDS table: labels a workgroup sums before it touches memory

// One listed block per workgroup pass, lane t voxels 2t and 2t + 1.  A valid voxel's bin is its label where the reader sees one
// below numBins, else 0.  Labels are spatially coherent and 65 536 bins do not fit LDS, so a wave aggregates first: the first
// remaining lane's bin (readfirstlane), the ballot of the lanes that hold the same, its popcount added by one lane with one
// atomic; then the lanes that are left.  No atomic per voxel.  That one atomic goes to a small direct-mapped LDS table keyed
// by label where its slot is free or already the label's (the workgroup's sums reach memory once, at the end), straight to
// memory where another label holds the slot: a few workgroups adding to a few words of memory per block serialise there.
// Bin 0, the commonest, is summed in a register over all passes of the wave.  `labels` may be null (no volume: everything
// valid is bin 0).
__global__ __launch_bounds__(256) void label_counts_kernel(const DevPtrs dp, const uint32_t *__restrict__ labels,
                                                           const int4 *__restrict__ items,
                                                           const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                           uint32_t minVotes, uint32_t numBins, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t sKey[kLabelSlots], sSum[kLabelSlots], sZeros;     // key 0: a free slot (bin 0 never comes here)
    const uint32_t count = label_list_count(numItems, listCapacity);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < kLabelSlots) { sKey[threadIdx.x] = 0u; sSum[threadIdx.x] = 0u; }
    if (threadIdx.x == 0) sZeros = 0u;
    __syncthreads();
    uint32_t zeros = 0;                                                   // (wave-uniform)
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int ptr = items[b].w;
        const float4 v = reinterpret_cast<const float4 *>(dp.blocks + (size_t)ptr)[threadIdx.x];      // {sdf0, w0, sdf1, w1}
        uint2 c = make_uint2(0u, 0u);
        if (labels) c = reinterpret_cast<const uint2 *>(labels + (size_t)ptr)[threadIdx.x];
        const bool valid[2] = {v.y > 0.0f && v.x == v.x, v.w > 0.0f && v.z == v.z};
        const uint32_t word[2] = {label_read(c.x, minVotes), label_read(c.y, minVotes)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t l = word[h] & 0xffffu;
            const uint32_t bin = l < numBins ? l : 0u;
            zeros += (uint32_t)__popcll(__ballot(valid[h] && bin == 0u));
            bool left = valid[h] && bin != 0u;
            while (left) {                                                // (only the lanes still left are active in here)
                const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
                const unsigned long long same = __ballot(bin == first);  // (of the active lanes: the first is among them)
                if (bin == first) {
                    if (lane == (int)__builtin_ctzll(same)) {
                        const uint32_t slot = first & (uint32_t)(kLabelSlots - 1), n = (uint32_t)__popcll(same);
                        const uint32_t held = atomicCAS(sKey + slot, 0u, first);
                        if (held == 0u || held == first) atomicAdd(sSum + slot, n);
                        else atomicAdd(counts + first, n);
                    }
                    left = false;
                }
            }
        }
    }
    if (lane == 0 && zeros) atomicAdd(&sZeros, zeros);
    __syncthreads();
    if (threadIdx.x < kLabelSlots && sSum[threadIdx.x]) atomicAdd(counts + sKey[threadIdx.x], sSum[threadIdx.x]);
    if (threadIdx.x == 0 && sZeros) atomicAdd(counts, sZeros);
}

// Every voxel of a listed block whose word has `label` with at least minVotes votes becomes {0, 0} (a de-integrated voxel), its
// colour word (where there is a colour volume) and its label word 0.  A block in which this pass cleared a voxel and whose 512
// weights are then all 0 gives its key to the deletion path.
__global__ __launch_bounds__(256) void label_remove_kernel(const DevPtrs dp, uint32_t *__restrict__ color, uint32_t *__restrict__ labels,
                                                           const int4 *__restrict__ items,
                                                           const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                           uint32_t label, uint32_t minVotes, int4 *__restrict__ keys,
                                                           unsigned long long *__restrict__ words)
{
    const uint32_t count = label_list_count(numItems, listCapacity);
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        float4 *cell = reinterpret_cast<float4 *>(dp.blocks + (size_t)item.w) + threadIdx.x;
        uint2 *pair = reinterpret_cast<uint2 *>(labels + (size_t)item.w) + threadIdx.x;
        float4 v = *cell;                                                                   // {sdf0, w0, sdf1, w1}
        uint2 c = *pair;
        const bool d0 = (c.x & 0xffffu) == label && (c.x >> 16) >= minVotes;
        const bool d1 = (c.y & 0xffffu) == label && (c.y >> 16) >= minVotes;
        if (d0) { v.x = 0.0f; v.y = 0.0f; c.x = 0u; }
        if (d1) { v.z = 0.0f; v.w = 0.0f; c.y = 0u; }
        if (d0 || d1) {
            *cell = v;
            *pair = c;
            if (color) {
                uint2 *rgb = reinterpret_cast<uint2 *>(color + (size_t)item.w) + threadIdx.x;
                uint2 w = *rgb;
                if (d0) w.x = 0u;
                if (d1) w.y = 0u;
                *rgb = w;
            }
        }
        const int voxels = __syncthreads_count(d0) + __syncthreads_count(d1);
        const int empty = __syncthreads_and(v.y == 0.0f && v.w == 0.0f);
        if (threadIdx.x == 0 && voxels) {
            atomicAdd(words + kLabelRemovedVoxels, (unsigned long long)voxels);
            if (empty) keys[atomicAdd(words + kLabelFreedBlocks, 1ull)] = make_int4(item.x, item.y, item.z, 0);
        }
    }
}

}  // namespace vh
