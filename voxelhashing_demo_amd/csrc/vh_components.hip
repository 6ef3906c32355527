// vh_components.hip -- connected pieces of the fused model: vh_components, vh_remove_components.
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_sample.hip (block list and scans: vh_blocklist.hip,
// lookup_block: vh_raycast.hip, sample_judge / LatticeBox: vh_sample.hip).
//
// The rule (include/voxelhash.h, tests/components_ref.py) is in integers: a node is a valid voxel of the target class in a
// listed block, its id is rank * 512 + voxel index (rank = position of its block in the mesh's ordered block list), an edge
// joins A and A + o for o in the three axis units (connectivity 6) or in {0,1}^3 \ {0} (14), a component's root is its node
// of least id.  A union-find whose parent never grows: parent[id] <= id always, a non-root's parent is strictly less.
//   (vh_blocklist.hip      the ordered block list with the region, a BlockBox, as predicate)
//   comp_local_kernel      one workgroup pass per listed block: classify the 512 voxels, unite the pairs inside the block
//                          in LDS, parent[id] = least node of the block's own component (none: VH_COMPONENT_NONE);
//                          rank[ptr >> 9] = list position
//   comp_seam_kernel       one workgroup pass per listed block: the pairs (A, A + o) with A + o in one of the seven
//                          +neighbour blocks, united in global memory with atomicMin on the larger root
//   comp_flatten_kernel    parent[id] = root for every node; one bit per root, roots per block
//   comp_count_kernel      nodes per root: summed per workgroup in an LDS table keyed by root, then one integer atomic per
//                          root the block saw, added onto the root's own parent word (so parent[root] = root + size)
//   (block_scan_*          exclusive scan of the roots per block: a root's component index)
//   comp_records_kernel    the records in root order; the largest size
//   comp_labels_kernel     a box of the lattice: sample_lattice_kernel's brick pass, the component index per voxel
//   comp_remove_kernel     vh_remove_components: the voxels (and colour words) of the small components cleared, the keys of
//                          the blocks that emptied listed for the deletion path
// No loop waits for another workgroup.  The only words workgroups share inside a launch are parent[] in comp_seam_kernel and
// comp_flatten_kernel (every access an agent-scope relaxed atomic: a stale parent is an older ancestor, still of the same
// component and still less than its child, which the algorithm tolerates; a cached or torn one it would not) and the integer
// sums of comp_count_kernel and of the stats.
#pragma once

namespace vh {

constexpr uint32_t kCompNone = 0xFFFFFFFFu;                 // VH_COMPONENT_NONE
constexpr uint32_t kCompMaxBlocks = (1u << 23) - 1u;        // ids fit a uint32 with kCompNone to spare
constexpr int kCompHashSlots = 1024;                        // comp_count_kernel's LDS table: at most 512 keys per block

// stats words of a call (unsigned long long each)
enum CompWord : int { kCompNodes = 0, kCompLargest, kCompRemovedComponents, kCompRemovedVoxels, kCompFreedBlocks, kCompWords };

// target class of a valid voxel (mesh rule: inside iff sdf <= 0, so -0.0, +0.0 and -inf are inside)
__device__ __forceinline__ bool comp_is_node(float sdf, float weight, int target)
{
    const bool valid = weight > 0.0f && sdf == sdf;
    return valid && ((sdf <= 0.0f) == (target == VH_COMPONENT_INSIDE));
}

// ---- the union-find, on LDS (workgroup scope) or on global memory (agent scope) ----
template <int kScope>
__device__ __forceinline__ uint32_t comp_find(uint32_t *parent, uint32_t x)
{
    for (;;) {                                   // ends: every step goes to a strictly smaller id
        const uint32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, kScope);
        if (p == x) return x;
        x = p;
    }
}

// After it a and b have one root.  The larger of the two roots is hung below the smaller with atomicMin; if that word had
// changed meanwhile (the "root" was one no more, or the load was stale) the walk goes on from the value it held.
template <int kScope>
__device__ __forceinline__ void comp_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = comp_find<kScope>(parent, a);
        b = comp_find<kScope>(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }               // a > b
        const uint32_t old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, kScope);
        if (old == a) return;                    // a was a root and now hangs below b
        a = old;                                 // a's former parent (< a) still has to meet b
    }
}

__device__ __forceinline__ uint32_t comp_count(const unsigned long long *numItems, uint32_t listCapacity)
{
    const unsigned long long n = *numItems;
    return n > (unsigned long long)kCompMaxBlocks ? 0u : min((uint32_t)n, listCapacity);      // beyond the limit nothing is written
}

// Lane t holds voxels t and t + 256 of the block (8-byte loads, a wave reads 512 contiguous bytes).
__global__ __launch_bounds__(256) void comp_local_kernel(const DevPtrs dp, const int4 *__restrict__ items,
                                                         const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                         int target, int connectivity, uint32_t *__restrict__ parent,
                                                         uint32_t *__restrict__ rank, uint32_t rankSize)
{
    __shared__ uint32_t sParent[kBlockVoxels];
    const uint32_t count = comp_count(numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = tid + 256 * h;
            const Voxel vox = dp.blocks[(size_t)item.w + (size_t)v];
            sParent[v] = comp_is_node(vox.sdf, vox.weight, target) ? (uint32_t)v : kCompNone;
        }
        if (tid == 0 && ((uint32_t)item.w >> 9) < rankSize) rank[(uint32_t)item.w >> 9] = b;
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = tid + 256 * h;
            if (__hip_atomic_load(sParent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == kCompNone) continue;      // (node or not never changes)
            const int x = v & 7, y = (v >> 3) & 7, z = v >> 6;
            for (int o = 1; o < 8; ++o) {
                if (connectivity == 6 && (o & (o - 1))) continue;        // axis units only: 1, 2, 4
                const int nx = x + (o & 1), ny = y + ((o >> 1) & 1), nz = z + (o >> 2);
                if ((nx | ny | nz) & 8) continue;                        // across a seam: comp_seam_kernel
                const int u = (nz << 6) | (ny << 3) | nx;
                if (__hip_atomic_load(sParent + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == kCompNone) continue;
                comp_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(sParent, (uint32_t)v, (uint32_t)u);
            }
        }
        __syncthreads();
        uint32_t root[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = tid + 256 * h;
            root[h] = sParent[v] == kCompNone ? kCompNone : b * 512u + comp_find<__HIP_MEMORY_SCOPE_WORKGROUP>(sParent, (uint32_t)v);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) parent[(size_t)b * 512u + tid + 256 * h] = root[h];
        __syncthreads();                          // (sParent is free for the next pass)
    }
}

__global__ __launch_bounds__(256) void comp_seam_kernel(const FrameParams fp, const DevPtrs dp, const int4 *__restrict__ items,
                                                        const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                        int connectivity, uint32_t *parent, const uint32_t *__restrict__ rank,
                                                        uint32_t rankSize)
{
    __shared__ uint32_t sNb[8];                   // list position of the block at offset (o & 1, o >> 1 & 1, o >> 2); none: kCompNone
    const uint32_t count = comp_count(numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        if (tid < 8) {
            uint32_t r = kCompNone;
            if (tid > 0 && (connectivity == 14 || !(tid & (tid - 1)))) {
                const int p = lookup_block(fp, dp, item.x + (tid & 1), item.y + ((tid >> 1) & 1), item.z + (tid >> 2));
                if (p != VH_FREE_BLOCK && ((uint32_t)p >> 9) < rankSize) r = rank[(uint32_t)p >> 9];      // (not listed: kCompNone)
                if (r >= count) r = kCompNone;
            }
            sNb[tid] = r;
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = tid + 256 * h;
            const int x = v & 7, y = (v >> 3) & 7, z = v >> 6;
            if (x != 7 && y != 7 && z != 7) continue;                    // no pair of this voxel crosses a seam
            const uint32_t a = b * 512u + (uint32_t)v;
            if (__hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kCompNone) continue;
            for (int o = 1; o < 8; ++o) {
                if (connectivity == 6 && (o & (o - 1))) continue;
                const int nx = x + (o & 1), ny = y + ((o >> 1) & 1), nz = z + (o >> 2);
                const int cross = (nx >> 3) | ((ny >> 3) << 1) | ((nz >> 3) << 2);
                if (cross == 0) continue;                                // inside the block: comp_local_kernel
                const uint32_t nb = sNb[cross];
                if (nb == kCompNone) continue;                           // absent, another shard's, or outside the region: a cut
                const uint32_t u = nb * 512u + (uint32_t)(((nz & 7) << 6) | ((ny & 7) << 3) | (nx & 7));
                if (__hip_atomic_load(parent + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kCompNone) continue;
                comp_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, a, u);
            }
        }
        __syncthreads();                          // (sNb is free for the next pass)
    }
}

// rootBits[b * 8 + w]: bit i = voxel w * 64 + i of block b is a root.  rootCount[b] = roots of the block.
__global__ __launch_bounds__(256) void comp_flatten_kernel(const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                           uint32_t *parent, unsigned long long *__restrict__ rootBits,
                                                           uint32_t *__restrict__ rootCount)
{
    __shared__ uint32_t sRoots[4];
    const uint32_t count = comp_count(numItems, listCapacity);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        uint32_t roots = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t id = b * 512u + (uint32_t)(tid + 256 * h);
            const uint32_t p = __hip_atomic_load(parent + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool isRoot = false;
            if (p != kCompNone) {
                const uint32_t r = comp_find<__HIP_MEMORY_SCOPE_AGENT>(parent, id);
                isRoot = r == id;                 // (a root stays one in this launch: nothing unites any more)
                if (r != p) __hip_atomic_store(parent + id, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const unsigned long long bits = __ballot(isRoot);
            if (lane == 0) rootBits[(size_t)b * 8u + (uint32_t)(4 * h + wave)] = bits;
            roots += (uint32_t)__popcll(bits);
        }
        if (lane == 0) sRoots[wave] = roots;
        __syncthreads();
        if (tid == 0) rootCount[b] = sRoots[0] + sRoots[1] + sRoots[2] + sRoots[3];
        __syncthreads();
    }
}

__device__ __forceinline__ bool comp_root_bit(const unsigned long long *__restrict__ rootBits, uint32_t id)
{
    return (rootBits[(size_t)(id >> 9) * 8u + ((id >> 6) & 7u)] >> (id & 63u)) & 1ull;
}

// position of root `id` among all roots: the scanned roots per block, plus the roots before it in its block
__device__ __forceinline__ unsigned long long comp_index(const unsigned long long *__restrict__ rootBits,
                                                         const uint32_t *__restrict__ rootOffset,
                                                         const unsigned long long *__restrict__ rootTiles, uint32_t id)
{
    const uint32_t b = id >> 9, v = id & 511u;
    const unsigned long long *bits = rootBits + (size_t)b * 8u;
    uint32_t before = 0;
    for (uint32_t w = 0; w < (v >> 6); ++w) before += (uint32_t)__popcll(bits[w]);
    before += (uint32_t)__popcll(bits[v >> 6] & ((1ull << (v & 63u)) - 1ull));
    return scanned_at(rootTiles, rootOffset, b) + before;
}

// Sizes.  A root's word is read by nobody in this launch (its block knows it as a root from rootBits), every other node's word
// holds its root and does not change: the sums go onto the roots' words, parent[root] = root + size (below 2^32 - 512).
__global__ __launch_bounds__(256) void comp_count_kernel(const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                         uint32_t *parent, const unsigned long long *__restrict__ rootBits,
                                                         unsigned long long *__restrict__ words)
{
    __shared__ uint32_t sKey[kCompHashSlots], sSum[kCompHashSlots];
    const uint32_t count = comp_count(numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        for (int s = tid; s < kCompHashSlots; s += 256) { sKey[s] = kCompNone; sSum[s] = 0u; }
        __syncthreads();
        int nodes = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t id = b * 512u + (uint32_t)(tid + 256 * h);
            const uint32_t key = comp_root_bit(rootBits, id) ? id : parent[id];
            if (key == kCompNone) continue;
            ++nodes;
            uint32_t s = (key * 2654435761u) >> 22;
            for (;;) {                            // (ends: 512 keys at most in 1024 slots)
                const uint32_t old = atomicCAS(sKey + s, kCompNone, key);
                if (old == kCompNone || old == key) break;
                s = (s + 1u) & (uint32_t)(kCompHashSlots - 1);
            }
            atomicAdd(sSum + s, 1u);
        }
        __syncthreads();
        for (int s = tid; s < kCompHashSlots; s += 256)
            if (sKey[s] != kCompNone) atomicAdd(parent + sKey[s], sSum[s]);
        unsigned long long mine = (unsigned long long)nodes;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) mine += __shfl_xor(mine, d);
        if ((tid & 63) == 0 && mine) atomicAdd(words + kCompNodes, mine);
        __syncthreads();
    }
}

struct CompRecord { int32_t voxel[3]; uint32_t size; };                  // vh_component

__global__ __launch_bounds__(256) void comp_records_kernel(const int4 *__restrict__ items,
                                                           const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                           const uint32_t *__restrict__ parent,
                                                           const unsigned long long *__restrict__ rootBits,
                                                           const uint32_t *__restrict__ rootOffset,
                                                           const unsigned long long *__restrict__ rootTiles,
                                                           unsigned long long capacity, CompRecord *__restrict__ records,
                                                           unsigned long long *__restrict__ words)
{
    const uint32_t count = comp_count(numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        uint32_t largest = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = tid + 256 * h;
            const uint32_t id = b * 512u + (uint32_t)v;
            if (!comp_root_bit(rootBits, id)) continue;
            const uint32_t size = parent[id] - id;
            largest = max(largest, size);
            const unsigned long long at = comp_index(rootBits, rootOffset, rootTiles, id);
            if (at >= capacity) continue;
            CompRecord r;
            r.voxel[0] = (int)((uint32_t)item.x * 8u) + (v & 7);
            r.voxel[1] = (int)((uint32_t)item.y * 8u) + ((v >> 3) & 7);
            r.voxel[2] = (int)((uint32_t)item.z * 8u) + (v >> 6);
            r.size = size;
            records[at] = r;
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) largest = max(largest, (uint32_t)__shfl_xor(largest, d));
        if ((tid & 63) == 0 && largest) atomicMax(words + kCompLargest, (unsigned long long)largest);
    }
}

// sample_lattice_kernel's brick pass: lane t holds voxels 2t and 2t + 1 of the brick
__global__ __launch_bounds__(256) void comp_labels_kernel(const FrameParams fp, const DevPtrs dp, const LatticeBox box,
                                                          unsigned long long numBricks,
                                                          const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                          const uint32_t *__restrict__ parent,
                                                          const unsigned long long *__restrict__ rootBits,
                                                          const uint32_t *__restrict__ rootOffset,
                                                          const unsigned long long *__restrict__ rootTiles,
                                                          const uint32_t *__restrict__ rank, uint32_t rankSize,
                                                          uint32_t *__restrict__ labels)
{
    __shared__ uint32_t sRank;
    const uint32_t count = comp_count(numItems, listCapacity);
    if (*numItems > (unsigned long long)kCompMaxBlocks) return;           // beyond the limit nothing is written
    const int x = (threadIdx.x & 3) * 2, y = (threadIdx.x >> 2) & 7, z = threadIdx.x >> 5;
    for (unsigned long long b = blockIdx.x; b < numBricks; b += gridDim.x) {
        const unsigned long long row = b / (unsigned long long)box.bricks[0];
        const int bx = box.brick0[0] + (int)(b - row * (unsigned long long)box.bricks[0]);
        const int by = box.brick0[1] + (int)(row % (unsigned long long)box.bricks[1]);
        const int bz = box.brick0[2] + (int)(row / (unsigned long long)box.bricks[1]);
        __syncthreads();                            // (the pass before has read sRank)
        if (threadIdx.x == 0) {
            const int p = lookup_block(fp, dp, bx, by, bz);
            uint32_t r = kCompNone;
            if (p != VH_FREE_BLOCK && ((uint32_t)p >> 9) < rankSize) r = rank[(uint32_t)p >> 9];
            sRank = r < count ? r : kCompNone;
        }
        __syncthreads();
        const uint32_t r = sRank;
        const long long i = (long long)bx * 8 + x - box.lo[0], j = (long long)by * 8 + y - box.lo[1],
                        k = (long long)bz * 8 + z - box.lo[2];
        if (j < 0 || j >= box.dims[1] || k < 0 || k >= box.dims[2]) continue;
        const size_t rowAt = ((size_t)k * (size_t)box.dims[1] + (size_t)j) * (size_t)box.dims[0];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (i + e < 0 || i + e >= box.dims[0]) continue;
            uint32_t label = kCompNone;
            if (r != kCompNone) {
                const uint32_t id = r * 512u + (uint32_t)sample_index(x + e, y, z);
                const uint32_t root = comp_root_bit(rootBits, id) ? id : parent[id];
                if (root != kCompNone) label = (uint32_t)comp_index(rootBits, rootOffset, rootTiles, root);
            }
            labels[rowAt + (size_t)(i + e)] = label;
        }
    }
}

// Every node of a component with size < minSize becomes {0, 0} (a de-integrated voxel), its colour word 0.  A block in which
// this pass cleared a voxel and whose 512 weights are then all 0 gives its key to the deletion path.
__global__ __launch_bounds__(256) void comp_remove_kernel(const DevPtrs dp, uint32_t *__restrict__ color,
                                                          const int4 *__restrict__ items,
                                                          const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                          const uint32_t *__restrict__ parent,
                                                          const unsigned long long *__restrict__ rootBits,
                                                          unsigned long long minSize, int4 *__restrict__ keys,
                                                          unsigned long long *__restrict__ words)
{
    const uint32_t count = comp_count(numItems, listCapacity);
    const int tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        bool doomed[2], doomedRoot[2], zero[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = tid + 256 * h;
            const uint32_t id = b * 512u + (uint32_t)v;
            const bool isRoot = comp_root_bit(rootBits, id);
            const uint32_t p = parent[id];
            uint32_t size = 0;
            if (isRoot) size = p - id;
            else if (p != kCompNone) size = parent[p] - p;
            doomed[h] = (isRoot || p != kCompNone) && (unsigned long long)size < minSize;
            doomedRoot[h] = doomed[h] && isRoot;
            Voxel *vox = dp.blocks + (size_t)item.w + (size_t)v;
            if (doomed[h]) {
                Voxel none;
                none.sdf = 0.0f;
                none.weight = 0.0f;
                *vox = none;
                if (color) color[(size_t)item.w + (size_t)v] = 0u;
                zero[h] = true;
            } else {
                zero[h] = vox->weight == 0.0f;
            }
        }
        const int voxels = __syncthreads_count(doomed[0]) + __syncthreads_count(doomed[1]);
        const int comps = __syncthreads_count(doomedRoot[0]) + __syncthreads_count(doomedRoot[1]);
        const int empty = __syncthreads_and(zero[0] && zero[1]);
        if (tid == 0 && voxels) {
            atomicAdd(words + kCompRemovedVoxels, (unsigned long long)voxels);
            if (comps) atomicAdd(words + kCompRemovedComponents, (unsigned long long)comps);
            if (empty) keys[atomicAdd(words + kCompFreedBlocks, 1ull)] = make_int4(item.x, item.y, item.z, 0);
        }
    }
}

}  // namespace vh
