// vh_changes.hip -- which blocks differ from what a caller-kept state last saw (vh_changes), and the two small kernels around
// mesh_block_kernel that mesh a list of keys block by block (vh_extract_mesh_blocks).  DESIGN.md 4.24; include/voxelhash.h
// states the rule, tests/changes_ref.py is its executable form.  Part of libvoxelhash_hip.so (gfx950); included by
// vh_kernels.hip after everything else: the list and its scans are vh_blocklist.hip's, the probe vh_raycast.hip's lookup_block.
//
// No model-changing kernel writes a dirty flag: the change set is computed afterwards, from a digest of each block's bits.
//   (vh_blocklist.hip          the ordered block list with the region grown by one block on every side as predicate)
//   changes_digest_kernel      one workgroup pass per listed block: listPos[ptr >> 9] = list position; for a block inside the
//                              region its 4 KiB (and 2 KiB of colour) read once, the digest, the comparison with the state slot
//   changes_stale_kernel       one lane per state slot: live, inside the region and not listed under that slot = stale; a stale
//                              key the table no longer holds = removed
//   changes_halo_kernel        one lane per self-changed block and per removed key: the allocated neighbours get the halo flag
//   changes_count_kernel       one lane per listed block: 1 if it carries a flag; block_scan_* over both count arrays
//   changes_commit_kernel      both totals fit: the two lists written at their scanned places, the state advanced; else nothing
#pragma once

namespace vh {

constexpr uint32_t kChangesColor = 2u;                         // VH_CHANGES_COLOR
constexpr uint32_t kChangedSelf = 1u, kChangedHalo = 2u;       // VH_CHANGED_SELF / VH_CHANGED_HALO
constexpr uint32_t kSlotStale = 1u, kSlotRemoved = 2u;
constexpr int kChangesHaloNone = 0, kChangesHaloMesh = 1, kChangesHaloNormals = 2;      // VH_CHANGES_HALO_*
constexpr unsigned long long kDigestG = 0x9e3779b97f4a7c15ull;

// one slot of the caller's state (32 bytes), indexed by ptr >> 9 behind a 64-byte header whose first word is the epoch
struct ChangesSlot {
    int32_t key[3];
    uint32_t live;
    unsigned long long h0, h1;
};
static_assert(sizeof(ChangesSlot) == 32, "the state's layout is part of the specification");
constexpr int kChangesHeaderBytes = 64;

// the splitmix64 finaliser: a bijection of the 64-bit words
__device__ __forceinline__ unsigned long long digest_mix(unsigned long long z)
{
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

// term j (0..511 the voxels, 512..1023 the colour words) of a block's digest
__device__ __forceinline__ void digest_term(unsigned long long x, uint32_t j, uint32_t what, unsigned long long &h0,
                                            unsigned long long &h1)
{
    const unsigned long long m = digest_mix(x + (unsigned long long)(j + 1u) * kDigestG + (unsigned long long)what);
    h0 += m;
    h1 += m * (unsigned long long)(2u * j + 1u);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}

__device__ __forceinline__ bool changes_same_key(const ChangesSlot &s, const int4 &it)
{
    return s.key[0] == it.x && s.key[1] == it.y && s.key[2] == it.z;
}

// One listed block per workgroup pass.  Lane t holds voxels 2t and 2t + 1 (one 16-byte load, the apron load of
// mesh_block_kernel) and, with the colour, their two colour words (one 8-byte load; zeros without a colour volume).  The sums are
// reduced in the wave by shuffles and across the four waves through eight LDS words; lane 0 compares with the state slot.
// flags[b] = kChangedSelf or 0; digest[2b], digest[2b + 1] = h0, h1 of a block inside the region (what the commit writes).
__global__ __launch_bounds__(256) void changes_digest_kernel(const DevPtrs dp, const uint32_t *__restrict__ color,
                                                             const BlockBox rg, uint32_t what, const int4 *__restrict__ items,
                                                             const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                             const ChangesSlot *__restrict__ slots, uint32_t numSlots,
                                                             uint32_t *__restrict__ listPos, uint32_t *__restrict__ flags,
                                                             unsigned long long *__restrict__ digest)
{
    __shared__ unsigned long long sSum[8];
    const uint32_t count = min((uint32_t)*numItems, listCapacity);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = blockIdx.x; b < count; b += gridDim.x) {
        const int4 item = items[b];
        const uint32_t p = (uint32_t)item.w >> 9;
        if (!rg.holds(item.x, item.y, item.z) || p >= numSlots) {      // (the apron of the list: a halo at most)
            if (tid == 0) {
                if (p < numSlots) listPos[p] = b;
                flags[b] = 0u;
            }
            continue;
        }
        const uint4 v = *reinterpret_cast<const uint4 *>(dp.blocks + (size_t)item.w + 2u * tid);
        unsigned long long h0 = 0, h1 = 0;
        digest_term(((unsigned long long)v.y << 32) | v.x, 2u * tid, what, h0, h1);
        digest_term(((unsigned long long)v.w << 32) | v.z, 2u * tid + 1u, what, h0, h1);
        if (what & kChangesColor) {
            uint2 c = make_uint2(0u, 0u);
            if (color) c = *reinterpret_cast<const uint2 *>(color + (size_t)item.w + 2u * tid);
            digest_term(c.x, 512u + 2u * tid, what, h0, h1);
            digest_term(c.y, 513u + 2u * tid, what, h0, h1);
        }
        h0 = wave_sum(h0);
        h1 = wave_sum(h1);
        if (lane == 0) { sSum[2 * wave] = h0; sSum[2 * wave + 1] = h1; }
        __syncthreads();
        if (tid == 0) {
            h0 = (sSum[0] + sSum[2]) + (sSum[4] + sSum[6]);
            h1 = (sSum[1] + sSum[3]) + (sSum[5] + sSum[7]);
            const ChangesSlot s = slots[p];
            const bool same = s.live != 0u && changes_same_key(s, item) && s.h0 == h0 && s.h1 == h1;
            listPos[p] = b;
            flags[b] = same ? 0u : kChangedSelf;
            digest[2 * (size_t)b] = h0;
            digest[2 * (size_t)b + 1] = h1;
        }
        __syncthreads();                          // (sSum is free for the next pass)
    }
}

// the list position of the block that holds pool slot p in this call's list, or ~0u (listPos keeps words of earlier calls)
__device__ __forceinline__ uint32_t changes_listed_at(const uint32_t *__restrict__ listPos, const int4 *__restrict__ items,
                                                      uint32_t count, uint32_t p)
{
    const uint32_t b = listPos[p];
    return b < count && ((uint32_t)items[b].w >> 9) == p ? b : ~0u;
}

// One lane per state slot: slotFlags[p] = kSlotStale (| kSlotRemoved), slotCount[p] = 1 for a removed key.
__global__ __launch_bounds__(256) void changes_stale_kernel(const FrameParams fp, const DevPtrs dp, const BlockBox rg,
                                                            const int4 *__restrict__ items,
                                                            const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                            const ChangesSlot *__restrict__ slots, uint32_t numSlots,
                                                            const uint32_t *__restrict__ listPos, uint32_t *__restrict__ slotFlags,
                                                            uint32_t *__restrict__ slotCount)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= numSlots) return;
    const uint32_t count = min((uint32_t)*numItems, listCapacity);
    const ChangesSlot s = slots[p];
    uint32_t f = 0;
    if (s.live != 0u && rg.holds(s.key[0], s.key[1], s.key[2])) {
        const uint32_t b = changes_listed_at(listPos, items, count, p);
        if (b == ~0u || !changes_same_key(s, items[b])) {
            f = kSlotStale;
            if (lookup_block(fp, dp, s.key[0], s.key[1], s.key[2]) == VH_FREE_BLOCK) f |= kSlotRemoved;
        }
    }
    slotFlags[p] = f;
    slotCount[p] = (f & kSlotRemoved) ? 1u : 0u;
}

// One lane per listed block (i < listCapacity) and per state slot (behind): around a self-changed block's key or a removed key
// k, the allocated blocks k + o, o != 0, get the halo flag.  MESH: o in {-1, 0}^3 (block j reads j + {0, 1}^3); NORMALS: o in
// {-1, 0, 1}^3.  A neighbour lies inside the grown region, so it is listed; a block of another shard is absent.
__global__ __launch_bounds__(256) void changes_halo_kernel(const FrameParams fp, const DevPtrs dp, int halo,
                                                           const int4 *__restrict__ items,
                                                           const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                           const ChangesSlot *__restrict__ slots, uint32_t numSlots,
                                                           const uint32_t *__restrict__ listPos, const uint32_t *__restrict__ slotFlags,
                                                           uint32_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t count = min((uint32_t)*numItems, listCapacity);
    int kx, ky, kz;
    if (i < listCapacity) {
        if (i >= count || !(flags[i] & kChangedSelf)) return;
        const int4 it = items[i];
        kx = it.x; ky = it.y; kz = it.z;
    } else {
        const uint32_t p = i - listCapacity;
        if (p >= numSlots || !(slotFlags[p] & kSlotRemoved)) return;
        const ChangesSlot s = slots[p];
        kx = s.key[0]; ky = s.key[1]; kz = s.key[2];
    }
    const int hi = halo == kChangesHaloNormals ? 1 : 0;
    for (int oz = -1; oz <= hi; ++oz)
        for (int oy = -1; oy <= hi; ++oy)
            for (int ox = -1; ox <= hi; ++ox) {
                if (ox == 0 && oy == 0 && oz == 0) continue;
                // (wrapping: a key at the end of int32 has no neighbour there that a table of the key domain could hold)
                const int nx = (int)((uint32_t)kx + (uint32_t)ox), ny = (int)((uint32_t)ky + (uint32_t)oy),
                          nz = (int)((uint32_t)kz + (uint32_t)oz);
                const int ptr = lookup_block(fp, dp, nx, ny, nz);
                if (ptr == VH_FREE_BLOCK) continue;
                const uint32_t p = (uint32_t)ptr >> 9;
                if (p >= numSlots) continue;
                const uint32_t b = changes_listed_at(listPos, items, count, p);
                if (b != ~0u) atomicOr(flags + b, kChangedHalo);
            }
}

__global__ __launch_bounds__(256) void changes_count_kernel(const unsigned long long *__restrict__ numItems, uint32_t listCapacity,
                                                            const uint32_t *__restrict__ flags, uint32_t *__restrict__ changedCount)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < min((uint32_t)*numItems, listCapacity)) changedCount[b] = flags[b] ? 1u : 0u;
}

// result = {listed, changed, removed}.  Both totals within their capacities: lane i < listCapacity writes its block's record at
// its scanned place, lane listCapacity + p writes slot p's removed key and advances state slot p (the block listed under p, if
// self-changed, takes the slot; else a stale slot is emptied), and one lane counts the epoch up.  Otherwise nothing is written.
__global__ __launch_bounds__(256) void changes_commit_kernel(const BlockBox rg, const int4 *__restrict__ items,
                                                             const unsigned long long *__restrict__ result, uint32_t listCapacity,
                                                             ChangesSlot *__restrict__ slots, uint32_t numSlots,
                                                             unsigned long long *__restrict__ epoch,
                                                             const uint32_t *__restrict__ listPos, const uint32_t *__restrict__ flags,
                                                             const unsigned long long *__restrict__ digest,
                                                             const uint32_t *__restrict__ changedCount,
                                                             const unsigned long long *__restrict__ changedTiles,
                                                             const uint32_t *__restrict__ slotFlags,
                                                             const uint32_t *__restrict__ slotCount,
                                                             const unsigned long long *__restrict__ slotTiles,
                                                             unsigned long long capacityChanged, int4 *__restrict__ changed,
                                                             unsigned long long capacityRemoved, int4 *__restrict__ removed)
{
    if (result[1] > capacityChanged || result[2] > capacityRemoved) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t count = min((uint32_t)result[0], listCapacity);
    if (i == 0) *epoch += 1ull;
    if (i < listCapacity) {
        if (i >= count || !flags[i]) return;
        const int4 it = items[i];
        changed[scanned_at(changedTiles, changedCount, i)] = make_int4(it.x, it.y, it.z, (int)flags[i]);
        return;
    }
    const uint32_t p = i - listCapacity;
    if (p >= numSlots) return;
    const uint32_t f = slotFlags[p];
    if (f & kSlotRemoved) {
        const ChangesSlot s = slots[p];
        removed[scanned_at(slotTiles, slotCount, p)] = make_int4(s.key[0], s.key[1], s.key[2], 0);
    }
    const uint32_t b = changes_listed_at(listPos, items, count, p);
    if (b != ~0u && (flags[b] & kChangedSelf)) {
        const int4 it = items[b];
        ChangesSlot s;
        s.key[0] = it.x; s.key[1] = it.y; s.key[2] = it.z;
        s.live = 1u;
        s.h0 = digest[2 * (size_t)b];
        s.h1 = digest[2 * (size_t)b + 1];
        slots[p] = s;
    } else if (f & kSlotStale) {
        ChangesSlot s;
        s.key[0] = s.key[1] = s.key[2] = 0;
        s.live = 0u;
        s.h0 = s.h1 = 0ull;
        slots[p] = s;
    }
}

// ---------------------------------------------------------------------------
// vh_extract_mesh_blocks: a list of keys in front of mesh_block_kernel, the per-key offsets behind it
// ---------------------------------------------------------------------------
// One lane per key: keyPtr[i] = its block through the probe (VH_FREE_BLOCK: absent), keyCount[i] = 1 if present.
__global__ __launch_bounds__(256) void mesh_keys_resolve_kernel(const FrameParams fp, const DevPtrs dp, const int4 *__restrict__ keys,
                                                                uint32_t n, int32_t *__restrict__ keyPtr,
                                                                uint32_t *__restrict__ keyCount)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int4 k = keys[i];
    const int ptr = lookup_block(fp, dp, k.x, k.y, k.z);
    keyPtr[i] = ptr;
    keyCount[i] = ptr != VH_FREE_BLOCK ? 1u : 0u;
}

// the present keys as the item list {x, y, z, ptr}, in the keys' order (keyCount holds the scanned places): an absent key is no
// item, so mesh_block_kernel never sees one
__global__ __launch_bounds__(256) void mesh_keys_items_kernel(const int4 *__restrict__ keys, uint32_t n,
                                                              const int32_t *__restrict__ keyPtr, const uint32_t *__restrict__ keyCount,
                                                              const unsigned long long *__restrict__ keyTiles, int4 *__restrict__ items,
                                                              uint32_t listCapacity)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || keyPtr[i] == VH_FREE_BLOCK) return;
    const unsigned long long at = scanned_at(keyTiles, keyCount, i);
    if (at < listCapacity) items[at] = make_int4(keys[i].x, keys[i].y, keys[i].z, keyPtr[i]);
}

// first[i], i <= n: the triangles before key i's = the scanned offset of the item the key became (an absent key: of the next
// present one); first[n] = the total.  result = {items, triangles}.
__global__ __launch_bounds__(256) void mesh_keys_first_kernel(uint32_t n, const uint32_t *__restrict__ keyCount,
                                                              const unsigned long long *__restrict__ keyTiles,
                                                              const uint32_t *__restrict__ blockCount,
                                                              const unsigned long long *__restrict__ blockTiles,
                                                              const unsigned long long *__restrict__ result,
                                                              unsigned long long *__restrict__ first)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    const unsigned long long at = i < n ? scanned_at(keyTiles, keyCount, i) : result[0];
    first[i] = at < result[0] ? scanned_at(blockTiles, blockCount, (uint32_t)at) : result[1];
}

}  // namespace vh
