"""The rule of vh_changes (include/voxelhash.h) in executable form: numpy, integers only.

A table is what SDFHashtable.hash_table() downloads (ENTRY records in entry order, ptr == -1 free; a shard's own entries), the
voxels what sdf_blocks() downloads, the colours color_volume() or None.  A state is State: the epoch and one SLOT per pool
block, indexed by ptr >> 9; State.tobytes() is the device buffer's content."""
import itertools

import numpy as np

U64 = np.uint64
SLOT = np.dtype([("key", "<i4", (3,)), ("live", "<u4"), ("h0", "<u8"), ("h1", "<u8")])
HEADER_BYTES = 64
VOXELS, COLOR = 1, 2
HALO_NONE, HALO_MESH, HALO_NORMALS = 0, 1, 2
SELF, HALO = 1, 2
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
G = 0x9e3779b97f4a7c15
MASK = (1 << 64) - 1


def mix(z):
    """The splitmix64 finaliser on a uint64 array (wrapping)."""
    z = np.asarray(z, U64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> U64(30)
        z *= U64(0xbf58476d1ce4e5b9)
        z ^= z >> U64(27)
        z *= U64(0x94d049bb133111eb)
        z ^= z >> U64(31)
    return z


def mix_int(z):
    """The same on a Python int: the arithmetic written a second way."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & MASK
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & MASK
    z ^= z >> 31
    return z


def terms(sdf_bits, weight_bits, colors, what):
    """(m [N], multiplier [N]) of a block: 512 voxel terms, then with COLOR 512 colour terms (colors None: all words 0)."""
    j = np.arange(512, dtype=U64)
    x = (np.asarray(weight_bits, np.uint32).astype(U64) << U64(32)) | np.asarray(sdf_bits, np.uint32).astype(U64)
    with np.errstate(over="ignore"):
        m = mix(x + (j + U64(1)) * U64(G) + U64(what))
        k = U64(2) * j + U64(1)
        if what & COLOR:
            c = np.zeros(512, U64) if colors is None else np.asarray(colors, np.uint32).astype(U64)
            m = np.concatenate([m, mix(c + (j + U64(513)) * U64(G) + U64(what))])
            k = np.concatenate([k, U64(2) * (j + U64(512)) + U64(1)])
    return m, k


def digest(sdf_bits, weight_bits, colors=None, what=VOXELS, order=None):
    """(h0, h1) as Python ints.  `order`: a permutation of the terms -- both are sums, so it must not matter."""
    m, k = terms(sdf_bits, weight_bits, colors, what)
    if order is not None:
        m, k = m[order], k[order]
    with np.errstate(over="ignore"):
        return int(np.add.reduce(m)), int(np.add.reduce(m * k))


def block_digest(voxels, colors, ptr, what):
    """The digest of the block at `ptr` of a downloaded voxel array (VOXEL records) and colour volume (or None)."""
    v = voxels[ptr:ptr + 512]
    c = None if colors is None else colors[ptr:ptr + 512]
    return digest(v["sdf"].view(np.uint32), v["weight"].view(np.uint32), c, what)


def halo_offsets(halo):
    """The offsets o != 0 with which k + o is a halo block of k."""
    rng = {HALO_NONE: (), HALO_MESH: (-1, 0), HALO_NORMALS: (-1, 0, 1)}[halo]
    return [o for o in itertools.product(rng, repeat=3) if o != (0, 0, 0)]


def halo_offsets_brute(halo):
    """The same from what a block's mesh reads: block j's cells read the blocks j + {0, 1}^3 (voxels 0..8 per axis); with
    normals the gradient at a voxel -1..9 per axis, so the blocks j + {-1, 0, 1}^3.  k is read by j = k - d."""
    if halo == HALO_NONE:
        return []
    reach = range(0, 9) if halo == HALO_MESH else range(-1, 10)
    blocks = sorted({v // 8 for v in reach})
    return [tuple(-d for d in o) for o in itertools.product(blocks, repeat=3) if o != (0, 0, 0)]


def grow(region):
    """The region grown by one block on every side, saturating (mesh_grow's rule on both ends)."""
    if region is None:
        region = ((INT32_MIN,) * 3, (INT32_MAX,) * 3)
    lo, hi = region
    return (tuple(v if v == INT32_MIN else v - 1 for v in lo), tuple(v if v == INT32_MAX else v + 1 for v in hi))


def holds(region, key):
    if region is None:
        region = ((INT32_MIN,) * 3, (INT32_MAX,) * 3)
    return all(lo <= k < hi for lo, hi, k in zip(region[0], region[1], key))


class State:
    def __init__(self, slots):
        self.epoch = 0
        self.slots = np.zeros(int(slots), SLOT)

    def copy(self):
        s = State(len(self.slots))
        s.epoch, s.slots = self.epoch, self.slots.copy()
        return s

    def tobytes(self):
        head = np.zeros(HEADER_BYTES // 8, U64)
        head[0] = self.epoch
        return head.tobytes() + self.slots.tobytes()

    @staticmethod
    def frombytes(raw):
        raw = bytes(raw)
        s = State((len(raw) - HEADER_BYTES) // SLOT.itemsize)
        head = np.frombuffer(raw, U64, HEADER_BYTES // 8)
        assert not head[1:].any()
        s.epoch = int(head[0])
        s.slots = np.frombuffer(raw, SLOT, len(s.slots), HEADER_BYTES).copy()
        return s


def changes(table, voxels, colors, state, region=None, what=VOXELS, halo=HALO_MESH, capacity_changed=None, capacity_removed=None):
    """One call of vh_changes: (changed int32 [n, 4], removed int32 [m, 4], committed).  `state` advances in place iff both
    counts fit (None: any count fits); otherwise it is left alone and the lists say what a call with room would write."""
    key_of = lambda e: tuple(int(c) for c in e["pos"])
    grown = grow(region)
    listed = [(i, key_of(e), int(e["ptr"])) for i, e in enumerate(table) if e["ptr"] != -1 and holds(grown, key_of(e))]
    held = {key_of(e): int(e["ptr"]) for e in table if e["ptr"] != -1}
    at = {k: n for n, (_, k, _) in enumerate(listed)}
    flags = [0] * len(listed)
    fresh = {}
    by_slot = {}
    for n, (_, k, ptr) in enumerate(listed):
        p = ptr >> 9
        by_slot[p] = k
        if not holds(region, k):
            continue
        h0, h1 = block_digest(voxels, colors, ptr, what)
        s = state.slots[p]
        if not (s["live"] and key_of({"pos": s["key"]}) == k and int(s["h0"]) == h0 and int(s["h1"]) == h1):
            flags[n] |= SELF
            fresh[p] = (k, h0, h1)
    stale, removed = [], []
    for p, s in enumerate(state.slots):
        k = tuple(int(c) for c in s["key"])
        if s["live"] and holds(region, k) and by_slot.get(p) != k:
            stale.append(p)
            if k not in held:
                removed.append(k)
    sources = [k for n, (_, k, _) in enumerate(listed) if flags[n] & SELF] + removed
    offsets = halo_offsets(halo)
    for k in sources:
        for o in offsets:
            n = at.get(tuple(a + b for a, b in zip(k, o)))
            if n is not None:
                flags[n] |= HALO
    changed = np.array([list(k) + [f] for (_, k, _), f in zip(listed, flags) if f], np.int32).reshape(-1, 4)
    gone = np.array([list(k) + [0] for k in removed], np.int32).reshape(-1, 4)
    fits = (capacity_changed is None or len(changed) <= capacity_changed) and (capacity_removed is None or len(gone) <= capacity_removed)
    if fits:
        for p in stale:
            state.slots[p] = np.zeros((), SLOT)
        for p, (k, h0, h1) in fresh.items():
            state.slots[p] = (k, 1, h0, h1)
        state.epoch += 1
    return changed, gone, fits
