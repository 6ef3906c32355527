"""Chosen voxel models for the tests of vh_extract_mesh, and the ways to put one into a context.

A model is {block key (x, y, z): (sdf[512] float32, weight[512] float32)}, voxel index ((z&7)<<6)|((y&7)<<3)|(x&7).  Every
builder is seeded and pure numpy; nothing is read from disk.  A model enters a context as a snapshot file (write_snapshot,
the format of vh_save_snapshot) or as the records of a view table (view_records).  The rest of the module computes, from a
model alone and independently of tests/mesh_ref.py, the facts the tests' conditions are about (dense arrays, cell masks,
the edges of the emitted vertices), so that a test can say why it cannot pass vacuously."""
import itertools
import os

import numpy as np

import mesh_ref

F = np.float32
ENTRY = np.dtype([("pos", "<i4", (3,)), ("ptr", "<i4"), ("offset", "<i4")])
VOXEL = np.dtype([("sdf", "<f4"), ("weight", "<f4")])
RECORD_BYTES, RECORD_VOXELS = 4112, 514            # vh_view_record: 16 bytes of header, 512 voxels
HEADER_BYTES = 280                                 # SnapshotHeader (checked against the file an empty context saves)
HEAP_COUNTER_AT, NUM_ALLOCATED_AT = 204, 232       # int32 heapCounter, uint64 numAllocated inside the header
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


# ---------------------------------------------------------------------------------------------------------------------
# placement: the hash of the table, entries in the bucket of their key
# ---------------------------------------------------------------------------------------------------------------------
def hash_block(keys, num_buckets):
    """Bucket of each key [N, 3]: the unsigned 32-bit xor of the three products, modulo the bucket count."""
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    h = ((k[:, 0] * 73856093) ^ (k[:, 1] * 19349669) ^ (k[:, 2] * 83492791)) & 0xFFFFFFFF
    return h % int(num_buckets)


def model_arrays(model):
    """(keys [N, 3] int64, voxels [N, 512] VOXEL) in the dictionary's order."""
    keys = np.array(list(model.keys()), np.int64).reshape(-1, 3)
    vox = np.zeros((len(model), 512), VOXEL)
    for i, (s, w) in enumerate(model.values()):
        vox["sdf"][i] = s
        vox["weight"][i] = w
    return keys, vox


def place(model, num_buckets, bucket_size, pool, seed=0):
    """The model as a table would hold it: (table [num_buckets * bucket_size] ENTRY, heap [pool] uint32, heap counter,
    voxels [pool * 512] VOXEL).  Every entry sits in the bucket its key hashes to, in the bucket's first free slots, offset
    0; block ids are handed out in a seeded random order; the free list is the ids not handed out."""
    keys, vox = model_arrays(model)
    n = len(keys)
    assert n <= pool, f"{n} blocks do not fit a pool of {pool}"
    bucket = hash_block(keys, num_buckets)
    order = np.argsort(bucket, kind="stable")
    sb = bucket[order]
    slot = np.arange(n) - np.searchsorted(sb, sb, side="left")              # rank inside the bucket
    assert n == 0 or slot.max() < bucket_size, \
        f"a bucket of the crafted key set needs {slot.max() + 1} slots, bucketSize is {bucket_size}: choose more buckets"
    ids = np.random.RandomState(seed).permutation(pool)
    table = np.zeros(num_buckets * bucket_size, ENTRY)
    table["ptr"] = -1
    at = sb * bucket_size + slot
    table["pos"][at] = keys[order]
    table["ptr"][at] = ids[:n] * 512
    heap = np.concatenate([ids[n:], ids[:n]]).astype(np.uint32)             # free ids first: heap[0 .. counter]
    voxels = np.zeros(pool * 512, VOXEL)
    voxels.reshape(pool, 512)[ids[:n]] = vox[order]
    return table, heap, pool - n - 1, voxels


def snapshot_parts(empty, model, seed=0):
    """The pieces of a VHSNAP01 file that holds `model`, from the bytes of the snapshot an EMPTY context of the same
    parameters saved: (header, table, heap, payload [allocated, 512] VOXEL in table order).  Only heapCounter and
    numAllocated of the header are patched; the free entries keep whatever the library writes into them."""
    assert empty[:8] == b"VHSNAP01"
    num_entries = int(np.frombuffer(empty, "<u8", 1, NUM_ALLOCATED_AT - 8)[0])
    num_buckets, bucket_size, _, pool = (int(v) for v in np.frombuffer(empty, "<u4", 4, 8 + 128))
    assert num_entries == num_buckets * bucket_size
    assert len(empty) == HEADER_BYTES + num_entries * ENTRY.itemsize + pool * 4, "not the snapshot of an empty context"
    assert int(np.frombuffer(empty, "<i4", 1, HEAP_COUNTER_AT)[0]) == pool - 1
    assert int(np.frombuffer(empty, "<u8", 1, NUM_ALLOCATED_AT)[0]) == 0
    table = np.frombuffer(empty, ENTRY, num_entries, HEADER_BYTES).copy()
    assert (table["ptr"] == -1).all()
    placed, heap, counter, voxels = place(model, num_buckets, bucket_size, pool, seed)
    used = placed["ptr"] != -1
    table[used] = placed[used]
    header = bytearray(empty[:HEADER_BYTES])
    header[HEAP_COUNTER_AT:HEAP_COUNTER_AT + 4] = np.int32(counter).tobytes()
    header[NUM_ALLOCATED_AT:NUM_ALLOCATED_AT + 8] = np.uint64(used.sum()).tobytes()
    payload = voxels.reshape(pool, 512)[table["ptr"][used] // 512]
    return bytes(header), table, heap, payload


ALLOCATED_TOTAL_AT = 208                           # uint32 allocatedTotal inside the header


def snapshot_of_state(empty, table, heap, counter, voxels):
    """The bytes of a VHSNAP01 file that holds an explicit state, slot for slot: `table` [entries] ENTRY (ptr, offset and the
    pos of the free slots as given), `heap` [pool] uint32, the heap counter and `voxels` [pool * 512] VOXEL, from the bytes of
    the snapshot an EMPTY context of the same parameters (and bucket range) saved.  heapCounter, allocatedTotal and
    numAllocated of the header are patched."""
    assert empty[:8] == b"VHSNAP01"
    num_entries = int(np.frombuffer(empty, "<u8", 1, NUM_ALLOCATED_AT - 8)[0])
    pool = int(np.frombuffer(empty, "<u4", 1, 8 + 128 + 12)[0])
    assert len(empty) == HEADER_BYTES + num_entries * ENTRY.itemsize + pool * 4, "not the snapshot of an empty context"
    table, heap = np.ascontiguousarray(table, ENTRY), np.ascontiguousarray(heap, "<u4")
    voxels = np.ascontiguousarray(voxels, VOXEL).reshape(pool, 512)
    assert len(table) == num_entries and len(heap) == pool
    used = table["ptr"] != -1
    assert int(used.sum()) + int(counter) + 1 == pool, "entries and free list do not partition the pool"
    header = bytearray(empty[:HEADER_BYTES])
    header[HEAP_COUNTER_AT:HEAP_COUNTER_AT + 4] = np.int32(counter).tobytes()
    header[ALLOCATED_TOTAL_AT:ALLOCATED_TOTAL_AT + 4] = np.uint32(used.sum()).tobytes()
    header[NUM_ALLOCATED_AT:NUM_ALLOCATED_AT + 8] = np.uint64(used.sum()).tobytes()
    return bytes(header) + table.tobytes() + heap.tobytes() + voxels[table["ptr"][used] // 512].tobytes()


def load_state(gt, table, heap, counter, voxels, tmp_path, name="state.snap"):
    """Put an explicit state into the empty context `gt` through a snapshot (snapshot_of_state)."""
    path = os.path.join(str(tmp_path), name)
    gt.save_snapshot(path + ".empty")
    with open(path + ".empty", "rb") as f:
        empty = f.read()
    os.remove(path + ".empty")
    with open(path, "wb") as f:
        f.write(snapshot_of_state(empty, table, heap, counter, voxels))
    gt.load_snapshot(path)
    os.remove(path)
    return gt


def write_snapshot(path, gt, model, seed=0):
    """A snapshot file gt.load_snapshot accepts, holding `model`.  `gt` must be empty: it saves itself for the header."""
    path = str(path)
    gt.save_snapshot(path + ".empty")
    with open(path + ".empty", "rb") as f:
        empty = f.read()
    os.remove(path + ".empty")
    header, table, heap, payload = snapshot_parts(empty, model, seed)
    with open(path, "wb") as f:
        f.write(header)
        f.write(table.tobytes())
        f.write(heap.tobytes())
        f.write(payload.tobytes())
    return table


def load_model(gt, model, tmp_path, seed=0):
    """Put `model` into the empty context `gt` through a snapshot and check that the table holds exactly its keys."""
    path = os.path.join(str(tmp_path), "crafted.snap")
    write_snapshot(path, gt, model, seed)
    gt.load_snapshot(path)
    os.remove(path)
    have = sorted(map(tuple, gt.allocated()["pos"].tolist()))
    assert have == sorted(tuple(int(c) for c in k) for k in model), "the table does not hold exactly the crafted keys"
    return gt


def view_records(model):
    """The model as vh_view_record s, [N, 4112] uint8 in the dictionary's order."""
    keys, vox = model_arrays(model)
    rec = np.zeros((len(keys), RECORD_BYTES), np.uint8)
    rec[:, :12] = keys.astype("<i4").view(np.uint8).reshape(-1, 12)
    rec[:, 16:] = vox.view(np.uint8).reshape(len(keys), 4096)
    return rec


def records_as_voxels(rec):
    """The record buffer as the Voxel array a view table's ptr values address (ptr = record * 514 + 2)."""
    return np.ascontiguousarray(rec).reshape(-1).view(VOXEL)


def model_of(table, voxels):
    """The model a downloaded table and voxel array hold."""
    out = {}
    for e in table[table["ptr"] != -1]:
        v = voxels[int(e["ptr"]):int(e["ptr"]) + 512]
        out[tuple(int(c) for c in e["pos"])] = (v["sdf"].copy(), v["weight"].copy())
    return out


def reference(model, normals=True, region=None, voxel_size=0.02, num_buckets=509, bucket_size=8):
    """tests/mesh_ref.py on the model alone (placed as a table would hold it)."""
    table, _, _, voxels = place(model, num_buckets, bucket_size, max(1, len(model)) + 3, seed=1)
    return mesh_ref.extract(table, voxels, voxel_size, region, normals=normals)


# ---------------------------------------------------------------------------------------------------------------------
# facts about a model (independent of mesh_ref.extract)
# ---------------------------------------------------------------------------------------------------------------------
class Dense:
    """The model as dense arrays over the bounding box of its keys plus one voxel of margin on every side:
    sdf, weight [Z, Y, X] (weight 0 outside the blocks), origin = global voxel of index (1, 1, 1)."""

    def __init__(self, model):
        keys = np.array(list(model.keys()), np.int64)
        lo, hi = keys.min(0), keys.max(0) + 1
        size = (hi - lo) * 8 + 2
        assert size.prod() < 1 << 27, "a dense copy is meant for clusters"
        self.origin = lo * 8
        self.sdf = np.zeros(size[::-1], F)
        self.weight = np.zeros(size[::-1], F)
        for k, (s, w) in model.items():
            x, y, z = (np.array(k) - lo) * 8 + 1
            self.sdf[z:z + 8, y:y + 8, x:x + 8] = np.asarray(s, F).reshape(8, 8, 8)
            self.weight[z:z + 8, y:y + 8, x:x + 8] = np.asarray(w, F).reshape(8, 8, 8)
        with np.errstate(invalid="ignore"):
            self.valid = (self.weight > 0) & ~np.isnan(self.sdf)           # the rule: weight > 0 (and a NaN sdf is no sample)
            self.inside = self.sdf <= 0

    def corner(self, a, i):
        """a shifted so that index (z, y, x) is corner i of the cell at (z, y, x)."""
        dz, dy, dx = i >> 2, (i >> 1) & 1, i & 1
        Z, Y, X = a.shape
        return a[dz:Z - 1 + dz, dy:Y - 1 + dy, dx:X - 1 + dx]

    def cells(self):
        """(cell valid [Z-1, Y-1, X-1], corner mask): a cell is valid iff its eight corners are."""
        ok = np.ones(tuple(s - 1 for s in self.sdf.shape), bool)
        mask = np.zeros(ok.shape, np.int64)
        for i in range(8):
            ok &= self.corner(self.valid, i)
            mask |= self.corner(self.inside, i).astype(np.int64) << i
        return ok, mask

    def emitting_cells(self):
        """Global voxel coordinates [K, 3] of the cells that emit: valid, mask neither 0 nor 255."""
        ok, mask = self.cells()
        z, y, x = np.nonzero(ok & (mask != 0) & (mask != 255))
        return np.stack([x, y, z], 1) - 1 + self.origin, mask[z, y, x]

    def vertices(self):
        """One row per emitted vertex (every triangle of every emitting cell, three each): dict of
        a, b = dense index (z, y, x) of the edge's ends [V, 3], sA, sB, and t = sA / (sA - sB) in float32."""
        ok, mask = self.cells()
        z, y, x = np.nonzero(ok & (mask != 0) & (mask != 255))
        cm = mask[z, y, x]
        tm = np.zeros((len(cm), 6), np.int64)
        for s in range(4):
            tm |= ((cm[:, None] >> mesh_ref.TETS[None, :, s]) & 1) << s
        present = np.arange(2)[None, None, :] < mesh_ref.TRI_N[np.arange(6)[None, :], tm][:, :, None]
        e, t, k = np.nonzero(present)
        edges = mesh_ref.TRI_E[t, tm[e, t], k]                                   # [T, 3, 2] slots
        ca = mesh_ref.TETS[t[:, None], edges[:, :, 0]].reshape(-1)
        cb = mesh_ref.TETS[t[:, None], edges[:, :, 1]].reshape(-1)
        cell = np.repeat(np.stack([z[e], y[e], x[e]], 1), 3, axis=0)              # [V, 3] (z, y, x)
        bits = lambda c: np.stack([c >> 2, (c >> 1) & 1, c & 1], 1)
        a, b = cell + bits(ca), cell + bits(cb)
        sA, sB = self.sdf[tuple(a.T)], self.sdf[tuple(b.T)]
        with np.errstate(all="ignore"):
            tt = (sA / (sA - sB)).astype(F)
        return {"a": a, "b": b, "sA": sA, "sB": sB, "t": tt, "tet": np.repeat(t, 3), "tet_mask": np.repeat(tm[e, t], 3)}

    def one_sided(self, p):
        """For dense indices p [V, 3] of valid voxels: True where, on at least one axis, exactly one of the two neighbours is
        valid (the gradient there is a one-sided difference)."""
        out = np.zeros(len(p), bool)
        for axis in range(3):
            d = np.zeros(3, np.int64)
            d[axis] = 1
            out |= self.valid[tuple((p + d).T)] != self.valid[tuple((p - d).T)]
        return out


def mask_census(model):
    """(count of valid cells per corner mask [256], set of (tetrahedron, mask) words used by the emitting cells)."""
    d = Dense(model)
    ok, mask = d.cells()
    census = np.bincount(mask[ok], minlength=256)
    v = d.vertices()
    return census, set(zip(v["tet"].tolist(), v["tet_mask"].tolist()))


def is_subnormal(a):
    a = np.abs(np.asarray(a, F))
    return (a > 0) & (a < np.finfo(F).tiny)


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def cube_keys(lo, hi):
    """Keys lo <= k < hi per axis (scalars or triples), x fastest."""
    lo, hi = np.broadcast_to(lo, 3), np.broadcast_to(hi, 3)
    return [(int(x), int(y), int(z)) for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])]


def uniform_model(keys, seed, dead=0.02):
    """sdf uniform in (-1, 1), weight 1 except a share `dead` of weight 0."""
    rng = np.random.RandomState(seed)
    model = {}
    for k in keys:
        sdf = rng.uniform(-1, 1, 512).astype(F)
        weight = np.where(rng.uniform(size=512) < dead, 0, 1).astype(F)
        model[k] = (sdf, weight)
    return model


def every_configuration(seed=3):
    """3x3x3 blocks of noise: every one of the 256 corner masks, every table word."""
    return uniform_model(cube_keys(0, 3), seed)


def wide_magnitudes(seed=3):
    """The signs of every_configuration, |sdf| log-uniform over 1e-30 .. 1e3: t next to 0 and next to 1."""
    rng = np.random.RandomState(seed + 1000)
    model = {}
    for k, (sdf, weight) in every_configuration(seed).items():
        mag = (10.0 ** rng.uniform(-30, 3, 512)).astype(F)
        model[k] = (np.copysign(mag, sdf).astype(F), weight)
    return model


def zeros(seed=5):
    """A good tenth of the voxels +0.0, another -0.0 (both inside): vertices on corners, degenerate triangles."""
    rng = np.random.RandomState(seed + 2000)
    model = {}
    for k, (sdf, weight) in uniform_model(cube_keys(-1, 1), seed).items():
        u = rng.uniform(size=512)
        sdf = np.where(u < 0.12, F(0.0), np.where(u < 0.24, F(-0.0), sdf)).astype(F)
        model[k] = (sdf, weight)
    return model


def subnormals(seed=7):
    """Four voxels in ten with |sdf| in the float32 subnormal range (random sign), the rest uniform in (-1, 1)."""
    rng = np.random.RandomState(seed + 3000)
    model = {}
    for k, (sdf, weight) in uniform_model(cube_keys(-1, 1), seed).items():
        tiny = rng.randint(1, 1 << 23, 512).astype(np.uint32).view(F)
        sdf = np.where(rng.uniform(size=512) < 0.4, np.copysign(tiny, sdf), sdf).astype(F)
        model[k] = (sdf, weight)
    return model


def non_finite(seed=9):
    """About 1 % of the voxels each: +inf, -inf, and a NaN sdf with weight 1."""
    rng = np.random.RandomState(seed + 4000)
    model = {}
    for k, (sdf, weight) in uniform_model(cube_keys(-1, 1), seed).items():
        u = rng.uniform(size=512)
        sdf = np.where(u < 0.01, F(np.inf), np.where(u < 0.02, F(-np.inf), np.where(u < 0.03, F(np.nan), sdf))).astype(F)
        weight = np.where((u >= 0.02) & (u < 0.03), F(1), weight).astype(F)
        model[k] = (sdf, weight)
    return model


WEIGHTS = np.array([0.0, -1.0, 1e-45, np.inf, np.nan, 1.0], F)             # valid iff weight > 0: 1e-45, +inf and 1
WEIGHT_SHARES = [0.03, 0.03, 0.3, 0.3, 0.03, 0.31]


def weights(seed=11):
    """Weights drawn from {0, -1, 1e-45 (subnormal), +inf, NaN, 1}; sdf uniform."""
    rng = np.random.RandomState(seed + 5000)
    assert WEIGHTS[2] > 0 and is_subnormal(WEIGHTS[2])
    model = {}
    for k, (sdf, _) in uniform_model(cube_keys(-1, 1), seed).items():
        model[k] = (sdf, WEIGHTS[rng.choice(6, 512, p=WEIGHT_SHARES)])
    return model


HOLE_SEEDS = list(range(16))
NEIGHBOURS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def holes(seed):
    """A random subset of a 3x3x3 cluster (always the centre) around a key with negative parts, 10 % of the weights 0."""
    rng = np.random.RandomState(seed + 6000)
    centre = (-2, 3, -1)
    keys = [centre] + [tuple(int(c + o) for c, o in zip(centre, d)) for d in NEIGHBOURS if rng.uniform() < 0.5]
    return uniform_model(keys, seed + 100, dead=0.10)


def holes_present(seed):
    """The offsets of the blocks of holes(seed) around its centre."""
    return {tuple(int(c) for c in np.array(k) - (-2, 3, -1)) for k in holes(seed)}


def zero_gradient():
    """sdf = -1 at even x, +1 at odd x, constant in y and z, 2x2x2 blocks, all weights 1: every central difference is 0."""
    x = np.arange(512) & 7
    sdf = np.where(x % 2 == 0, F(-1), F(1)).astype(F)
    return {k: (sdf.copy(), np.ones(512, F)) for k in cube_keys(0, 2)}


def lone_block(seed=13):
    return uniform_model([(5, -3, 2)], seed, dead=0.0)


FAR = 1 << 21                  # 8 * key = 2^24: from here on the voxel coordinate is not exact in float32
EDGE = (1 << 28) - 1           # the largest |key| of the rule's domain
KEY_CLUSTERS = {
    "origin": cube_keys(-1, 1),
    "plus 2^24": cube_keys((FAR - 1, -1, FAR - 1), (FAR + 1, 1, FAR + 1)),
    "minus 2^24": cube_keys((-FAR - 1, -FAR - 1, -1), (-FAR + 1, -FAR + 1, 1)),
    "plus end": cube_keys((EDGE - 1, EDGE - 1, -1), (EDGE + 1, EDGE + 1, 1)),
    "minus end": cube_keys((-EDGE, -1, -EDGE), (-EDGE + 2, 1, -EDGE + 2)),
}
KEY_REGIONS = [
    ((INT32_MIN,) * 3, (0, 0, 0)),
    ((-1, -1, -1), (INT32_MAX,) * 3),
    ((INT32_MIN, -FAR - 1, INT32_MIN), (INT32_MAX, -FAR, INT32_MAX)),
    ((-FAR, INT32_MIN, -1), (FAR, INT32_MAX, FAR)),
    ((EDGE, EDGE - 1, INT32_MIN), (INT32_MAX, INT32_MAX, INT32_MAX)),
    ((INT32_MIN, INT32_MIN, INT32_MIN), (-EDGE + 1, INT32_MAX, -EDGE + 1)),
]


def keys_model(seed=15):
    """2x2x2 clusters across the origin, across 8 * key = +-2^24 and at both ends of the key domain |key| < 2^28."""
    return uniform_model([k for c in KEY_CLUSTERS.values() for k in c], seed)


# ---- sizes ----
def ball_model(keys, centre, radius, seed, dead=0.01, noise=0.05):
    """The distance (in voxels) to a sphere, plus a little noise, sampled in the given blocks: only the blocks the surface
    passes through emit.  Vectorised: (keys [N, 3], voxels [N, 512] VOXEL)."""
    rng = np.random.RandomState(seed)
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    i = np.arange(512)
    local = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    p = keys[:, None, :] * 8 + local[None, :, :] - np.asarray(centre, np.float64)[None, None, :]
    vox = np.zeros((len(keys), 512), VOXEL)
    vox["sdf"] = (np.sqrt((p * p).sum(-1)) - radius + rng.uniform(-noise, noise, (len(keys), 512))).astype(F)
    vox["weight"] = np.where(rng.uniform(size=(len(keys), 512)) < dead, 0, 1)
    return keys, vox


def as_model(keys, vox):
    return {tuple(int(c) for c in k): (vox["sdf"][i], vox["weight"][i]) for i, k in enumerate(keys)}


MANY_BLOCKS = 3 * 8192 + 517                      # 517 workgroups run four passes, the others three
MANY_BUCKETS, MANY_BUCKET_SIZE = 1 << 16, 8      # (a cuboid of keys crowds the hash: 8 in one bucket)


def many_blocks(seed=21):
    """MANY_BLOCKS blocks of a 30x29x29 cuboid (the others missing, so that neighbourhoods differ), a sphere through it:
    the blocks the surface misses emit nothing and lie between those that emit in table order."""
    keys = np.array(cube_keys((-15, -14, -14), (15, 15, 15)), np.int64)
    keep = np.sort(np.random.RandomState(seed).permutation(len(keys))[:MANY_BLOCKS])
    return as_model(*ball_model(keys[keep], (3.3, 2.1, -1.7), 97.4, seed + 1))


PLANE = (np.arange(512) & 7).astype(F) - F(3.4)                                # a plane x = 3.4 through a block


def plane_block(rng):
    return (PLANE + rng.uniform(-0.2, 0.2, 512)).astype(F), np.ones(512, F)


def key_for_bucket(x, y, bucket, num_buckets):
    """The key (x, y, z >= 0) that hashes to `bucket` of a power-of-two table: the z factor of the hash is odd, so it has an
    inverse modulo the bucket count."""
    assert num_buckets & (num_buckets - 1) == 0
    m = num_buckets - 1
    z = ((bucket ^ ((x * 73856093) ^ (y * 19349669))) & m) * pow(83492791, -1, num_buckets) & m
    assert hash_block([(x, y, z)], num_buckets)[0] == bucket
    return (x, y, int(z))


SLICE_BUCKETS = 1 << 21        # 2048 slices of 1024 buckets: two tiles of the slice scan
SLICE_BALL_LO = (94, 31, -56)  # many_slices: the ball's 12^3 blocks begin here (away from the origin, where the hash crowds)


def many_slices(seed=23):
    """A ball of 12^3 blocks plus 1500 lone blocks with a plane through them, in a table of 2^21 buckets: entries in both
    tiles of the slice scan, in the last slice and in the last bucket."""
    rng = np.random.RandomState(seed)
    lo = np.array(SLICE_BALL_LO)
    model = as_model(*ball_model(cube_keys(lo, lo + 12), lo * 8 + 48.3, 40.3, seed + 1))
    taken = set()
    lone = []
    while len(lone) < 1500:
        k = tuple(int(c) * 3 for c in rng.randint(10, 300, 3) * rng.choice([-1, 1], 3))      # multiples of 3: never adjacent
        if k not in taken and not ((np.array(k) >= lo - 1) & (np.array(k) <= lo + 12)).all():      # clear of the ball
            taken.add(k)
            lone.append(k)
    # chosen buckets: the last one (twice: two slots), the last slice, the first bucket, both sides of the tile boundary
    for n, bucket in enumerate((SLICE_BUCKETS - 1, SLICE_BUCKETS - 1, SLICE_BUCKETS - 700, 0, (1 << 20) - 1, 1 << 20)):
        k = key_for_bucket(1000 + 3 * n, -1000, bucket, SLICE_BUCKETS)
        assert k not in taken
        taken.add(k)
        lone.append(k)
    for k in lone:
        model[k] = plane_block(rng)
    return model


def many_slices_table(vh, tmp_path):
    """many_slices() loaded into its table of 2^21 buckets of 2 slots."""
    gt = vh.SDFHashtable(vh.default_params(numBuckets=SLICE_BUCKETS, bucketSize=2, numVoxelBlocks=4096), 640, 480, 1)
    return load_model(gt, many_slices(), tmp_path)


def in_both_slice_tiles(entries):
    """Whether entry indices of that table lie in both tiles of the slice scan: on both sides of bucket 2^20."""
    bucket = np.asarray(entries) // 2
    return bool((bucket < SLICE_BUCKETS // 2).any() and (bucket >= SLICE_BUCKETS // 2).any())


TILE_BUCKETS, TILE_BUCKET_SIZE = 1 << 19, 8
MANY_TILES = 258 * 1024 + 37   # listed blocks: 259 tiles of the block-count scan, two rounds of its second level
TILES_WITH_SURFACE = (0, 128, 255, 256, 258)


def many_tiles_plan(seed=25):
    """(keys [N, 3] int32, emits [N] bool) of MANY_TILES isolated blocks: random keys on the lattice of multiples of 3 (no two are
    adjacent); a block emits (holds a plane) if its position in the list is = 30 modulo 61 or lies in the middle of one of
    TILES_WITH_SURFACE, all others hold nothing.  The position in the list is the rank of the key's bucket; the order inside
    a bucket (the import's choice) moves it by less than a bucket's slots."""
    rng = np.random.RandomState(seed)
    keys = np.unique(rng.randint(-(1 << 18), 1 << 18, (MANY_TILES + 4096, 3)), axis=0)
    keys = keys[rng.permutation(len(keys))[:MANY_TILES]] * 3
    bucket = hash_block(keys, TILE_BUCKETS)
    assert np.bincount(bucket).max() <= TILE_BUCKET_SIZE
    rank = np.argsort(np.argsort(bucket, kind="stable"), kind="stable")
    middle = (rank & 1023 >= 500) & (rank & 1023 < 520) & np.isin(rank >> 10, TILES_WITH_SURFACE)
    return keys.astype(np.int32), (rank % 61 == 30) | middle


VIEW_STEP_BUCKETS, VIEW_STEP_BUCKET_SIZE = 1 << 15, 8


def view_steps(seed=27):
    """Three models for one view context that grows and shrinks: 100, 5000 and 50 blocks, a sphere through each."""
    out = []
    off = np.array((200, -150, 90))                                            # (away from the origin, where the hash crowds)
    for n, (lo, hi), radius in ((100, ((0, 0, 0), (5, 5, 4)), 20.3), (5000, ((-8, -8, -9), (9, 9, 9)), 90.3),
                                (50, ((3, -2, 1), (8, 3, 3)), 20.3)):
        lo, hi = np.array(lo) + off, np.array(hi) + off
        keys = np.array(cube_keys(lo, hi), np.int64)
        keep = np.sort(np.random.RandomState(seed + n).permutation(len(keys))[:n])
        out.append(as_model(*ball_model(keys[keep], np.array(lo) * 8 - 0.3, radius, seed + n + 1)))
    return out
