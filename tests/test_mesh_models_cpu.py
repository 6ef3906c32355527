"""The crafted models of tests/mesh_models.py without a GPU: every condition that keeps a GPU test of
tests/test_gpu_mesh_crafted.py / test_gpu_mesh_scale.py from passing vacuously holds for the specification
(tests/mesh_ref.py) on the built model, so a later edit of a seed cannot hollow a GPU test out."""
import ctypes as C

import numpy as np

import mesh_models as mm
import mesh_ref
from voxelhashing_demo_amd import _lib as L

U = np.uint32


def directed_edges_once(tris):
    """Every directed edge of the welded mesh at most once (degenerate triangles aside)."""
    _, faces = mesh_ref.weld(tris)
    good = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]
    directed = np.concatenate([good[:, [0, 1]], good[:, [1, 2]], good[:, [2, 0]]])
    _, counts = np.unique(directed, axis=0, return_counts=True)
    return counts.max() == 1


def cells_of(info):
    return set(map(tuple, info["cell"].tolist()))


def test_every_configuration():
    model = mm.every_configuration()
    tris, _, info = mm.reference(model)
    census, words = mm.mask_census(model)
    mixed = census[1:255]
    print(f"blocks={len(model)} cells={info['cells']} triangles={len(tris)} masks={np.count_nonzero(census)} rarest mixed={mixed.min()} "
          f"words={len(words)}")
    assert np.count_nonzero(census) == 256 and mixed.min() >= 10
    assert words == {(t, m) for t in range(6) for m in range(1, 15)}
    cells, _ = mm.Dense(model).emitting_cells()
    assert set(map(tuple, cells.tolist())) == cells_of(info) and len(cells) == info["cells"]
    assert directed_edges_once(tris)


def test_wide_magnitudes():
    model = mm.wide_magnitudes()
    tris, _, info = mm.reference(model)
    v = mm.Dense(model).vertices()
    assert len(v["t"]) == 3 * len(tris) > 10000
    low, high = (v["t"] < 1e-6).mean(), (v["t"] > 1 - 1e-6).mean()
    print(f"vertices={len(v['t'])} t<1e-6: {low:.3f}  t>1-1e-6: {high:.3f}")
    assert low >= 0.01 and high >= 0.01


def test_zeros():
    model = mm.zeros()
    sdf = np.concatenate([s for s, _ in model.values()])
    plus, minus = (sdf.view(U) == 0).mean(), (sdf.view(U) == 0x80000000).mean()
    assert plus >= 0.10 and minus >= 0.10
    tris, _, _ = mm.reference(model)
    same = lambda a, b: (tris[:, a].view(U) == tris[:, b].view(U)).all(1)
    two = same(0, 1) | same(1, 2) | same(0, 2)
    three = same(0, 1) & same(1, 2)
    print(f"+0: {plus:.3f} -0: {minus:.3f} triangles={len(tris)} two coincident={two.sum()} three={three.sum()}")
    assert (two & ~three).sum() > 0 and three.sum() > 0
    # an emitted edge has exactly one end inside: both zeros occur as that end
    v = mm.Dense(model).vertices()
    for bits in (0, 0x80000000):
        inside_end = ((v["sA"].view(U) == bits) & (v["sB"] > 0)) | ((v["sB"].view(U) == bits) & (v["sA"] > 0))
        assert inside_end.sum() > 100


def test_subnormals():
    model = mm.subnormals()
    tris, _, _ = mm.reference(model)
    v = mm.Dense(model).vertices()                          # one row per emitted vertex: the edge did emit
    share = (mm.is_subnormal(v["sA"]) | mm.is_subnormal(v["sB"])).mean()
    both = (mm.is_subnormal(v["sA"]) & mm.is_subnormal(v["sB"])).mean()
    print(f"vertices={len(v['t'])} on an edge with a subnormal end: {share:.3f}, both ends: {both:.3f}")
    assert len(v["t"]) == 3 * len(tris) and share >= 0.10 and both >= 0.01


def test_non_finite():
    model = mm.non_finite()
    d = mm.Dense(model)
    nan_valid = np.isnan(d.sdf) & (d.weight > 0)
    assert nan_valid.sum() > 20 and np.isinf(d.sdf).sum() > 40
    tris, nrm, info = mm.reference(model)
    cell = info["cell"] - d.origin + 1                      # dense index (x, y, z)
    for i in range(8):
        assert not nan_valid[cell[:, 2] + (i >> 2), cell[:, 1] + ((i >> 1) & 1), cell[:, 0] + (i & 1)].any()
    cells, _ = d.emitting_cells()                           # and with them not valid, the rule gives exactly these cells
    assert set(map(tuple, cells.tolist())) == cells_of(info)
    print(f"triangles={len(tris)} with a NaN coordinate={np.isnan(tris).any((1, 2)).sum()}")
    assert np.isnan(tris).any() and not np.isnan(tris).all()


def test_weights():
    model = mm.weights()
    d = mm.Dense(model)
    tris, _, info = mm.reference(model)
    cells, _ = d.emitting_cells()
    assert set(map(tuple, cells.tolist())) == cells_of(info) and len(cells) > 500
    cell = info["cell"] - d.origin + 1
    seen = set()
    for i in range(8):
        w = d.weight[cell[:, 2] + (i >> 2), cell[:, 1] + ((i >> 1) & 1), cell[:, 0] + (i & 1)]
        seen |= set(w.view(U).tolist())
    print(f"cells={len(cells)} weights at the corners of emitting cells: {sorted(np.array(sorted(seen), U).view(np.float32).tolist())}")
    assert seen == set(mm.WEIGHTS[[2, 3, 5]].view(U).tolist())            # 1e-45, +inf and 1 -- never 0, -1 or NaN


def test_holes():
    absent, present = set(), set()
    for seed in mm.HOLE_SEEDS:
        model = mm.holes(seed)
        have = mm.holes_present(seed)
        assert (0, 0, 0) in have
        present |= have
        absent |= set(mm.NEIGHBOURS) - have
        d = mm.Dense(model)
        v = d.vertices()
        share = (d.one_sided(v["a"]) | d.one_sided(v["b"])).mean()
        print(f"seed {seed}: blocks={len(model)} vertices={len(v['t'])} one-sided={share:.3f}")
        assert 0.10 <= share <= 0.90 and len(v["t"]) > 1000
        if seed < 4:
            tris, _, info = mm.reference(model)
            assert 3 * len(tris) == len(v["t"]) and directed_edges_once(tris)
    assert present >= set(mm.NEIGHBOURS) and absent == set(mm.NEIGHBOURS)


def test_zero_gradient():
    model = mm.zero_gradient()
    tris, nrm, _ = mm.reference(model)
    zero = (nrm.reshape(-1, 3).view(U) << 1 == 0).all(1).mean()
    print(f"triangles={len(tris)} zero normals={zero:.3f}")
    assert len(tris) > 1000 and zero >= 0.5 and not np.isnan(nrm).any()


def test_lone_block():
    model = mm.lone_block()
    (key,) = model
    tris, _, info = mm.reference(model)
    local = info["cell"] - np.array(key) * 8
    assert local.min() >= 0 and local.max() <= 6
    cells, _ = mm.Dense(model).emitting_cells()
    print(f"emitting cells={info['cells']} of 343")
    assert len(cells) == info["cells"] >= 300 and set(map(tuple, cells.tolist())) == cells_of(info)


def test_keys():
    model = mm.keys_model()
    tris, _, info = mm.reference(model)
    blocks = set(map(tuple, info["block"].tolist()))
    for name, keys in mm.KEY_CLUSTERS.items():
        assert set(keys) <= blocks, name                     # triangles in every block: on both sides of every seam
        lo = np.array(keys).min(0)
        mine = info["cell"][(info["block"] == lo).all(1)] - lo * 8
        for axis in range(3):
            assert (mine[:, axis] == 7).any(), (name, axis)  # and in the cells that straddle the seam
    assert max(abs(c) for k in model for c in k) == mm.EDGE == (1 << 28) - 1
    for region in mm.KEY_REGIONS:
        _, _, part = mm.reference(model, region=region)
        print(region, part["blocks"])
        assert 0 < part["blocks"] < len(model)
        lo, hi = np.array(region[0]), np.array(region[1])
        assert part["blocks"] == sum(bool(((np.array(k) >= lo) & (np.array(k) < hi)).all()) for k in model)


def test_capacities_are_distinct():
    tris, _, info = mm.reference(mm.every_configuration())
    first_cell = int((info["cell"] == info["cell"][0]).all(1).sum())
    first_block = int((info["block"] == info["block"][0]).all(1).sum())
    print(f"first cell: {first_cell} triangles, first block: {first_block}, all: {len(tris)}")
    assert 2 < first_cell + 1 < first_block - 1 and first_block + 1 < len(tris) - 1


def test_many_blocks():
    model = mm.many_blocks()
    assert len(model) == mm.MANY_BLOCKS > 3 * 8192
    keys = set(model)
    full = sum(all((k[0] + d[0], k[1] + d[1], k[2] + d[2]) in keys for d in mm.NEIGHBOURS) for k in keys)
    assert 0 < full < len(model)                             # neighbourhoods differ
    table, _, _, voxels = mm.place(model, mm.MANY_BUCKETS, mm.MANY_BUCKET_SIZE, len(model) + 11)
    tris, _, info = mesh_ref.extract(table, voxels, 0.02, normals=False)
    listed = table[table["ptr"] != -1]
    index = {tuple(p): i for i, p in enumerate(listed["pos"].tolist())}
    emits = np.zeros(len(listed), bool)
    emits[[index[b] for b in set(map(tuple, info["block"].tolist()))]] = True
    changes = np.count_nonzero(emits[1:] != emits[:-1])
    print(f"blocks={len(listed)} emitting={emits.sum()} runs={changes + 1} triangles={len(tris)}")
    assert 1000 < emits.sum() < len(listed) - 1000 and changes > 1000
    for lo in range(0, len(listed), 8192):                   # in every pass of the grid
        assert emits[lo:lo + 8192].any() and not emits[lo:lo + 8192].all()


def test_many_slices():
    model = mm.many_slices()
    table, _, _, voxels = mm.place(model, mm.SLICE_BUCKETS, 2, 4096)
    at = np.nonzero(table["ptr"] != -1)[0]
    bucket = at // 2
    assert len(at) == len(model) > 3000
    assert (bucket == mm.SLICE_BUCKETS - 1).sum() == 2 and (bucket == 0).any()
    assert ((bucket >> 10) == 2047).sum() >= 3 and (bucket == (1 << 20) - 1).any() and (bucket == 1 << 20).any()
    tris, _, info = mesh_ref.extract(table, voxels, 0.02, normals=False)
    where = {tuple(p): b for p, b in zip(table["pos"][at].tolist(), bucket.tolist())}
    emitting = np.array(sorted({where[b] for b in set(map(tuple, info["block"].tolist()))}))
    tiles = np.bincount(emitting >> 20, minlength=2)
    print(f"blocks={len(at)} emitting blocks per slice tile={tiles.tolist()} triangles={len(tris)}")
    assert tiles.min() > 500 and emitting.max() == mm.SLICE_BUCKETS - 1


def test_many_tiles_plan():
    keys, emit = mm.many_tiles_plan()
    assert len(keys) == mm.MANY_TILES > 256 * 1024 + 1024 and len(np.unique(keys, axis=0)) == len(keys)
    assert (keys % 3 == 0).all()                             # isolated: no two keys adjacent
    bucket = mm.hash_block(keys, mm.TILE_BUCKETS)
    assert np.bincount(bucket).max() <= mm.TILE_BUCKET_SIZE
    rank = np.argsort(np.argsort(bucket, kind="stable"), kind="stable")      # list position, up to the order inside a bucket
    last = (len(keys) - 1) >> 10
    sure = emit & ((rank & 1023) >= mm.TILE_BUCKET_SIZE) & ((rank & 1023) < 1024 - mm.TILE_BUCKET_SIZE)   # in their tile whatever that order
    tiles = set((rank[sure] >> 10).tolist())
    print(f"records={len(keys)} emitting={emit.sum()} block tiles={last + 1} tiles with surface={len(tiles)}")
    assert set(mm.TILES_WITH_SURFACE) <= tiles and last == 258 and mm.TILES_WITH_SURFACE[-1] == last
    assert 1000 < emit.sum() < len(keys) // 10


def test_view_steps():
    sizes = [len(m) for m in mm.view_steps()]
    assert sizes == [100, 5000, 50]
    for m in mm.view_steps():
        tris, _, _ = mm.reference(m, normals=False, num_buckets=mm.VIEW_STEP_BUCKETS, bucket_size=mm.VIEW_STEP_BUCKET_SIZE)
        assert len(tris) > 100


def test_snapshot_bytes_parse_back(tmp_path):
    """A parser of the file format written here, on the bytes write_snapshot's core produces for a small model."""
    nb, bs, pool = 64, 4, 40
    params = L.HashTableParams()
    params.numBuckets, params.bucketSize, params.numVoxelBlocks, params.voxelBlockSize, params.voxelSize = nb, bs, pool, 8, 0.02
    free = np.zeros(nb * bs, mm.ENTRY)
    free["pos"], free["ptr"] = -(1 << 31), -1
    tail = np.zeros(1, np.dtype([("heapCounter", "<i4"), ("counters", "<u4", (3,)), ("pad", "<u4"), ("numEntries", "<u8"),
                                 ("numAllocated", "<u8"), ("proj", "<f4", (9,)), ("pad2", "<u4")]))
    tail["heapCounter"], tail["numEntries"] = pool - 1, nb * bs
    head = b"VHSNAP01" + bytes(params) + np.array([640, 480, 1], "<i4").tobytes() + np.array([0, nb], "<u4").tobytes() + tail.tobytes()
    assert len(head) == mm.HEADER_BYTES
    empty = head + free.tobytes() + np.arange(pool, dtype="<u4").tobytes()
    model = mm.holes(0)
    header, table, heap, payload = mm.snapshot_parts(empty, model, seed=4)
    blob = header + table.tobytes() + heap.tobytes() + payload.tobytes()

    # ---- the parser ----
    assert blob[:8] == b"VHSNAP01"
    p = L.HashTableParams.from_buffer_copy(blob[8:8 + C.sizeof(L.HashTableParams)])
    assert (p.numBuckets, p.bucketSize, p.numVoxelBlocks) == (nb, bs, pool)
    rest = np.frombuffer(blob[:mm.HEADER_BYTES], tail.dtype, 1, 204)[0]
    n = len(model)
    assert rest["numEntries"] == nb * bs and rest["numAllocated"] == n and rest["heapCounter"] == pool - n - 1
    t = np.frombuffer(blob, mm.ENTRY, nb * bs, mm.HEADER_BYTES)
    h = np.frombuffer(blob, "<u4", pool, mm.HEADER_BYTES + t.nbytes)
    body = np.frombuffer(blob, mm.VOXEL, offset=mm.HEADER_BYTES + t.nbytes + h.nbytes).reshape(-1, 512)
    assert len(blob) == mm.HEADER_BYTES + t.nbytes + h.nbytes + n * 4096
    used = np.nonzero(t["ptr"] != -1)[0]
    assert len(used) == n and (t["offset"] == 0).all() and (t["ptr"][used] % 512 == 0).all()
    ids = t["ptr"][used] // 512
    assert sorted(ids.tolist() + h[:pool - n].tolist()) == list(range(pool))          # blocks and free list partition the pool
    for row, e in zip(body, t[used]):
        key = tuple(int(c) for c in e["pos"])
        x, y, z = key
        assert (((x * 73856093) ^ (y * 19349669) ^ (z * 83492791)) & 0xFFFFFFFF) % nb == np.nonzero(t["ptr"] == e["ptr"])[0][0] // bs
        assert np.array_equal(row["sdf"].view(U), model[key][0].view(U)) and np.array_equal(row["weight"].view(U), model[key][1].view(U))
    for b in range(nb):                                                                # a bucket's entries are a prefix of its slots
        taken = t["ptr"][b * bs:(b + 1) * bs] != -1
        assert not (taken[1:] & ~taken[:-1]).any()
    assert (t["pos"][t["ptr"] == -1] == -(1 << 31)).all()                              # free entries as the library left them


def test_view_records_layout():
    model = mm.lone_block()
    rec = mm.view_records(model)
    (key,) = model
    assert rec.shape == (1, 4112) and rec[0, :16].view("<i4").tolist() == [*key, 0]
    vox = mm.records_as_voxels(rec)
    assert np.array_equal(vox["sdf"][2:514].view(U), model[key][0].view(U))
