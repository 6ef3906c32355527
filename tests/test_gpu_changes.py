"""vh_changes against tests/changes_ref.py, the rule in numpy: the lists in order, the counts and the state's bytes after every
call, on small crowded tables (bucket size 1, 2 and 5, with and without the overflow list, a shard pair) whose blocks are
hand-made records put in by stream_in.  A voxel's bits are changed the only way arbitrary bits get into a table: the block
is deleted and streamed in again."""
import ctypes as C
import itertools

import numpy as np
import pytest

import changes_ref as R
import mesh_models as mm

pytestmark = pytest.mark.gpu
U = np.uint32
F = np.float32
# (numBuckets, bucketSize, numVoxelBlocks, overflow_list)
CONFIGS = [(64, 1, 64, 0), (64, 1, 64, 1), (64, 2, 128, 0), (64, 2, 128, 1), (1024, 5, 256, 0), (256, 5, 256, 1)]
IDS = [f"{b}x{s} pool {p}{' chains' if o else ''}" for b, s, p, o in CONFIGS]
HALOS = [R.HALO_NONE, R.HALO_MESH, R.HALO_NORMALS]
CENTRE = (0, 0, 0)
VOXEL = mm.VOXEL


ESSENTIAL = [CENTRE, (-1, 0, 0), (5, 5, 5), (5, 5, 6)]            # blocks the tests name: each alone in its bucket of the smallest table


def cluster_keys():
    """A 3x3x3 cluster around the origin with holes, and blocks far away.  No other key shares a bucket (of 64, so of 256 and
    1024 too) with an ESSENTIAL one, so that those are placed even where a bucket has one slot and no chain."""
    rng = np.random.RandomState(5)
    home = lambda k: int(mm.hash_block([k], 64)[0])
    taken = {home(k) for k in ESSENTIAL}
    assert len(taken) == len(ESSENTIAL)
    keys = [d for d in itertools.product((-1, 0, 1), repeat=3) if d not in ESSENTIAL and rng.uniform() < 0.7]
    keys += [(-7, 3, 2), (40, -40, 3), (5, 4, 5)]
    return ESSENTIAL + [k for k in keys if home(k) not in taken]


def block(seed):
    rng = np.random.RandomState(1000 + seed)
    v = np.zeros(512, VOXEL)
    v["sdf"], v["weight"] = rng.standard_normal(512), rng.randint(0, 9, 512)
    return v, rng.randint(0, 1 << 32, 512, dtype=np.uint64).astype(U)


def chunk(keys, seeds=None):
    parts = [block(hash(k) % 977 if seeds is None else seeds[i]) for i, k in enumerate(keys)]
    return {"keys": np.array(keys, np.int32).reshape(-1, 3), "voxels": np.stack([p[0] for p in parts]),
            "colors": np.stack([p[1] for p in parts])}


def table(vh, cfg, bucket_range=None, keys=None):
    nb, bs, pool, overflow = cfg
    gt = vh.SDFHashtable(vh.default_params(numBuckets=nb, bucketSize=bs, numVoxelBlocks=pool), 64, 48, 1, bucket_range=bucket_range)
    if overflow:
        gt.set_option("overflow_list", 1)
    st = gt.stream_in(chunk(cluster_keys() if keys is None else keys))
    assert st["placed"] >= 4
    return gt


def held(gt):
    return [tuple(k) for k in gt.allocated()["pos"].tolist()]


def keys4(torch, keys):
    k = np.zeros((len(keys), 4), np.int32)
    k[:, :3] = np.asarray(keys, np.int32).reshape(-1, 3)
    return torch.from_numpy(k).cuda()


def state_bytes(st):
    return st.cpu().numpy().tobytes()


def call(torch, gt, st, ref, region=None, color=True, halo=R.HALO_MESH, caps=None):
    """One vh_changes and the reference's call on the arrays the context holds: counts, lists (in order; untouched where the
    call must not write) and the state's bytes.  Returns (changed {key: flags}, removed [key], committed)."""
    pool = gt.params.numVoxelBlocks
    tab, vox = gt.hash_table(), gt.sdf_blocks()
    col = gt.color_volume() if gt.has_color() else None
    capc, capr = caps if caps is not None else (pool, pool)
    wc, wr, ok = R.changes(tab, vox, col, ref, region, R.VOXELS | (R.COLOR if color else 0), halo, capc, capr)
    dc = torch.full((capc + 2, 4), -77, dtype=torch.int32, device="cuda")
    dr = torch.full((capr + 2, 4), -77, dtype=torch.int32, device="cuda")
    nc, nr = gt.changes_into(st, capc, dc if capc else None, capr, dr if capr else None, region, color, halo)
    print(f"listed={nc} removed={nr} committed={ok} epoch={ref.epoch}")
    assert (nc, nr) == (len(wc), len(wr))
    gc, gr = dc.cpu().numpy(), dr.cpu().numpy()
    if ok:
        assert np.array_equal(gc[:nc], wc) and np.array_equal(gr[:nr], wr)
        assert (gc[nc:] == -77).all() and (gr[nr:] == -77).all()
    else:
        assert (gc == -77).all() and (gr == -77).all()
    assert state_bytes(st) == ref.tobytes()
    return {tuple(r[:3]): int(r[3]) for r in wc.tolist()}, [tuple(r[:3]) for r in wr.tolist()], ok


def fresh(torch, gt, color=True, halo=R.HALO_MESH):
    """A state that has seen the model as it is."""
    st, ref = gt.changes_state(), R.State(gt.params.numVoxelBlocks)
    assert st.dtype == torch.uint8 and st.numel() == 64 + 32 * gt.params.numVoxelBlocks and not st.any()
    ch, rm, ok = call(torch, gt, st, ref, color=color, halo=halo)
    assert ok and not rm and sorted(ch) == sorted(held(gt)) and all(f & R.SELF for f in ch.values())
    return st, ref


def replace(torch, gt, key, voxels, colors):
    """The block of `key` with other bits: deleted and streamed in again."""
    gt.delete_blocks(keys4(torch, [key]))
    st = gt.stream_in({"keys": np.array([key], np.int32), "voxels": voxels.reshape(1, 512), "colors": colors.reshape(1, 512)})
    assert st["placed"] == 1


def bits_of(gt, key):
    e = gt.allocated()
    ptr = int(e["ptr"][[tuple(k) for k in e["pos"].tolist()].index(key)])
    return gt.sdf_blocks()[ptr:ptr + 512].copy(), gt.color_volume()[ptr:ptr + 512].copy()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_empty_state_then_nothing(vh, torch_cuda, cfg):
    gt = table(vh, cfg)
    st, ref = fresh(torch_cuda, gt)
    assert ref.epoch == 1 and int(ref.slots["live"].sum()) == len(held(gt))
    before = state_bytes(st)
    ch, rm, ok = call(torch_cuda, gt, st, ref)                     # a second call right after: 0 / 0
    assert ok and not ch and not rm and ref.epoch == 2
    assert state_bytes(st)[8:] == before[8:]                      # unchanged but for the epoch
    # a peek consumes changes only when there are none: here there are none, so it counts the epoch up too
    ch, rm, ok = call(torch_cuda, gt, st, ref, caps=(0, 0))
    assert ok and ref.epoch == 3
    gt.close()


def flips(torch, gt, st, ref, target, halo, expect_foreign=()):
    """One bit of sdf, weight and the colour word at voxels 0, 255 and 511 of `target`: exactly it is self-changed, and the
    reference's halo is listed."""
    offsets = R.halo_offsets(halo)
    for field, voxel in itertools.product(("sdf", "weight", "color"), (0, 255, 511)):
        vox, col = bits_of(gt, target)
        if field == "color":
            col[voxel] ^= U(1 << (voxel % 32))
        else:
            vox[field].view(U)[voxel] ^= U(1 << (voxel % 31))
        replace(torch, gt, target, vox, col)
        ch, rm, ok = call(torch, gt, st, ref, halo=halo)
        now = set(held(gt))
        want = {tuple(a + b for a, b in zip(target, o)) for o in offsets} & now
        assert ok and not rm and [k for k, f in ch.items() if f & R.SELF] == [target], (field, voxel)
        assert {k for k, f in ch.items() if f == R.HALO} == want and ch[target] == R.SELF
        assert not (set(expect_foreign) & set(ch))
    return want


@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_one_bit_in_one_block(vh, torch_cuda, cfg, halo):
    nb, bs, pool, overflow = cfg
    gt = table(vh, cfg)
    assert CENTRE in held(gt)
    st, ref = fresh(torch_cuda, gt, halo=halo)
    want = flips(torch_cuda, gt, st, ref, CENTRE, halo)
    # where the halo's neighbours are: absent ones, ones in other buckets, ones behind their home bucket (chains)
    e = gt.hash_table()
    at = {tuple(k): i for i, k in enumerate(e["pos"].tolist()) if e["ptr"][i] != -1}
    around = [tuple(a + b for a, b in zip(CENTRE, o)) for o in R.halo_offsets(R.HALO_NORMALS)]
    absent = [k for k in around if k not in at]
    buckets = {int(mm.hash_block([k], nb)[0]) for k in around if k in at}
    chained = [k for k in at if at[k] // bs != int(mm.hash_block([k], nb)[0])]
    print(f"neighbours: absent={len(absent)} buckets={len(buckets)} entries behind their home bucket={len(chained)} halo={len(want)}")
    assert absent and len(buckets) > 1
    if overflow and bs == 2:
        assert chained                   # (bucket size 2 forces chains; with one slot per bucket a colliding key is not placed at all)
    gt.close()


@pytest.mark.parametrize("halo", [R.HALO_MESH, R.HALO_NORMALS])
@pytest.mark.parametrize("overflow", [0, 1])
def test_a_shard_pair(vh, torch_cuda, overflow, halo):
    cfg = (64, 2, 128, overflow)
    shards = [table(vh, cfg, bucket_range=r) for r in ((0, 32), (32, 64))]
    owned = [set(held(s)) for s in shards]
    assert not (owned[0] & owned[1]) and all(len(o) >= 4 for o in owned)
    seen = 0
    for gt, mine, other in ((shards[0], owned[0], owned[1]), (shards[1], owned[1], owned[0])):
        st, ref = fresh(torch_cuda, gt, halo=halo)
        # a block of this shard with a neighbour in the other: that neighbour is absent here, never halo
        for target in sorted(mine):
            foreign = {tuple(a + b for a, b in zip(target, o)) for o in R.halo_offsets(halo)} & other
            if foreign:
                flips(torch_cuda, gt, st, ref, target, halo, expect_foreign=foreign)
                seen += 1
                break
        # a deleted key is removed here whatever the other shard holds
        gone = sorted(mine)[0]
        gt.delete_blocks(keys4(torch_cuda, [gone]))
        ch, rm, ok = call(torch_cuda, gt, st, ref, halo=halo)
        assert rm == [gone]
    assert seen >= 1
    for s in shards:
        s.close()


def free_key(gt, cfg, like):
    """A key far from the model whose home bucket is empty in this table."""
    nb, bs, _, _ = cfg
    e = gt.hash_table()
    used = set((np.nonzero(e["ptr"] != -1)[0] // bs).tolist())
    for x in range(100, 400):
        k = (x, like[1], like[2])
        if int(mm.hash_block([k], nb)[0]) not in used:
            return k
    raise AssertionError("no free bucket")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_deleted_restored_and_rekeyed(vh, torch_cuda, cfg):
    torch = torch_cuda
    gt = table(vh, cfg)
    st, ref = fresh(torch, gt, halo=R.HALO_NORMALS)
    vox, col = bits_of(gt, CENTRE)
    around = {tuple(a + b for a, b in zip(CENTRE, o)) for o in R.halo_offsets(R.HALO_NORMALS)}
    # deleted: removed, and its halo listed
    gt.delete_blocks(keys4(torch, [CENTRE]))
    ch, rm, ok = call(torch, gt, st, ref, halo=R.HALO_NORMALS)
    assert rm == [CENTRE] and set(ch) == around & set(held(gt)) and set(ch.values()) == {R.HALO}
    # deleted and streamed in again before the next call, the same bits: not removed; self-changed only if it changed slot
    ch, rm, ok = call(torch, gt, st, ref, halo=R.HALO_NONE)
    assert not ch and not rm
    gt.stream_in({"keys": np.array([CENTRE], np.int32), "voxels": vox.reshape(1, 512), "colors": col.reshape(1, 512)})
    ch, rm, ok = call(torch, gt, st, ref, halo=R.HALO_NONE)
    assert ch == {CENTRE: R.SELF} and not rm                         # (its slot was emptied: a block the state has not seen)
    replace(torch, gt, CENTRE, vox, col)                            # the same bits again: never removed
    assert not call(torch, gt, st, ref, halo=R.HALO_NONE)[1]
    vox2 = vox.copy()
    vox2["sdf"][17] += F(1.0)
    replace(torch, gt, CENTRE, vox2, col)                           # delete, then stream_in the same key
    ch, rm, ok = call(torch, gt, st, ref, halo=R.HALO_NONE)
    assert ch == {CENTRE: R.SELF} and not rm
    # K1 deleted, K2 streamed in with K1's very bits: it takes K1's pool slot -- K1 removed, K2 self-changed
    ptr_of = lambda k: int(gt.allocated()["ptr"][held(gt).index(k)])
    k1, p1 = (-1, 0, 0), None
    p1 = ptr_of(k1)
    v1, c1 = bits_of(gt, k1)
    k2 = free_key(gt, cfg, k1)
    gt.delete_blocks(keys4(torch, [k1]))
    assert gt.stream_in({"keys": np.array([k2], np.int32), "voxels": v1.reshape(1, 512), "colors": c1.reshape(1, 512)})["placed"] == 1
    assert ptr_of(k2) == p1                                          # (the heap hands the freed block out first)
    ch, rm, ok = call(torch, gt, st, ref, halo=R.HALO_NONE)
    assert rm == [k1] and ch == {k2: R.SELF}
    slot = ref.slots[p1 >> 9]
    assert slot["live"] and tuple(slot["key"].tolist()) == k2
    gt.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_a_capacity_one_short_commits_nothing(vh, torch_cuda, cfg):
    torch = torch_cuda
    gt = table(vh, cfg)
    st, ref = fresh(torch, gt)
    vox, col = bits_of(gt, CENTRE)
    vox["weight"][3] += F(1.0)
    replace(torch, gt, CENTRE, vox, col)
    gt.delete_blocks(keys4(torch, [(5, 5, 5)]))
    before = state_bytes(st)
    peek = call(torch, gt, st, ref, caps=(0, 0))
    nc, nr = len(peek[0]), len(peek[1])
    assert not peek[2] and nc >= 2 and nr == 1                       # the centre, its halo; the deleted key
    for caps in ((nc - 1, nr), (nc, nr - 1), (nc - 1, nr - 1)):
        got = call(torch, gt, st, ref, caps=caps)
        assert not got[2] and got[:2] == peek[:2] and state_bytes(st) == before
    full = call(torch, gt, st, ref, caps=(nc, nr))
    assert full[2] and full[:2] == peek[:2] and state_bytes(st) != before
    assert call(torch, gt, st, ref)[:2] == ({}, [])
    gt.close()


@pytest.mark.parametrize("cfg", [CONFIGS[3], CONFIGS[4]], ids=[IDS[3], IDS[4]])
def test_a_region(vh, torch_cuda, cfg):
    torch = torch_cuda
    gt = table(vh, cfg)
    st, ref = fresh(torch, gt)
    far = (5, 5, 5)
    for k in (CENTRE, far):
        vox, col = bits_of(gt, k)
        vox["sdf"][100] = -vox["sdf"][100] if vox["sdf"][100] != 0 else F(1)
        replace(torch, gt, k, vox, col)
    region = ((0, 0, 0), (2, 2, 2))                                 # the centre at its corner: its halo lies one block outside
    ch, rm, ok = call(torch, gt, st, ref, region=region, halo=R.HALO_MESH)
    assert ch[CENTRE] == R.SELF and far not in ch and not rm
    outside = [k for k in ch if not R.holds(region, k)]
    assert outside and all(ch[k] == R.HALO for k in outside) and (-1, 0, 0) in outside
    assert call(torch, gt, st, ref, region=region)[:2] == ({}, [])
    ch, rm, ok = call(torch, gt, st, ref, halo=R.HALO_MESH)         # what lay outside was still pending
    assert ch[far] == R.SELF and CENTRE not in ch and (5, 5, 6) not in ch
    # a region at the ends of int32 lists what a grown region without saturation would lose
    ch, rm, ok = call(torch, gt, st, ref, region=((R.INT32_MIN,) * 3, (R.INT32_MAX,) * 3))
    assert not ch and not rm
    gt.close()


def test_colour_counts_only_when_asked(vh, torch_cuda):
    torch = torch_cuda
    gt = table(vh, CONFIGS[4])
    st, ref = fresh(torch, gt, color=False)
    stc, refc = fresh(torch, gt, color=True)
    assert state_bytes(st)[64:] != state_bytes(stc)[64:]            # `what` is part of the digest
    vox, col = bits_of(gt, CENTRE)
    col[511] ^= U(0x80000000)
    replace(torch, gt, CENTRE, vox, col)
    # (the block kept its pool slot, so the voxel digest finds nothing)
    assert call(torch, gt, st, ref, color=False, halo=R.HALO_NONE)[:2] == ({}, [])
    assert call(torch, gt, stc, refc, color=True, halo=R.HALO_NONE)[:2] == ({CENTRE: R.SELF}, [])
    # a table without a colour volume: every colour word counts as 0
    plain = vh.SDFHashtable(vh.default_params(numBuckets=64, bucketSize=2, numVoxelBlocks=64), 64, 48, 1)
    c = chunk([(0, 0, 0), (1, 0, 0)])
    c["colors"] = None
    plain.stream_in(c)
    assert not plain.has_color()
    fresh(torch, plain, color=True)
    plain.close()
    gt.close()


def test_a_pending_pipelined_frame_is_in_the_answer(oracle, vh, torch_cuda):
    import deintegrate_cases as DC
    import merge_color_cases as CC
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = CC.table(vh, DC.KW, 1)
    gt.set_option("pipeline", 1)
    gt.integrate(frames[0][0], CC.dev(torch, frames[0][2]))
    st = gt.changes_state()
    first, _ = gt.changes(st, halo="none")
    had = set(held(gt))
    assert len(first) == len(had) > 20
    gt.integrate(frames[1][0], CC.dev(torch, frames[1][2]))         # with "pipeline" its commit + TSDF update stay pending
    ref = R.State.frombytes(state_bytes(st))
    ch, rm = gt.changes(st, halo="none")                            # launches the pending half first
    ch, rm = ch.cpu().numpy(), rm.cpu().numpy()
    wc, wr, _ = R.changes(gt.hash_table(), gt.sdf_blocks(), None, ref, None, R.VOXELS, R.HALO_NONE)
    assert np.array_equal(ch, wc) and np.array_equal(rm, wr) and state_bytes(st) == ref.tobytes()
    new = set(held(gt)) - had
    assert new and new <= {tuple(r[:3]) for r in ch.tolist()}
    gt.close()


def test_a_view_table_is_refused_and_argument_errors(vh, torch_cuda):
    torch = torch_cuda
    model = mm.uniform_model(mm.cube_keys(0, 2), 3)
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=64, bucketSize=4, numVoxelBlocks=1), 64, 48, 1)
    view.import_view(rec, len(model))
    lib, nc, nr = view._lib, C.c_uint64(), C.c_uint64()
    st = torch.zeros((64 + 32 * 64,), dtype=torch.uint8, device="cuda")
    assert lib.vh_changes(view._h, st.data_ptr(), None, 1, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1
    assert b"view" in lib.vh_last_error()
    assert lib.vh_changes_host(view._h, st.data_ptr(), None, 1, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1
    view.close()
    gt = table(vh, CONFIGS[4])
    st = gt.changes_state()
    buf = torch.zeros((256, 4), dtype=torch.int32, device="cuda")
    ok = lambda *a: lib.vh_changes(*a)
    h, s, b = gt._h, st.data_ptr(), buf.data_ptr()
    assert ok(None, s, None, 1, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1
    assert ok(h, None, None, 1, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1
    assert ok(h, s, None, 1, 1, 0, None, 0, None, None, C.byref(nr)) == 1
    assert ok(h, s, None, 1, 1, 0, None, 0, None, C.byref(nc), None) == 1
    assert ok(h, s, None, 0, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1          # no VH_CHANGES_VOXELS
    assert ok(h, s, None, 2, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1
    assert ok(h, s, None, 5, 1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1          # an unknown bit
    assert ok(h, s, None, 1, 3, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1          # an unknown halo
    assert ok(h, s, None, 1, -1, 0, None, 0, None, C.byref(nc), C.byref(nr)) == 1
    assert ok(h, s, None, 1, 1, 4, None, 0, None, C.byref(nc), C.byref(nr)) == 1          # a capacity without its buffer
    assert ok(h, s, None, 1, 1, 0, None, 4, None, C.byref(nc), C.byref(nr)) == 1
    assert not st.any()                                                                    # none of them touched the state
    n = C.c_uint64()
    assert lib.vh_changes_state_bytes(h, C.byref(n)) == 0 and n.value == 64 + 32 * 256
    assert lib.vh_changes_state_bytes(h, None) == 1 and lib.vh_changes_state_bytes(None, C.byref(n)) == 1
    # the host form gives the device form's lists
    want_c, want_r = gt.changes(gt.changes_state(), halo="normals")
    hc, hr = np.zeros((256, 4), np.int32), np.zeros((256, 4), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vh_changes_host(h, s, None, 1, 2, 256, vp(hc), 256, vp(hr), C.byref(nc), C.byref(nr)) == 0
    assert nc.value == len(want_c) > 0 and nr.value == 0 and np.array_equal(hc[:nc.value], want_c.cpu().numpy())
    gt.close()
