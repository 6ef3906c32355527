"""vh_components / vh_remove_components on the GPU against the rule in executable form (tests/components_ref.py, pinned by
tests/test_components_ref_cpu.py): records, stats and label lattices bit for bit on the table as placed, on models the tests
choose themselves (tests/components_cases.py, tests/mesh_models.py) and on tables the frame path filled.  Every case asserts,
on the reference's own answer, a condition without which it could pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import components_cases as cc
import components_ref as cr
import mesh_models as mm
from test_gpu_gc import frames, pair, same_state
from test_gpu_mesh import fuse, shard_pair, table_of

pytestmark = pytest.mark.gpu
F = np.float32
BOTH = [(t, c) for t in (cr.INSIDE, cr.OUTSIDE) for c in (6, 14)]
# two placements of one model: the block ids are dealt by the seed, the entry order follows the hash modulo the bucket count
PLACEMENTS = ((0, dict(numBuckets=509, bucketSize=8)), (1, dict(numBuckets=1021, bucketSize=8)))


def placed(vh, model, tmp_path, placement=0, **kw):
    seed, table = PLACEMENTS[placement]
    params = dict(table, numVoxelBlocks=len(model) + 11)
    params.update(kw)
    gt = vh.SDFHashtable(vh.default_params(**params), 640, 480, 1)
    return mm.load_model(gt, model, tmp_path, seed)


def model_and_order(gt):
    table = gt.hash_table()
    return mm.model_of(table, gt.sdf_blocks()), cr.order_of(table)


def same_as_reference(gt, model, order, target, connectivity, region=None, box=None):
    """Records, stats and (with box = (lo, dims)) labels against the rule on the table as placed; returns the rule's answer."""
    want = cr.label(model, order, target, connectivity, region)
    rec, lab, stats = gt.components(region, target, connectivity, box)
    assert stats == want.stats, (stats, want.stats)
    assert rec.dtype == cr.RECORD and np.array_equal(rec, want.records), f"records differ (target {target}, connectivity {connectivity})"
    if box is not None:
        got = lab.cpu().numpy().view(np.uint32)
        ref = want.labels(*box)
        assert got.shape == ref.shape and np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} labels differ"
    return want


def box_of(model, grow=3):
    """A box across the block seams of the model's first blocks that leaves the model on the low side."""
    keys = np.array(list(model), np.int64)
    lo = keys.min(0) * 8 - grow
    return tuple(int(v) for v in lo), (21, 19, 14)


# ---- 1. parity on every model, both placements ---------------------------------------------------------------------------
MODELS = {
    "offsets": lambda: cc.offsets()[0],
    "offsets_outside": lambda: cc.offsets(True)[0],
    "serpentine": cc.serpentine,
    "serpentine_outside": lambda: cc.serpentine(True),
    "sparse30": lambda: cc.sparse(0.30),
    "sparse16": lambda: cc.sparse(0.16),
    "holes": lambda: mm.holes(0),
    "zeros": mm.zeros,
    "non_finite": mm.non_finite,
    "weights": mm.weights,
    "every_configuration": mm.every_configuration,
}


@pytest.mark.parametrize("name", list(MODELS))
def test_parity(vh, torch_cuda, tmp_path, name):
    model = MODELS[name]()
    box = box_of(model)
    answers = []
    for placement in (0, 1):
        gt = placed(vh, model, tmp_path, placement)
        order = cr.order_of(gt.hash_table())
        answers.append([same_as_reference(gt, model, order, t, c, box=box) for t, c in BOTH])
        gt.close()
    orders_differ = False
    for a, b in zip(*answers):
        ga, ca = a.canonical()
        gb, cb = b.canonical()
        assert np.array_equal(ga, gb) and np.array_equal(ca, cb)                                   # the partition
        assert np.array_equal(np.sort(a.records["size"]), np.sort(b.records["size"]))             # the sizes
        orders_differ |= not np.array_equal(a.records["voxel"], b.records["voxel"])
    if max(len(a.records) for a in answers[0]) > 50:                 # (one component has one order; its root moves with block (0, 0, 0))
        assert orders_differ                                         # ... while the table decides the order
    inside14, inside6 = answers[0][1], answers[0][0]
    print(f"{name}: {[(w.stats['nodes'], w.stats['components'], w.stats['largest']) for w in answers[0]]}")
    assert sum(int((w.labels(*box) != cr.NONE).sum()) for w in answers[0]) > 100 and (inside14.labels(*box) == cr.NONE).sum() > 100
    if name.startswith("offsets"):
        target = cr.OUTSIDE if name.endswith("outside") else cr.INSIDE
        for conn, lab in zip((6, 14), answers[0][2 * target:2 * target + 2]):
            for p in cc.offsets()[1]:
                ia, ib = (lab.index[lab.rank[tuple(c >> 3 for c in g)]][cc.index(*g)] for g in (p["A"], p["B"]))
                assert ia != cr.NONE and ib != cr.NONE and (ia == ib) == p[f"joined{conn}"], (p, conn)
    if name.startswith("serpentine"):
        t = 2 if name.endswith("outside") else 0
        for lab in answers[0][t:t + 2]:
            assert lab.stats["components"] == 1 and lab.stats["nodes"] == cc.SERPENTINE_NODES and lab.blocks_of()[0] == 36
        other = answers[0][2 - t]                                    # the sea at 6
        assert other.stats["components"] == 1 and other.stats["nodes"] == cc.SERPENTINE_REST
    if name.startswith("sparse"):
        lab = inside6 if name == "sparse30" else inside14
        assert lab.stats["components"] >= 400 and (lab.blocks_of() > 1).sum() >= 50 and lab.stats["largest"] <= 0.2 * lab.stats["nodes"]
    if name == "every_configuration":
        assert inside6.stats["components"] >= 205 and inside14.stats["components"] >= 2 and inside14.blocks_of().max() == 27
    if name == "zeros":                                              # +-0 is inside
        zero = sum(int(((s == 0) & (w > 0)).sum()) for s, w in model.values())
        assert zero > 100 and inside14.stats["nodes"] >= zero
    if name == "non_finite":                                         # -inf is inside, a NaN sdf is no node of either target
        nan = sum(int((np.isnan(s) & (w > 0)).sum()) for s, w in model.values())
        valid = sum(int(((w > 0)).sum()) for s, w in model.values())
        ninf = sum(int((np.isneginf(s) & (w > 0)).sum()) for s, w in model.values())
        assert nan > 10 and ninf > 10 and inside14.stats["nodes"] + answers[0][3].stats["nodes"] == valid - nan


# ---- 2. capacity, guards, each output alone --------------------------------------------------------------------------
def test_capacity_and_guards(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    model = cc.sparse(0.30)
    gt = placed(vh, model, tmp_path)
    order = cr.order_of(gt.hash_table())
    want = cr.label(model, order, cr.INSIDE, 6)
    n = want.stats["components"]
    assert n > 400
    lo, dims = box_of(model)
    ref = want.labels(lo, dims)
    voxels, guard = int(np.prod(dims)), 1024
    assert gt.components_into(0, None, target="inside", connectivity=6) == want.stats       # count only
    rec = torch.full((n + 2 * guard, 4), -77, dtype=torch.int32, device="cuda")
    lab = torch.full((voxels + 2 * guard,), -77, dtype=torch.int32, device="cuda")
    clip = 100
    assert (ref.astype(np.int64)[ref != cr.NONE] >= clip).any()      # labels that index beyond the capacity
    for cap, use_lab in ((n, True), (clip, True), (clip, False), (0, True), (n + 50, False)):
        rec.fill_(-77)
        lab.fill_(-77)
        stats = gt.components_into(cap, rec[guard:guard + cap] if cap else None, lo if use_lab else None, dims if use_lab else None,
                                   lab[guard:guard + voxels] if use_lab else None, target="inside", connectivity=6)
        assert stats == want.stats
        hr, hl = rec.cpu().numpy(), lab.cpu().numpy()
        wrote = min(cap, n)
        assert (hr[:guard] == -77).all() and (hr[guard + wrote:] == -77).all()
        assert np.array_equal(hr[guard:guard + wrote].copy().view(cr.RECORD).reshape(-1), want.records[:wrote])
        assert (hl[:guard] == -77).all() and (hl[guard + voxels:] == -77).all()
        if use_lab:
            assert np.array_equal(hl[guard:guard + voxels].view(np.uint32), ref.reshape(-1))
        else:
            assert (hl == -77).all()
    gt.close()


# ---- 3. regions ------------------------------------------------------------------------------------------------------
def test_regions(vh, torch_cuda, tmp_path):
    model = cc.serpentine()
    gt = placed(vh, model, tmp_path)
    order = cr.order_of(gt.hash_table())
    # blocks x 2..3: the twelve rows cut at both sides, the turns lie outside: 12 pieces of 16 voxels
    region = ((2, 0, 0), (4, 6, 1))
    want = same_as_reference(gt, model, order, cr.INSIDE, 14, region, box=((10, -2, 0), (30, 52, 6)))
    assert want.stats["components"] == 12 and want.stats["blocks"] == 12 and (want.records["size"] == 16).all()
    # blocks x 0..2: the turns at x = 0 stay: row pairs (5, 9), (13, 17) ... joined, rows 1 and 45 alone: 7 pieces
    want = same_as_reference(gt, model, order, cr.INSIDE, 6, ((0, 0, 0), (3, 6, 1)))
    assert want.stats["components"] == 7 and sorted(want.records["size"].tolist()) == [24, 24] + [51] * 5
    # an empty region: nothing listed
    for region in (((2, 0, 0), (2, 6, 1)), ((50, 50, 50), (60, 60, 60))):
        rec, lab, stats = gt.components(region, "inside", 14, ((0, 0, 0), (9, 9, 5)))
        assert len(rec) == 0 and not any(stats.values()) and (lab.cpu().numpy() == -1).all()
    gt.close()
    model = cc.sparse(0.30)
    gt = placed(vh, model, tmp_path)
    order = cr.order_of(gt.hash_table())
    whole = cr.label(model, order, cr.INSIDE, 6)
    big = int(np.argmax(whole.blocks_of()))
    assert whole.blocks_of()[big] >= 3
    rows = np.nonzero((whole.index == big).any(1))[0]
    keys = np.array(whole.keys)[rows]
    axis = int(np.argmax(keys.max(0) - keys.min(0)))
    lo, hi = [mm.INT32_MIN] * 3, [mm.INT32_MAX] * 3
    hi[axis] = int(keys[:, axis].max())                              # the component's last blocks along that axis fall outside
    want = same_as_reference(gt, model, order, cr.INSIDE, 6, (lo, hi), box=box_of(model))
    assert want.stats["blocks"] < len(model) and want.stats["nodes"] < whole.stats["nodes"]
    kept = whole.records["size"][big] - int((whole.index[rows][keys[:, axis] == hi[axis]] == big).sum())
    root = whole.records["voxel"][big]
    assert 0 < kept < whole.records["size"][big]
    pieces = want.records[[tuple(v) in {tuple(g) for g in whole_voxels(whole, big)} for v in want.records["voxel"].tolist()]]
    assert len(pieces) >= 1 and pieces["size"].sum() == kept, (root, pieces)
    gt.close()


def whole_voxels(lab, comp):
    r, c = np.nonzero(lab.index == comp)
    return (np.array(lab.keys, np.int64)[r] * 8 + cr.LOCAL[c]).tolist()


# ---- 4. tables -------------------------------------------------------------------------------------------------------
def test_two_shards(vh, torch_cuda):
    shards = shard_pair(vh, torch_cuda)
    cut = 0
    for sh, other in zip(shards, shards[::-1]):
        model, order = model_and_order(sh.table)
        theirs = set(cr.order_of(other.table.hash_table()))
        assert not set(model) & theirs
        k0 = next(k for k in sorted(model) if (k[0] + 1, k[1], k[2]) in theirs)       # a face neighbour in the other shard
        for t, c in ((cr.INSIDE, 14), (cr.OUTSIDE, 6)):
            want = same_as_reference(sh.table, model, order, t, c, box=(tuple(v * 8 - 3 for v in k0), (22, 14, 13)))
            assert want.stats["nodes"] > 1000
        # the same voxels with the other shard's blocks present join more: the seam did cut
        both = dict(model)
        both.update(model_and_order(other.table)[0])
        cut += cr.label(both, None, cr.OUTSIDE, 6).stats["components"] < sum(
            cr.label(m, None, cr.OUTSIDE, 6).stats["components"] for m in (model, model_and_order(other.table)[0]))
    assert cut
    for sh in shards:
        sh.table.close()


def test_overflow_list_chains(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096,
                                   attachedLinkedListSize=8))
    table = gt.hash_table()
    assert (table["offset"] != 0).sum() > 20                         # chains did form
    model, order = model_and_order(gt)
    key = order[len(order) // 2]
    for t, c in BOTH:
        want = same_as_reference(gt, model, order, t, c, box=(tuple(v * 8 - 2 for v in key), (20, 19, 18)))
        assert want.stats["nodes"] > 1000 and want.blocks_of().max() > 3
    gt.close()


def test_view_table(vh, torch_cuda):
    torch = torch_cuda
    model = mm.every_configuration()
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), 640, 480, 1)
    view.import_view(rec, len(model))
    order = cr.order_of(view.hash_table())
    for t, c in BOTH:
        want = same_as_reference(view, model, order, t, c, box=((-2, 5, 3), (20, 17, 9)))
        assert want.stats["blocks"] == 27 and want.stats["nodes"] > 5000
    with pytest.raises(vh.VoxelHashError):
        view.remove_components(5)
    view.close()


def test_sees_queued_frames_and_changes_nothing(vh, torch_cuda):
    torch = torch_cuda
    plain = fuse(torch, table_of(vh, 1))
    model, order = model_and_order(plain)
    gt = table_of(vh, 1)
    fr = frames(6)
    keep = [torch.from_numpy(v).cuda() for _, v in fr]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([q for q, _ in fr[:5]], keep[:5])
    gt.integrate(fr[5][0], keep[5])                                  # pipelined: its second half is still pending, no flush
    key = order[len(order) // 2]
    box = (tuple(v * 8 - 9 for v in key), (37, 30, 21))
    want = cr.label(model, order, cr.INSIDE, 14)
    before = gt.components(None, "inside", 14, box)
    gt.flush()
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    after = gt.components(None, "inside", 14, box)
    for rec, lab, stats in (before, after):
        assert stats == want.stats and np.array_equal(rec, want.records)
        assert np.array_equal(lab.cpu().numpy().view(np.uint32), want.labels(*box))
    assert want.stats["components"] > 3 and want.stats["largest"] > 1000
    assert state(gt) == s0 and sorted(model_and_order(gt)[1]) == sorted(order)
    gt.close()
    plain.close()


# ---- 5. more listed blocks than one scan tile ------------------------------------------------------------------------
def test_many_blocks(vh, torch_cuda, tmp_path):
    model = mm.many_blocks()
    gt = placed(vh, model, tmp_path, numBuckets=mm.MANY_BUCKETS, bucketSize=mm.MANY_BUCKET_SIZE)
    order = cr.order_of(gt.hash_table())
    want = cr.label(model, order, cr.INSIDE, 14)
    box = ((94, -3, -6), (21, 10, 9))                                # the sphere passes through it
    rec, lab, stats = gt.components(None, "inside", 14, box)
    assert stats["blocks"] == mm.MANY_BLOCKS > 24 * 1024 and stats["components"] == want.stats["components"] >= 1
    assert np.array_equal(rec, want.records) and want.stats["largest"] > 3000000
    ref = want.labels(*box)
    assert np.array_equal(lab.cpu().numpy().view(np.uint32), ref) and (ref == cr.NONE).any() and (ref != cr.NONE).any()
    gt.close()


def test_more_than_one_tile_of_slices(vh, torch_cuda, tmp_path):
    """The list walk over 2 048 slices, two tiles of the slice scan: a box that cuts the ball of mesh_models.many_slices, and
    no region."""
    gt = mm.many_slices_table(vh, tmp_path)
    table = gt.hash_table()
    model, order = mm.model_of(table, gt.sdf_blocks()), cr.order_of(table)
    live = np.nonzero(table["ptr"] != -1)[0]
    lo = np.array(mm.SLICE_BALL_LO)
    box = (tuple(int(v) for v in lo + (4, 0, 2)), tuple(int(v) for v in lo + (9, 12, 40)))
    for region in (box, None):
        want = same_as_reference(gt, model, order, cr.INSIDE, 14, region)
        listed = live[[k in want.rank for k in order]]
        print(f"region {region}: {want.stats}")
        assert len(listed) == want.stats["blocks"] and mm.in_both_slice_tiles(listed) and want.stats["components"] >= 1
        if region is None:
            assert len(listed) == len(live) and (listed // 2 == mm.SLICE_BUCKETS - 1).sum() == 2
            assert want.stats["components"] > 1500                    # (the lone blocks: a piece each)
        else:
            assert 500 < len(listed) < 12 ** 3 and mm.in_both_slice_tiles(np.setdiff1d(live, listed))
    gt.close()


# ---- 6. removal ------------------------------------------------------------------------------------------------------
def heap_is_sound(gt):
    c, table = gt.counters(), gt.hash_table()
    live = table["ptr"][table["ptr"] != -1] // 512
    free = gt.heap()[:c["heap_counter"] + 1]
    n = gt.params.numVoxelBlocks
    assert sorted(live.tolist() + free.tolist()) == list(range(n))
    assert not gt.sdf_blocks().view(np.uint32).reshape(n, 1024)[free].any()
    return len(live)


def same_model(gt, want):
    got = mm.model_of(gt.hash_table(), gt.sdf_blocks())
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k][0].view(np.uint32), want[k][0].view(np.uint32)), k
        assert np.array_equal(got[k][1].view(np.uint32), want[k][1].view(np.uint32)), k


def with_floaters(model):
    """The model plus a block that holds only a floater of one voxel, one that holds only a floater of 5 voxels, and a block
    of weight 0 (empty before any call).  Returns (model, the three keys)."""
    out = {k: (s.copy(), w.copy()) for k, (s, w) in model.items()}
    top = np.array(list(out), np.int64).max(0)
    far1, far5, empty = (tuple(int(v) for v in top + (3 * i, 0, 0)) for i in (1, 2, 3))
    for key, n in ((far1, 1), (far5, 5), (empty, 0)):
        s, w = np.zeros(512, F), np.zeros(512, F)
        for x in range(n):
            s[cc.index(2 + x, 4, 4)], w[cc.index(2 + x, 4, 4)] = -0.5, 1.0
        out[key] = (s, w)
    return out, far1, far5, empty


@pytest.mark.parametrize("min_size", (2, 8, 10**9))
@pytest.mark.parametrize("kind", ("sparse", "fused"))
def test_removal(vh, torch_cuda, tmp_path, kind, min_size):
    torch = torch_cuda
    if kind == "sparse":
        base = cc.sparse(0.30)
    else:
        src = fuse(torch, table_of(vh, 1), 3)
        base = mm.model_of(src.hash_table(), src.sdf_blocks())
        src.close()
    model, far, far5, empty = with_floaters(base)
    gt = placed(vh, model, tmp_path, numBuckets=1 << 12, bucketSize=8)
    order = cr.order_of(gt.hash_table())
    # colour: a word per voxel so that clearing shows (set through the volume's file)
    want, wstats, cleared, freed = cr.remove(model, min_size, order, cr.INSIDE, 14)
    assert far in freed and (far5 in freed) == (min_size >= 8) and wstats["freed_blocks"] > 0 and empty in want
    assert wstats["removed_components"] > 0 and (min_size == 10**9 or wstats["removed_components"] < wstats["components"])
    entries = heap_is_sound(gt)
    c0 = gt.counters()
    stats = gt.remove_components(min_size, None, "inside", 14)
    assert stats == wstats, (stats, wstats)
    same_model(gt, want)
    assert empty in mm.model_of(gt.hash_table(), gt.sdf_blocks())   # a block that was empty before stays
    c = gt.counters()
    assert c["last_freed"] == len(freed) and c["freed_total"] == c0["freed_total"] + len(freed)
    assert heap_is_sound(gt) == entries - len(freed) and c["occupied"] == 0
    # a second call removes nothing; no component below min_size is left
    again = gt.remove_components(min_size, None, "inside", 14)
    assert again["removed_voxels"] == 0 and again["freed_blocks"] == 0 and gt.counters()["last_freed"] == 0
    same_model(gt, want)
    rec, _, after = gt.components(None, "inside", 14)
    assert after["components"] == wstats["components"] - wstats["removed_components"]
    assert len(rec) == 0 or rec["size"].min() >= min_size
    # the other class is untouched
    for k, (s, w) in want.items():
        keep = ~cr.node_mask(model[k][0], model[k][1], cr.INSIDE)
        assert np.array_equal(s[keep].view(np.uint32), model[k][0][keep].view(np.uint32))
    # the mesh and the ESDF no longer contain the floater
    fb = ((far[0], far[1], far[2]), (far[0] + 1, far[1] + 1, far[2] + 1))
    assert gt.mesh_count(fb) == 0
    d2 = gt.esdf_lattice(tuple(v * 8 for v in far), (8, 8, 8), 3, dist2=True, distance=False).cpu().numpy()
    assert (d2 == -2**31).all()                                      # unknown: nothing is there any more
    gt.close()


def test_removal_clears_colour_and_the_table_goes_on(vh, torch_cuda):
    torch = torch_cuda
    gt = table_of(vh, 1)
    fr = frames(4)
    rgba = torch.full((240, 320), 0x00804020, dtype=torch.int32, device="cuda")
    for pose, verts in fr[:3]:
        v = torch.from_numpy(verts).cuda()
        gt.integrate(pose, v)
        gt.integrate_color_map(pose, v, rgba, 0.1)
    model, order = model_and_order(gt)
    table0, colour0 = gt.hash_table(), gt.color_volume()
    EVERY = 10**9                                                    # (a room fused from clean depth has no floaters: every inside piece goes)
    want, wstats, cleared, freed = cr.remove(model, EVERY, order, cr.INSIDE, 14)
    coloured = sum(int((colour0[int(e["ptr"]):int(e["ptr"]) + 512][cleared[tuple(e["pos"].tolist())]] != 0).sum())
                   for e in table0[table0["ptr"] != -1] if tuple(e["pos"].tolist()) in cleared)
    assert wstats["removed_voxels"] > 20 and coloured > 0            # cleared voxels that did hold a colour
    assert gt.remove_components(EVERY) == wstats
    same_model(gt, want)
    colour = gt.color_volume()
    for e in table0[table0["ptr"] != -1]:
        k, p = tuple(e["pos"].tolist()), int(e["ptr"])
        gone = cleared.get(k, np.zeros(512, bool))
        if k in freed:
            assert not colour[p:p + 512].any()
        else:
            assert not colour[p:p + 512][gone].any() and np.array_equal(colour[p:p + 512][~gone], colour0[p:p + 512][~gone])
    # the table goes on: the next frame allocates and fuses as on a table that was loaded with the reference's removal
    heap_is_sound(gt)
    other = table_of(vh, 1)
    for pose, verts in fr[:3]:
        other.integrate(pose, torch.from_numpy(verts).cuda())
    assert other.remove_components(EVERY) == wstats
    for t in (gt, other):
        t.integrate(fr[3][0], torch.from_numpy(fr[3][1]).cuda())
    a, b = (mm.model_of(t.hash_table(), t.sdf_blocks()) for t in (gt, other))
    assert sorted(a) == sorted(b) and len(a) > len(want) - 1 and heap_is_sound(gt) == len(a)
    for k in a:
        assert np.array_equal(a[k][0].view(np.uint32), b[k][0].view(np.uint32))
    gt.close()
    other.close()


def test_frame_after_removal_against_the_oracle(oracle, vh, torch_cuda):
    """The oracle has no removal, so the reference's is written into its volume (the cleared voxels) and table (the freed
    blocks: its delete_blocks); from there on the two tables must stay equal through the next frames, as in test_gpu_gc.py."""
    torch = torch_cuda
    ot, gt = pair(oracle, vh, "fused-indexed-walk", numBuckets=1 << 12, numVoxelBlocks=8192)
    fr = frames(8)
    for pose, verts in fr[:6]:
        ot.integrate(pose, verts)
        gt.integrate(pose, torch.from_numpy(verts).cuda())
    same_state(ot, gt)
    model, order = model_and_order(gt)
    big = int(cr.label(model, order, cr.INSIDE, 14).stats["largest"])
    want, wstats, cleared, freed = cr.remove(model, big, order, cr.INSIDE, 14)          # every inside piece but the largest
    assert wstats["removed_voxels"] > 20 and wstats["removed_components"] == wstats["components"] - 1
    vol = ot.sdf_blocks()
    for e in ot.allocated():
        gone = cleared.get(tuple(int(c) for c in e["pos"]))
        if gone is not None:
            at = int(e["ptr"]) + np.nonzero(gone)[0]
            vol["sdf"][at] = 0
            vol["weight"][at] = 0
    assert ot.delete_blocks(freed) == len(freed)
    assert gt.remove_components(big, None, "inside", 14) == wstats
    n = same_state(ot, gt)
    assert n == len(want)
    for pose, verts in fr[6:]:                                       # the table goes on: allocation and fusion as the oracle's
        ot.integrate(pose, verts)
        gt.integrate(pose, torch.from_numpy(verts).cuda())
    assert same_state(ot, gt) > n
    gt.close()
    ot.close()


# ---- 7. arguments ----------------------------------------------------------------------------------------------------
def test_argument_errors(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    model = mm.lone_block()
    gt = placed(vh, model, tmp_path)
    lib, h = vh.load(), gt._h
    from voxelhashing_demo_amd import _lib as L
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    INVALID = 1
    rec = torch.full((64, 4), -77, dtype=torch.int32, device="cuda")
    lab = torch.full((64,), -77, dtype=torch.int32, device="cuda")
    R, Lb = C.c_void_p(rec.data_ptr()), C.c_void_p(lab.data_ptr())
    st = L.ComponentStats()
    call = lambda t=0, c=14, cap=8, r=R, lo=(40, -24, 16), d=(4, 3, 2), lb=Lb, s=st, ctx=h: \
        lib.vh_components(ctx, None, t, c, cap, r, i3(*lo) if lo else None, i3(*d) if d else None, lb, C.byref(s) if s else None)
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    for t in (-1, 2, 7):
        assert call(t=t) == INVALID
    for c in (0, 4, 8, 18, 26, -6):
        assert call(c=c) == INVALID
    assert call(r=None) == INVALID                                   # a capacity without a buffer
    assert call(lo=None) == INVALID and call(d=None) == INVALID and call(lb=None) == INVALID      # a box given in part
    assert call(d=(4, -3, 2)) == INVALID and call(lo=(2**31 - 3, 0, 0)) == INVALID
    assert call(s=None) == INVALID and call(ctx=None) == INVALID
    for t, c in ((2, 14), (0, 26)):
        assert lib.vh_remove_components(h, None, t, c, 5, C.byref(st)) == INVALID
    assert lib.vh_remove_components(None, None, 0, 14, 5, C.byref(st)) == INVALID
    gt.synchronize()
    assert (rec.cpu().numpy() == -77).all() and (lab.cpu().numpy() == -77).all() and state(gt) == s0
    # and the good calls are good: with everything, without a box, count-only
    want = cr.label(model, None, cr.INSIDE, 6)
    assert want.stats["components"] > 2
    assert call(c=6, cap=64) == 0 and st.as_dict() == want.stats
    n = min(want.stats["components"], 64)
    assert np.array_equal(rec.cpu().numpy()[:n].copy().view(cr.RECORD).reshape(-1), want.records[:n])
    assert np.array_equal(lab.cpu().numpy()[:24].view(np.uint32), want.labels((40, -24, 16), (4, 3, 2)).reshape(-1))
    assert (lab.cpu().numpy()[24:] == -77).all() and (rec.cpu().numpy()[n:] == -77).all()
    assert call(lo=None, d=None, lb=None) == 0 and call(cap=0, r=None, lo=None, d=None, lb=None) == 0
    assert lib.vh_remove_components(h, None, 0, 14, 0, None) == 0 and lib.vh_remove_components(h, None, 0, 14, 1, C.byref(st)) == 0
    assert st.removed_voxels == 0 and state(gt)[:3] == s0[:3]        # min_size 0 or 1 removes nothing
    gt.close()
