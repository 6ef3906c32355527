"""Block streaming on the GPU: vh_stream_out / vh_stream_in against tests/stream_ref.py (the selection rule, the order, the
statuses) and against the calls they are built from (vh_delete_blocks on a twin), bit for bit, and streaming.BlockStore on top.
64x48 frames of the synthetic room, 2^11 buckets, at most 512 blocks (tests/deintegrate_cases.py), two frames coloured twice each
(tests/merge_color_cases.py).  Models are compared per block key: slots may differ after a round trip."""
import ctypes as C

import numpy as np
import pytest

import deintegrate_cases as DC
import merge_color_cases as CC
import mesh_models as mm
import stream_cases as SC
import stream_ref as S
from voxelhashing_demo_amd import streaming

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
VS = SC.VS
INVALID = 1


def keys4(torch, keys):
    k = np.zeros((len(keys), 4), np.int32)
    k[:, :3] = keys
    return CC.dev(torch, k)


def check_chunk(chunk, pre, order):
    """The records are the blocks of entries `order` of the snapshot `pre`, in that order, bit for bit."""
    tab = pre["table"]
    assert np.array_equal(chunk["keys"], tab["pos"][order])
    for i, e in enumerate(tab[order]):
        p = int(e["ptr"])
        assert np.array_equal(chunk["voxels"][i].view(U), pre["vox"][p:p + 512].view(U)), i
        assert np.array_equal(chunk["colors"][i], pre["color"][p:p + 512]), i


def same_state(a, b, compact=False):
    """Two contexts that went through the same calls (or one, before and after): the table, the heap, both volumes and every
    counter, slot for slot.  compact: the bytes of the compact buffer too (one context before and after a call that must not touch
    it; between two contexts its order is an atomic race of the walk that filled it)."""
    CC.unchanged(a, b)
    if compact:
        assert np.array_equal(a["compact"].view(np.uint8), b["compact"].view(np.uint8))


def same_after_removal(a, b, pre, n):
    """`a` after vh_stream_out of n blocks against the twin `b` after vh_delete_blocks of the same keys, both from the state
    `pre`: the table, both volumes and every counter slot for slot.  The heap slot for slot too, except for the ORDER of the n
    slots the call pushed: gc_release_kernel pushes one block per workgroup through an atomic counter, so the order of the freed
    blocks on the heap is a race of the deletion path itself (two twins that both call vh_delete_blocks differ there); those n
    slots are compared as sets."""
    assert np.array_equal(a["table"], b["table"])
    assert np.array_equal(a["vox"].view(U), b["vox"].view(U)) and np.array_equal(a["color"], b["color"])
    assert a["counters"] == b["counters"] and a["has_color"] == b["has_color"]
    top = pre["counters"]["heap_counter"] + 1
    for h in (a["heap"], b["heap"]):
        assert np.array_equal(h[:top], pre["heap"][:top]) and np.array_equal(h[top + n:], pre["heap"][top + n:])
    print(f"pushed slots in the same order: {np.array_equal(a['heap'][top:top + n], b['heap'][top:top + n])}")
    assert sorted(a["heap"][top:top + n].tolist()) == sorted(b["heap"][top:top + n].tolist())
    live = set(a["table"]["ptr"][a["table"]["ptr"] != -1].tolist())
    freed = sorted(int(p) // 512 for p in pre["table"]["ptr"][pre["table"]["ptr"] != -1].tolist() if p not in live)
    assert sorted(a["heap"][top:top + n].tolist()) == freed


def loaded_twins(vh, torch, oracle, sem, tmp_path):
    """Two contexts that are equal slot for slot: both load the snapshot and the colour file of one fused model (which heap block
    a key gets while frames are fused is a race among the frame's winners, so two models fused separately differ in their ptrs)."""
    src = SC.coloured(vh, torch, oracle, sem)
    src.save_snapshot(str(tmp_path / "model.snap"))
    src.save_color(str(tmp_path / "model.color"))
    src.close()
    out = []
    for _ in range(2):
        t = CC.table(vh, DC.KW, sem)
        t.load_snapshot(str(tmp_path / "model.snap"))
        t.load_color(str(tmp_path / "model.color"))
        out.append(t)
    return out


# ---- 1. stream-out against the rule, and against vh_delete_blocks on a twin --------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("kind", ["box", "sphere", "outside"])
def test_stream_out_against_the_rule(oracle, vh, torch_cuda, tmp_path, sem, kind):
    torch = torch_cuda
    gt, twin = loaded_twins(vh, torch, oracle, sem, tmp_path)
    pre = CC.snapshot(gt)
    same_state(pre, CC.snapshot(twin))
    region = SC.regions(SC.live_keys(pre["table"]))[kind]
    order = S.selection_of_table(pre["table"], region, VS)
    total = int((pre["table"]["ptr"] != -1).sum())
    print(f"sem {sem} {kind}: {len(order)} of {total} blocks go")
    assert len(order) >= 8 and total - len(order) >= 8
    assert (pre["color"] != 0).sum() > 1000
    chunk = gt.stream_out(region)
    assert chunk["selected"] == len(order)
    check_chunk(chunk, pre, order)
    twin.delete_blocks(keys4(torch, pre["table"]["pos"][order]))
    post = CC.snapshot(gt)
    same_after_removal(post, CC.snapshot(twin), pre, len(order))
    assert post["counters"]["last_freed"] == len(order) and post["counters"]["occupied"] == 0
    assert post["counters"]["heap_counter"] == pre["counters"]["heap_counter"] + len(order)
    assert post["counters"]["epoch"] == pre["counters"]["epoch"] + 1
    S.same_models(CC.model(post), {k: v for k, v in CC.model(pre).items() if k not in set(map(tuple, chunk["keys"].tolist()))})
    gt.close()
    twin.close()


# ---- 2. the count-only call ------------------------------------------------------------------------------------------------------
def test_count_only_changes_nothing(oracle, vh, torch_cuda):
    gt = SC.coloured(vh, torch_cuda, oracle)
    pre = CC.snapshot(gt)
    for kind, region in SC.regions(SC.live_keys(pre["table"])).items():
        assert gt.stream_count(region) == len(S.selection_of_table(pre["table"], region, VS)), kind
    assert gt.stream_count(SC.EVERYTHING) == int((pre["table"]["ptr"] != -1).sum())
    same_state(CC.snapshot(gt), pre, compact=True)
    gt.close()


# ---- 3. a capacity below the selection -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
def test_capacity_below_the_selection(oracle, vh, torch_cuda, sem):
    gt = SC.coloured(vh, torch_cuda, oracle, sem)
    pre = CC.snapshot(gt)
    region = SC.middle_sphere(SC.live_keys(pre["table"]), invert=True)
    order = S.selection_of_table(pre["table"], region, VS)
    cap = len(order) // 3
    assert cap >= 3
    first = gt.stream_out(region, capacity=cap)
    assert first["selected"] == len(order) and len(first["keys"]) == cap
    check_chunk(first, pre, order[:cap])
    mid = CC.snapshot(gt)
    left = {tuple(k) for k in pre["table"]["pos"][order[cap:]].tolist()}
    assert left <= CC.model(mid).keys() and mid["counters"]["last_freed"] == cap
    second = gt.stream_out(region)
    assert second["selected"] == len(order) - cap == len(second["keys"])
    assert {tuple(k) for k in second["keys"].tolist()} == left
    both = {**SC.chunk_model(first), **SC.chunk_model(second)}
    S.same_models(both, {k: v for k, v in CC.model(pre).items() if k in both})
    assert len(both) == len(order) and gt.stream_count(region) == 0
    gt.close()


# ---- 4. the round trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("variant", [3, 4])
def test_round_trip(oracle, vh, torch_cuda, sem, variant):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt, twin = SC.coloured(vh, torch, oracle, sem), SC.coloured(vh, torch, oracle, sem)
    pre = CC.snapshot(gt)
    live = SC.live_keys(pre["table"])
    rng = np.random.default_rng(7)
    points = CC.dev(torch, ((8.0 * live[rng.integers(0, len(live), 4000)] + rng.uniform(0, 8, (4000, 3))) * VS).astype(F))

    def looks(t):
        out = []
        for pose, _, _ in frames[:2]:
            depth = torch.empty((DC.H, DC.W), dtype=torch.float32, device="cuda")
            t.raycast(pose, depth)
            out.append(depth.view(torch.int32).cpu().numpy())
        sdf, w = t.sample_sdf(points, weight=True)
        return out + [sdf.view(torch.int32).cpu().numpy(), w.view(torch.int32).cpu().numpy()]

    before = looks(gt)
    print(f"sem {sem}: {[(b != 0).sum() for b in before[:2]]} pixels hit, {np.isfinite(before[2].view(F)).sum()} valid samples")
    assert (sem == 0 or (before[0] != 0).sum() > 100) and np.isfinite(before[2].view(F)).sum() > 100
    chunk = gt.stream_out(SC.middle_sphere(live, invert=True))
    n = len(chunk["keys"])
    assert n >= 8 and len(live) - n >= 8
    gone = looks(gt)
    assert any(not np.array_equal(a, b) for a, b in zip(before, gone))          # (the blocks did leave)
    st = gt.stream_in(chunk)
    assert (st["status"] == S.PLACED).all() and st["placed"] == n and st["present"] == st["unplaced"] == st["foreign"] == 0
    assert st["rounds"] >= 1
    post = CC.snapshot(gt)
    S.same_models(CC.model(post), CC.model(pre))
    assert post["counters"]["heap_counter"] == pre["counters"]["heap_counter"] and post["counters"]["occupied"] == 0
    for a, b in zip(before, looks(gt)):
        assert np.array_equal(a, b)
    # the table is whole: the next frame finds its heap, the buckets' prefix property and the occupancy index in order
    for t in (gt, twin):
        t.set_option("flatten_variant", variant)
        t.integrate_depth_color(frames[2][0], CC.dev(torch, frames[2][1]), DC.k_inv(), CC.dev(torch, CC.image(2)), CC.BAND, 255)
    a, b = CC.snapshot(gt), CC.snapshot(twin)
    S.same_models(CC.model(a), CC.model(b))
    assert len(CC.model(a)) > len(CC.model(pre)) and a["counters"]["occupied"] == b["counters"]["occupied"] > 0
    assert a["counters"]["heap_counter"] == b["counters"]["heap_counter"]
    gt.close()
    twin.close()


# ---- 5. everything out -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
def test_everything_out(oracle, vh, torch_cuda, sem):
    torch = torch_cuda
    gt, fresh = SC.coloured(vh, torch, oracle, sem), SC.coloured(vh, torch, oracle, sem)
    pre = CC.snapshot(gt)
    chunk = gt.stream_out(SC.EVERYTHING)
    S.same_models(SC.chunk_model(chunk), CC.model(pre))
    post = CC.snapshot(gt)
    assert (post["table"]["ptr"] == -1).all() and post["counters"]["heap_counter"] == gt.params.numVoxelBlocks - 1
    assert not post["vox"].view(U).any() and not post["color"].any()
    assert sorted(post["heap"].tolist()) == list(range(gt.params.numVoxelBlocks))
    CC.fuse(torch, gt, oracle, CC.SRC_COLORS)
    S.same_models(CC.model(CC.snapshot(gt)), CC.model(CC.snapshot(fresh)))
    gt.close()
    fresh.close()


# ---- 6. statuses -----------------------------------------------------------------------------------------------------------------
def random_chunk(keys, seed, colors=True):
    r = np.random.default_rng(seed)
    n = len(keys)
    vox = np.zeros((n, 512), S.VOXEL)
    vox["sdf"], vox["weight"] = r.standard_normal((n, 512)).astype(F), r.integers(1, 9, (n, 512)).astype(F)
    col = r.integers(1, 1 << 32, (n, 512), dtype=np.uint64).astype(U)
    return {"keys": np.asarray(keys, np.int32).reshape(-1, 3), "voxels": vox, "colors": col if colors else None}


@pytest.mark.parametrize("sem", [0, 1])
def test_present_and_duplicate_records(oracle, vh, torch_cuda, sem):
    gt = SC.coloured(vh, torch_cuda, oracle, sem)
    pre = CC.snapshot(gt)
    held = SC.live_keys(pre["table"])[:12]
    st = gt.stream_in(random_chunk(held, 1))                                      # keys the model holds: not touched
    assert (st["status"] == S.PRESENT).all() and st["present"] == 12 and st["placed"] == st["unplaced"] == st["foreign"] == 0
    mid = CC.snapshot(gt)
    S.same_models(CC.model(mid), CC.model(pre))
    assert mid["counters"]["heap_counter"] == pre["counters"]["heap_counter"]
    # the same key twice in one call, with different contents, between two other records
    new = [(900, 1, -2), (901, 1, -2), (901, 1, -2), (-902, 0, 5)]
    chunk = random_chunk(new, 2)
    st = gt.stream_in(chunk)
    assert st["status"][0] == st["status"][3] == S.PLACED and sorted(st["status"][1:3].tolist()) == [S.PLACED, S.PRESENT]
    assert (st["placed"], st["present"], st["unplaced"], st["foreign"]) == (3, 1, 0, 0)
    post = CC.snapshot(gt)
    model = CC.model(post)
    winner = 1 + st["status"][1:3].tolist().index(S.PLACED)
    want = dict(CC.model(pre))
    for i in (0, winner, 3):
        want[new[i]] = (chunk["voxels"]["sdf"][i], chunk["voxels"]["weight"][i], chunk["colors"][i])
    S.same_models(model, want)                                                    # the placed record is whole, nothing else moved
    assert post["counters"]["heap_counter"] == pre["counters"]["heap_counter"] - 3
    assert post["counters"]["occupied"] == 0
    gt.close()


@pytest.mark.parametrize("sem", [0, 1])
def test_pool_of_eight(oracle, vh, torch_cuda, sem):
    src = SC.coloured(vh, torch_cuda, oracle, sem)
    chunk = src.stream_out(SC.EVERYTHING)
    src.close()
    n = len(chunk["keys"])
    assert n > 16
    small = CC.table(vh, DC.KW, sem, numVoxelBlocks=8)
    st = small.stream_in(chunk)
    assert st["placed"] + st["unplaced"] == n and st["placed"] == 8 and st["present"] == st["foreign"] == 0
    assert (st["status"] == S.PLACED).sum() == 8 and (st["status"] == S.UNPLACED).sum() == n - 8
    snap = CC.snapshot(small)
    assert snap["counters"]["heap_counter"] == -1 and snap["has_color"]
    placed = SC.chunk_model(chunk)
    S.same_models(CC.model(snap), {tuple(k): placed[tuple(k)] for k in chunk["keys"][st["status"] == S.PLACED].tolist()})
    small.close()


def same_bucket_keys(count, buckets):
    """`count` keys of one bucket, found by running through x with the hash of the known-answer vectors (stream_ref.hash_block)."""
    target, out, x = S.hash_block((3, -2, 7), buckets), [], -4000
    while len(out) < count:
        if S.hash_block((x, -2, 7), buckets) == target:
            out.append((x, -2, 7))
        x += 1
    return out


@pytest.mark.parametrize("overflow", [0, 1])
def test_more_keys_than_a_bucket_holds(vh, torch_cuda, overflow):
    gt = CC.table(vh, DC.KW, 1)
    if overflow:
        gt.set_option("overflow_list", 1)
    size = gt.params.bucketSize
    keys = same_bucket_keys(size + 2, gt.params.numBuckets)
    chunk = random_chunk(keys, 3)
    st = gt.stream_in(chunk)
    print(f"overflow {overflow}: {st}")
    if overflow:
        assert st["placed"] == size + 2 and st["unplaced"] == 0
    else:
        assert st["placed"] == size and st["unplaced"] == 2 and (st["status"] == S.UNPLACED).sum() == 2
    assert st["rounds"] >= st["placed"]                                            # one insertion per bucket and lock epoch
    placed = [tuple(k) for k in chunk["keys"][st["status"] == S.PLACED].tolist()]
    want = SC.chunk_model(chunk)
    snap = CC.snapshot(gt)
    S.same_models(CC.model(snap), {k: want[k] for k in placed})
    if overflow:
        assert (snap["table"]["offset"] != 0).any()                                # a chain exists ...
    back = gt.stream_out(SC.EVERYTHING)                                            # ... and the stream-out walks it
    S.same_models(SC.chunk_model(back), {k: want[k] for k in placed})
    after = CC.snapshot(gt)
    assert (after["table"]["ptr"] == -1).all() and after["counters"]["heap_counter"] == gt.params.numVoxelBlocks - 1
    assert not (after["table"]["offset"] != 0).any()
    gt.close()


# ---- 7. two half-range shards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
def test_two_shards(oracle, vh, torch_cuda, sem):
    src = SC.coloured(vh, torch_cuda, oracle, sem)
    original = CC.model(CC.snapshot(src))
    chunk = src.stream_out(SC.EVERYTHING)
    src.close()
    buckets = DC.KW["numBuckets"]
    union = {}
    for lo, hi in ((0, buckets // 2), (buckets // 2, buckets)):
        shard = CC.table(vh, DC.KW, sem, bucket_range=(lo, hi))
        st = shard.stream_in(chunk)
        mine = np.array([lo <= S.hash_block(k, buckets) < hi for k in chunk["keys"].tolist()])
        assert 8 <= mine.sum() <= len(mine) - 8
        assert np.array_equal(st["status"] == S.FOREIGN, ~mine) and np.array_equal(st["status"] == S.PLACED, mine)
        assert st["foreign"] == (~mine).sum() and st["placed"] == mine.sum()
        part = CC.model(CC.snapshot(shard))
        assert part.keys() == {tuple(k) for k in chunk["keys"][mine].tolist()}
        back = shard.stream_out(SC.middle_sphere(chunk["keys"]))                   # a shard streams out too
        assert len(back["keys"]) == S.selected(chunk["keys"][mine], SC.middle_sphere(chunk["keys"]), VS).sum()
        shard.stream_in(back)
        S.same_models(CC.model(CC.snapshot(shard)), part)
        union.update(part)
        shard.close()
    S.same_models(union, original)


# ---- 8. the host forms, and a pending pipelined frame ----------------------------------------------------------------------------
def test_host_forms_equal_device_forms(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    a, b = loaded_twins(vh, torch, oracle, 1, tmp_path)
    pre = CC.snapshot(a)
    region = SC.middle_sphere(SC.live_keys(pre["table"]), invert=True)
    chunk = a.stream_out(region)
    n = len(chunk["keys"])
    records = torch.zeros((n + 3, 4112), dtype=torch.uint8, device="cuda")
    colors = torch.zeros((n + 3, 512), dtype=torch.int32, device="cuda")
    assert b.stream_out_into(region, n + 3, records, colors) == (n, n)
    recs = records.cpu().numpy().view(vh.RECORD_DTYPE).reshape(-1)
    assert np.array_equal(recs["pos"][:n], chunk["keys"]) and not recs["reserved"].any()
    assert np.array_equal(recs["voxels"][:n].view(U), chunk["voxels"].view(U))
    assert np.array_equal(colors.cpu().numpy().view(U)[:n], chunk["colors"])
    assert not records[n:].any() and not colors[n:].any()                         # nothing beyond the written records
    same_after_removal(CC.snapshot(a), CC.snapshot(b), pre, n)
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    st_b = b.stream_in_from(records, n, colors, status)
    st_a = a.stream_in(chunk)
    assert np.array_equal(status.cpu().numpy(), st_a["status"]) and st_b == {k: v for k, v in st_a.items() if k != "status"}
    sa, sb = CC.snapshot(a), CC.snapshot(b)                                       # (which heap block a record got is the commit's race)
    S.same_models(CC.model(sa), CC.model(sb))
    S.same_models(CC.model(sa), CC.model(pre))
    assert sa["counters"] == sb["counters"] and np.array_equal(sa["table"]["pos"], sb["table"]["pos"])
    a.close()
    b.close()


@pytest.mark.parametrize("sem", [0, 1])
def test_stream_out_launches_a_pending_frame(oracle, vh, torch_cuda, sem):
    torch = torch_cuda
    frames = DC.frames(oracle)
    piped, plain = CC.table(vh, DC.KW, sem), CC.table(vh, DC.KW, sem)
    piped.set_option("pipeline", 1)
    for t in (piped, plain):
        for i in (0, 1):
            t.integrate_depth(frames[i][0], CC.dev(torch, frames[i][1]), DC.k_inv())
    plain.synchronize()
    region = SC.middle_sphere(SC.live_keys(plain.hash_table()), invert=True)
    got, want = piped.stream_out(region), plain.stream_out(region)                # (frame 1's second half is still pending in `piped`)
    assert len(want["keys"]) >= 8 and want["colors"] is None
    S.same_models(SC.chunk_model(got), SC.chunk_model(want))
    S.same_models(CC.model(CC.snapshot(piped)), CC.model(CC.snapshot(plain)))
    piped.close()
    plain.close()


# ---- 9. refusals change nothing --------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle, vh, torch_cuda):
    torch = torch_cuda
    gt, donor = SC.coloured(vh, torch, oracle), SC.coloured(vh, torch, oracle)
    pre = CC.snapshot(gt)
    lib = gt._lib
    from voxelhashing_demo_amd import _lib as L
    good = gt._stream_region(SC.EVERYTHING)
    sel, wr, st = C.c_uint64(), C.c_uint64(), L.StreamStats()
    buf = torch.zeros((4, 4112), dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert lib.vh_stream_out(None, C.byref(good), 0, None, None, C.byref(sel), C.byref(wr)) == INVALID
    assert lib.vh_stream_out(gt._h, None, 0, None, None, C.byref(sel), C.byref(wr)) == INVALID
    assert lib.vh_stream_out(gt._h, C.byref(good), 0, None, None, None, C.byref(wr)) == INVALID
    assert lib.vh_stream_out(gt._h, C.byref(good), 0, None, None, C.byref(sel), None) == INVALID
    assert lib.vh_stream_out(gt._h, C.byref(good), 4, None, None, C.byref(sel), C.byref(wr)) == INVALID
    assert lib.vh_stream_out_host(gt._h, C.byref(good), 4, None, None, C.byref(sel), C.byref(wr)) == INVALID
    assert lib.vh_stream_in(None, 4, p, None, None, C.byref(st)) == INVALID
    assert lib.vh_stream_in(gt._h, 4, None, None, None, C.byref(st)) == INVALID
    assert lib.vh_stream_in_host(gt._h, 4, None, None, None, C.byref(st)) == INVALID
    assert lib.vh_stream_in(gt._h, (1 << 24) + 1, p, None, None, C.byref(st)) == INVALID
    assert lib.vh_stream_in_host(gt._h, (1 << 24) + 1, p, None, None, C.byref(st)) == INVALID
    for bad in (dict(S.sphere((0, 0, 0), 1.0), kind=2), dict(S.sphere((0, 0, 0), 1.0), kind=-1), S.sphere((0, 0, 0), float("nan")),
                S.sphere((0, 0, 0), -0.5), S.sphere((0, 0, 0), float("inf")), S.sphere((0, float("nan"), 0), 1.0),
                S.sphere((float("inf"), 0, 0), 1.0)):
        with pytest.raises(vh.VoxelHashError):
            gt.stream_out(bad)
        with pytest.raises(vh.VoxelHashError):
            gt.stream_count(bad)
    same_state(CC.snapshot(gt), pre, compact=True)
    # a view table owns no blocks: both calls refuse it, and it stays the view it was
    n = donor.stream_count(SC.EVERYTHING)
    records = torch.zeros((n, 4112), dtype=torch.uint8, device="cuda")
    assert donor.stream_out_into(SC.EVERYTHING, n, records, None) == (n, n)
    view = CC.table(vh, DC.KW, 1, numVoxelBlocks=1)
    view.import_view(records, n)
    depth = torch.empty((DC.H, DC.W), dtype=torch.float32, device="cuda")
    view.raycast(DC.POSES[0], depth)
    seen = depth.cpu().numpy().copy()
    with pytest.raises(vh.VoxelHashError, match="view table"):
        view.stream_count(SC.EVERYTHING)
    with pytest.raises(vh.VoxelHashError, match="view table"):
        view.stream_in_from(records, n)
    view.raycast(DC.POSES[0], depth)
    assert np.array_equal(depth.cpu().numpy().view(U), seen.view(U)) and (seen != 0).sum() > 100
    for t in (gt, donor, view):
        t.close()


# ---- 10. BlockStore --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
def test_block_store_on_the_gpu(oracle, vh, torch_cuda, sem):
    gt = SC.coloured(vh, torch_cuda, oracle, sem)
    pre = CC.snapshot(gt)
    original = CC.model(pre)
    live = SC.live_keys(pre["table"])
    store = streaming.BlockStore(VS)
    far = (500.0, -300.0, 100.0)
    moved = store.update(gt, far, 1.0, 2.0)                                       # the camera is elsewhere: everything leaves
    assert moved["out"] == len(original) == len(store) and moved["in"] == 0
    assert (gt.hash_table()["ptr"] == -1).all() and gt.counters()["heap_counter"] == gt.params.numVoxelBlocks - 1
    here = SC.middle_sphere(live)
    c, r = here["centre"], here["radius"]
    moved = store.update(gt, c, 100.0, 100.0)                                     # ... and back: the model returns, bit for bit
    assert moved["in"] == len(original) and moved["out"] == 0 and len(store) == 0
    S.same_models(CC.model(CC.snapshot(gt)), original)
    # hysteresis: r_in < r_out around the middle of the model
    moved = store.update(gt, c, 0.5 * r, r)
    outside = S.selected(live, S.sphere(c, r, invert=True), VS)
    assert moved["out"] == outside.sum() >= 8 and moved["in"] == 0 and len(store) == moved["out"]
    moved = store.update(gt, c, 0.5 * r, 4.0 * r)                                 # a wider r_out alone brings nothing back
    assert moved == {"out": 0, "in": 0, "present": 0, "unplaced": 0, "foreign": 0, "stored": int(outside.sum())}
    ring = S.selected(live, S.sphere(c, 1.5 * r), VS) & outside
    assert 0 < ring.sum() < outside.sum()
    moved = store.update(gt, c, 1.5 * r, 4.0 * r)                                 # r_in grown: the ring between r and 1.5 r returns
    assert moved["in"] == ring.sum() and moved["out"] == 0 and len(store) == outside.sum() - ring.sum()
    kept = CC.model(CC.snapshot(gt))
    assert kept.keys() == {tuple(k) for k in live[~outside | ring].tolist()}
    st = store.restore_all(gt)
    assert st["placed"] == outside.sum() - ring.sum() and st["stored"] == 0
    S.same_models(CC.model(CC.snapshot(gt)), original)
    gt.close()


# ---- 11. more than one tile of slice counts --------------------------------------------------------------------------------------
def selection_spans_the_table(table, order, last_bucket):
    """The conditions that make a selection of many_slices' table mean something: selected entries in both tiles of the slice
    scan, unselected allocated entries in both, and (last_bucket) both entries of the last bucket selected."""
    live = np.nonzero(table["ptr"] != -1)[0]
    assert mm.in_both_slice_tiles(order) and mm.in_both_slice_tiles(np.setdiff1d(live, order))
    assert not last_bucket or (order // 2 == mm.SLICE_BUCKETS - 1).sum() == 2


def records_of(chunk, table, vox, order, selected):
    """`chunk` holds the blocks of entries `order` of the downloaded table, in that order, bit for bit."""
    assert chunk["selected"] == selected and len(chunk["keys"]) == len(order) and chunk["colors"] is None
    assert np.array_equal(chunk["keys"], table["pos"][order])
    at = (table["ptr"][order].astype(np.int64)[:, None] + np.arange(512)[None, :]).reshape(-1)
    assert np.array_equal(np.ascontiguousarray(chunk["voxels"]).view(U).reshape(-1), vox[at].view(U).reshape(-1))


@pytest.mark.parametrize("kind", ["outside_sphere", "box"])
def test_more_than_one_tile_of_slices(vh, torch_cuda, tmp_path, kind):
    """The list walk of vh_stream_out over 2 048 slices, two tiles of the slice scan: the count-only call, a call with a
    capacity below the selection and the full call, against the rule on the downloaded table."""
    gt = mm.many_slices_table(vh, tmp_path)
    vs = gt.params.voxelSize
    lo = np.array(mm.SLICE_BALL_LO)
    cube = set(mm.cube_keys(lo, lo + 12))
    # the ball's block centres lie within 77.6 voxels of its centre; the box cuts it on x and z
    region = {"outside_sphere": S.sphere((lo * 8 + 48.3) * vs, 80 * vs, invert=True),
              "box": S.box(lo + (4, 0, 2), lo + (9, 12, 40))}[kind]
    table, vox = gt.hash_table(), gt.sdf_blocks()
    model = mm.model_of(table, vox)
    order = S.selection_of_table(table, region, vs)
    chosen = set(map(tuple, table["pos"][order].tolist()))
    print(f"{kind}: {len(order)} of {len(model)} blocks selected, {len(chosen & cube)} of the ball's {len(cube)}")
    selection_spans_the_table(table, order, last_bucket=kind == "outside_sphere")
    if kind == "outside_sphere":
        assert not chosen & cube                                                    # the radius covers the ball
    else:
        assert 0 < len(chosen & cube) < len(cube)                                   # the box cuts it

    assert gt.stream_count(region) == len(order)                                   # the count-only call: nothing changes
    assert np.array_equal(gt.hash_table(), table) and np.array_equal(gt.sdf_blocks().view(U), vox.view(U))

    cap = len(order) // 3                                                           # a capacity below the selection
    first = gt.stream_out(region, capacity=cap)
    records_of(first, table, vox, order[:cap], len(order))
    mid_table, mid_vox = gt.hash_table(), gt.sdf_blocks()
    taken = set(map(tuple, first["keys"].tolist()))
    S.same_models(mm.model_of(mid_table, mid_vox), {k: v for k, v in model.items() if k not in taken})

    rest = S.selection_of_table(mid_table, region, vs)                              # the full call: what is left of the selection
    assert len(rest) == len(order) - cap
    selection_spans_the_table(mid_table, rest, last_bucket=kind == "outside_sphere")
    second = gt.stream_out(region)
    records_of(second, mid_table, mid_vox, rest, len(rest))
    S.same_models(mm.model_of(gt.hash_table(), gt.sdf_blocks()), {k: v for k, v in model.items() if k not in chosen})
    assert gt.stream_count(region) == 0
    gt.close()
