"""vh_merge on the GPU against tests/merge_ref.py applied to the downloaded pre-state of dst and the downloaded src model: every
voxel bit per key (block ids and slots are free, as same_model of tests/test_gpu_deintegrate.py has it), the key set, the heap
counter, the compact set, `occupied` and the stats.  64x48 frames of the synthetic room (tests/merge_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import deintegrate_cases as DC
import merge_cases as MC
import merge_ref as R
import mesh_indexed_ref as IR
import mesh_models as MM
import sample_ref as S

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
W, H = MC.W, MC.H
NEAREST, TRILINEAR = 0, 1


def table(vh, kw, sem=1, bucket_range=None, **over):
    p = dict(kw)
    p.update(over)
    gt = vh.SDFHashtable(vh.default_params(**p), W, H, sem, bucket_range=bucket_range)
    gt.set_projection(DC.projection(sem, W, H))
    return gt


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(torch, gt, oracle, which):
    frames = DC.frames(oracle)
    for i in which:
        pose, d16, _ = frames[i]
        gt.integrate_depth(pose, dev(torch, d16), DC.k_inv())


def snapshot(gt):
    gt.synchronize()
    c = gt.counters()
    return dict(table=gt.hash_table(), heap=gt.heap(), vox=gt.sdf_blocks(), compact=gt.compact(), counters=c)


def unchanged(a, b):
    assert np.array_equal(a["table"], b["table"]) and np.array_equal(a["heap"], b["heap"])
    assert np.array_equal(a["vox"].view(U), b["vox"].view(U))
    assert a["counters"] == b["counters"]


def model(snap):
    return MM.model_of(snap["table"], snap["vox"])


def solid(m):
    """The blocks that hold anything: a block of zeros is the same model with or without it."""
    return {k: v for k, v in m.items() if v[0].view(U).any() or v[1].view(U).any()}


def same_blocks(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k][0].view(U), b[k][0].view(U)) and np.array_equal(a[k][1].view(U), b[k][1].view(U)), k


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


def owned(keys, gt):
    """The keys whose bucket lies in the context's range."""
    keys = sorted(keys)
    if not keys:
        return set()
    h = MM.hash_block(np.array(keys, np.int64), gt.params.numBuckets)
    lo, hi = gt.bucket_range
    return {k for k, b in zip(keys, np.asarray(h).tolist()) if lo <= b < hi}


_SRC = {}


def source(vh, torch, oracle, sem=1, **over):
    """A src context fused from SRC_FRAMES and its snapshot; one per configuration for the whole module (src is only read)."""
    key = (sem, tuple(sorted(over.items())))
    if key not in _SRC:
        options = {k: over.pop(k) for k in list(over) if k == "overflow_list"}
        gt = table(vh, MC.SRC_KW, sem, **over)
        for name, value in options.items():
            gt.set_option(name, value)
        # (a frame inserts one key per bucket: with the overflow list the frames go in three times over, so that chains can form)
        fuse(torch, gt, oracle, MC.SRC_FRAMES * (3 if options else 1))
        snap = snapshot(gt)
        assert snap["counters"]["heap_exhausted"] == 0 and 50 < len(model(snap)) < 512
        _SRC[key] = (gt, snap)
    return _SRC[key]


def merge_and_check(oracle, dst, src, src_snap, T, mode, expect_placed=True):
    """One vh_merge, compared with the rule.  Returns (stats, the rule's stats, post snapshot, candidate keys that are dst's)."""
    pre = snapshot(dst)
    stats = dst.merge(src, T, mode)
    post = snapshot(dst)
    unchanged(src_snap, snapshot(src))                                           # src is only read
    src_model, pre_model, post_model = model(src_snap), model(pre), model(post)
    vs_s, vs_d = F(src.params.voxelSize), F(dst.params.voxelSize)
    mult = R.multiplicity(src_model.keys(), T, vs_s, vs_d)
    cand, records = R.candidates(src_model.keys(), T, vs_s, vs_d)
    assert set(mult) == cand and sum(mult.values()) == records
    mine = owned(cand, dst)
    assert set(pre_model) <= set(post_model) <= set(pre_model) | mine
    present = mine & set(post_model)
    want, rule = R.apply(MC.with_new_blocks(pre_model, post_model.keys()), src_model, sorted(present), oracle.invert4x4(T), vs_s, vs_d,
                         dst.params.truncation, dst.params.integrationWeightMax, mode)
    print(f"merge: {stats}; rule: {rule}; src blocks {len(src_model)}, candidates {len(cand)} ({len(mine)} owned), pre {len(pre_model)}")
    assert post_model.keys() == want.keys()
    for k in want:
        assert np.array_equal(post_model[k][0].view(U), want[k][0].view(U)), k
        assert np.array_equal(post_model[k][1].view(U), want[k][1].view(U)), k
    # the stats are the rule's counts
    assert stats["source_blocks"] == len(src_model) and stats["skipped_blocks"] == R.skipped(src_model.keys(), T, vs_s, vs_d)
    assert stats["candidates"] == records
    assert stats["allocated"] == len(post_model) - len(pre_model)
    assert stats["allocated"] == pre["counters"]["heap_counter"] - post["counters"]["heap_counter"]
    assert stats["allocated"] == post["counters"]["allocated_total"] - pre["counters"]["allocated_total"]
    assert stats["blocks"] == len(present) == post["counters"]["occupied"]
    assert keys_of(post["compact"]) == sorted(present)                           # the compact list: the blocks the update ran over
    assert stats["unplaced"] == sum(mult[k] for k in mine - set(post_model))
    assert stats["rounds"] >= 1 and post["counters"]["epoch"] == pre["counters"]["epoch"] + stats["rounds"]
    if expect_placed:
        assert stats["unplaced"] == 0 and set(post_model) == set(pre_model) | mine
        assert post["counters"]["heap_exhausted"] == pre["counters"]["heap_exhausted"]
    return stats, rule, post, mine


def collect_and_check(dst, rule, post):
    """vh_garbage_collect directly afterwards frees exactly the updated blocks the rule leaves without any weight."""
    dst.garbage_collect(float("inf"))
    c = dst.counters()
    assert c["last_freed"] == rule["empty_blocks"]
    assert c["heap_counter"] == post["counters"]["heap_counter"] + rule["empty_blocks"]
    return c


# ---- 1. the identity copy ------------------------------------------------------------------------------------------------
def test_identity_nearest_into_an_empty_model_is_a_copy(oracle, vh, torch_cuda):
    src, src_snap = source(vh, torch_cuda, oracle)
    dst = table(vh, MC.DST_KW)
    stats, rule, post, mine = merge_and_check(oracle, dst, src, src_snap, MC.IDENTITY, NEAREST)
    src_model, got = model(src_snap), model(post)
    assert set(src_model) <= set(got) and rule["combined"] == 0 and rule["fresh"] > 10000
    copied = 0
    for k, (s, w) in src_model.items():
        valid = (w > 0) & (s == s)
        assert np.array_equal(got[k][0][valid].view(U), s[valid].view(U)) and np.array_equal(got[k][1][valid].view(U), w[valid].view(U))
        assert not got[k][0][~valid].view(U).any() and not got[k][1][~valid].view(U).any()
        copied += int(valid.sum())
    assert copied == rule["fresh"]
    collect_and_check(dst, rule, post)
    dst.close()


# ---- 2. oblique, trilinear, into a model that is already there -------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
def test_oblique_trilinear_into_a_fused_model(oracle, vh, torch_cuda, sem):
    src, src_snap = source(vh, torch_cuda, oracle, sem)
    dst = table(vh, MC.DST_KW, sem)
    fuse(torch_cuda, dst, oracle, MC.DST_FRAMES)
    stats, rule, post, _ = merge_and_check(oracle, dst, src, src_snap, MC.OBLIQUE, TRILINEAR)
    assert stats["allocated"] > 0 and stats["blocks"] > stats["allocated"]        # blocks newly allocated and blocks combined
    assert rule["fresh"] > 0 and rule["combined"] > 0 and rule["empty_blocks"] > 0
    collect_and_check(dst, rule, post)
    dst.close()


# ---- 3. other voxel sizes, the nearest sample under a rotation, the half-voxel shift -----------------------------------------
@pytest.mark.parametrize("name,ratio,mode", MC.REGRID, ids=[f"{n}-x{r}-{'trilinear' if m else 'nearest'}" for n, r, m in MC.REGRID])
def test_regrid_and_modes(oracle, vh, torch_cuda, name, ratio, mode):
    src, src_snap = source(vh, torch_cuda, oracle)
    # (half the voxel size: eight dst blocks per src block before the dilation -- a pool of 2^15 there, 4096 elsewhere)
    dst = table(vh, MC.DST_KW, voxelSize=float(F(MC.VS * ratio)), **({"numVoxelBlocks": 1 << 15, "numBuckets": 1 << 13} if ratio < 1 else {}))
    stats, rule, post, _ = merge_and_check(oracle, dst, src, src_snap, MC.TRANSFORMS[name], mode)
    assert rule["fresh"] > 1000
    dst.close()


# ---- 4. the overflow list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_overflow", [False, True])
def test_overflow_list_chains_and_rounds(oracle, vh, torch_cuda, src_overflow):
    src, src_snap = (source(vh, torch_cuda, oracle, 1, overflow_list=1, numBuckets=64, bucketSize=2) if src_overflow
                     else source(vh, torch_cuda, oracle))
    if src_overflow:
        assert (src_snap["table"]["offset"] != 0).any()                          # src holds chained entries: they are walked too
    dst = table(vh, MC.DST_KW, numBuckets=64, bucketSize=2)
    dst.set_option("overflow_list", 1)
    # 128 slots for some hundreds of candidates: chains form, the table fills, and what is present follows the rule
    stats, rule, post, mine = merge_and_check(oracle, dst, src, src_snap, MC.IDENTITY, TRILINEAR, expect_placed=False)
    assert stats["rounds"] > 1 and (post["table"]["offset"] != 0).any()
    assert stats["blocks"] > 64 and rule["fresh"] > 0
    dst.close()
    # and with room for all of them (256 slots; some buckets are the home of three keys): chains, several rounds, all placed
    dst = table(vh, MC.DST_KW, numBuckets=128, bucketSize=2)
    dst.set_option("overflow_list", 1)
    homes = np.bincount(np.asarray(MM.hash_block(np.array(sorted(model(src_snap)), np.int64), 128)), minlength=128)
    assert homes.max() > 2
    stats, rule, post, mine = merge_and_check(oracle, dst, src, src_snap, MC.IDENTITY, TRILINEAR)
    assert stats["rounds"] > 1 and (post["table"]["offset"] != 0).any()
    dst.close()


# ---- 5. a heap too small for the candidates ------------------------------------------------------------------------------------
def test_heap_too_small(oracle, vh, torch_cuda):
    src, src_snap = source(vh, torch_cuda, oracle)
    dst = table(vh, MC.DST_KW, numVoxelBlocks=96)
    stats, rule, post, mine = merge_and_check(oracle, dst, src, src_snap, MC.OBLIQUE, TRILINEAR, expect_placed=False)
    assert stats["unplaced"] > 0 and stats["allocated"] == 96 and post["counters"]["heap_exhausted"] > 0
    assert post["counters"]["heap_counter"] == -1
    assert rule["empty_blocks"] > 0
    collect_and_check(dst, rule, post)
    # the collection has made room: a second merge places more blocks (and follows the rule from the state it finds)
    again, _, _, _ = merge_and_check(oracle, dst, src, src_snap, MC.OBLIQUE, TRILINEAR, expect_placed=False)
    assert again["allocated"] > 0
    dst.close()


# ---- 6. shards -------------------------------------------------------------------------------------------------------------------
def test_dst_as_two_shards_and_src_as_a_shard(oracle, vh, torch_cuda):
    src, src_snap = source(vh, torch_cuda, oracle)
    whole = table(vh, MC.DST_KW)
    fuse(torch_cuda, whole, oracle, MC.DST_FRAMES)
    pre_whole = model(snapshot(whole))
    _, _, post_whole, _ = merge_and_check(oracle, whole, src, src_snap, MC.OBLIQUE, TRILINEAR)
    want = model(post_whole)
    n = MC.DST_KW["numBuckets"]
    union = {}
    for rng in ((0, n // 2), (n // 2, n)):
        shard = table(vh, MC.DST_KW, bucket_range=rng)
        # the shard starts from its part of the whole's pre-state: a nearest identity merge into an empty shard is a copy
        seed = table(vh, MC.DST_KW)
        fuse(torch_cuda, seed, oracle, MC.DST_FRAMES)
        merge_and_check(oracle, shard, seed, snapshot(seed), MC.IDENTITY, NEAREST)
        shard.garbage_collect(float("inf"))                                       # (the candidates that stayed empty)
        seed.close()
        mine_before = owned(pre_whole.keys(), shard)
        same_blocks(solid(model(snapshot(shard))), {k: v for k, v in solid(pre_whole).items() if k in mine_before})
        _, _, post, mine = merge_and_check(oracle, shard, src, src_snap, MC.OBLIQUE, TRILINEAR)
        assert 0 < len(mine) and not set(model(post)) & set(union)
        union.update(model(post))
        shard.close()
    same_blocks(solid(union), solid(want))                                         # the union per key is the unsharded merge
    whole.close()
    # src as a shard: the blocks of the other half are simply absent
    half = table(vh, MC.SRC_KW, bucket_range=(0, MC.SRC_KW["numBuckets"] // 2))
    merge_and_check(oracle, half, src, src_snap, MC.IDENTITY, NEAREST)
    half_snap = snapshot(half)
    assert 0 < len(model(half_snap)) < len(model(src_snap))
    dst = table(vh, MC.DST_KW)
    stats, rule, _, _ = merge_and_check(oracle, dst, half, half_snap, MC.OBLIQUE, TRILINEAR)
    assert stats["source_blocks"] == len(model(half_snap)) and rule["fresh"] > 0
    dst.close()
    half.close()


# ---- 7. ordering -------------------------------------------------------------------------------------------------------------------
def test_pending_frames_and_a_stream_of_its_own(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    results = []
    for eager in (False, True):
        src, dst = table(vh, MC.SRC_KW), table(vh, MC.DST_KW)
        stream = None
        if not eager:
            stream = torch.cuda.Stream()
            src.set_stream(stream)
            src.set_option("pipeline", 1)
            dst.set_option("pipeline", 1)
        images = [dev(torch, frames[i][1]) for i in range(3)]
        torch.cuda.synchronize()
        for i in MC.SRC_FRAMES:
            src.integrate_depth(frames[i][0], images[i], DC.k_inv())              # (pipelined: the last frame stays pending)
        for i in MC.DST_FRAMES:
            dst.integrate_depth(frames[i][0], images[i], DC.k_inv())
        if eager:
            src.synchronize()
            dst.synchronize()
        stats = dst.merge(src, MC.OBLIQUE, TRILINEAR)                             # no synchronisation of ours in between
        results.append((stats, snapshot(dst), snapshot(src)))
        src.close()
        dst.close()
    (sa, a, srca), (sb, b, srcb) = results
    assert sa == sb and sa["allocated"] > 0
    same_blocks(model(a), model(b))
    same_blocks(model(srca), model(srcb))
    assert keys_of(a["compact"]) == keys_of(b["compact"]) and a["counters"]["heap_counter"] == b["counters"]["heap_counter"]


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle, vh, torch_cuda):
    torch = torch_cuda
    src, src_snap = source(vh, torch, oracle)
    dst = table(vh, MC.DST_KW)
    fuse(torch, dst, oracle, MC.DST_FRAMES)
    pre = snapshot(dst)
    lib = vh.load()
    fp = C.POINTER(C.c_float)

    def call(d, s, T, mode):
        m = None if T is None else np.ascontiguousarray(np.asarray(T, F).reshape(16)).ctypes.data_as(fp)
        return lib.vh_merge(d, s, m, mode, None)

    nan = MC.OBLIQUE.copy()
    nan[1, 2] = np.nan
    inf = MC.OBLIQUE.copy()
    inf[0, 3] = np.inf
    singular = np.zeros((4, 4), F)                                                # finite, its inverse is not
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), W, H, 1)
    ball = MC.shell()
    rec = torch.from_numpy(MM.view_records(ball)).cuda()
    view.import_view(rec, len(ball))
    view_pre = snapshot(view)
    INVALID = 1
    assert call(None, src._h, MC.IDENTITY, 1) == INVALID and call(dst._h, None, MC.IDENTITY, 1) == INVALID
    assert call(dst._h, src._h, None, 1) == INVALID
    assert call(dst._h, dst._h, MC.IDENTITY, 1) == INVALID                         # src == dst
    assert call(view._h, src._h, MC.IDENTITY, 1) == INVALID                        # dst holds an imported view
    for mode in (-1, 2, 7):
        assert call(dst._h, src._h, MC.IDENTITY, mode) == INVALID
    for T in (nan, inf, singular):
        assert call(dst._h, src._h, T, 1) == INVALID
    with pytest.raises(vh.VoxelHashError, match="invalid argument"):
        dst.merge(src, nan)
    unchanged(pre, snapshot(dst))
    unchanged(view_pre, snapshot(view))
    unchanged(src_snap, snapshot(src))
    # an empty src: VH_OK, zeros, nothing changed
    empty = table(vh, MC.SRC_KW)
    stats = dst.merge(empty, MC.OBLIQUE, TRILINEAR)
    assert stats == dict(source_blocks=0, skipped_blocks=0, candidates=0, allocated=0, blocks=0, unplaced=0, rounds=0)
    unchanged(pre, snapshot(dst))
    # a view table as SRC is a model like any other
    fresh = table(vh, MC.DST_KW, voxelSize=0.02)
    stats = fresh.merge(view, MC.IDENTITY, NEAREST)
    got = model(snapshot(fresh))
    assert stats["source_blocks"] == len(ball) and set(ball) <= set(got)
    for k, (s, w) in ball.items():
        valid = w > 0
        assert np.array_equal(got[k][0][valid].view(U), np.clip(s[valid], -1, 1).view(U))       # (clamped to dst's truncation, 1.0)
    for t in (empty, fresh, view, dst):
        t.close()


# ---- 9. the merged model is an ordinary model ----------------------------------------------------------------------------------------
def test_merged_model_meshes_and_samples(oracle, vh, torch_cuda):
    torch = torch_cuda
    src, src_snap = source(vh, torch, oracle)
    dst = table(vh, MC.DST_KW)
    fuse(torch, dst, oracle, MC.DST_FRAMES)
    dst.merge(src, MC.OBLIQUE, TRILINEAR)
    v, f, n = dst.extract_mesh_indexed(normals=True)
    snap = snapshot(dst)
    wv, wf, wn, _ = IR.extract_indexed(snap["table"], snap["vox"], dst.params.voxelSize, None, normals=True)
    assert len(wv) > 100 and len(wf) > 100 and np.array_equal(f.astype(np.int64), wf)
    assert S.same_bits(v, wv) and S.same_bits(n, wn)
    m = model(snap)
    keys = np.array(sorted(m), np.int64)
    rng = np.random.RandomState(41)
    pts = ((keys[rng.randint(0, len(keys), 4096)] * 8 + rng.uniform(-1, 9, (4096, 3))) * dst.params.voxelSize).astype(F)
    field = S.Field(m)
    for mode in (NEAREST, TRILINEAR):
        sdf, w, g = (t.cpu().numpy() for t in dst.sample_sdf(dev(torch, pts), mode, weight=True, gradient=True))
        ws, ww, wg = S.sample(field, pts, dst.params.voxelSize, mode)
        assert (ws == ws).sum() > 500
        assert S.same_bits(sdf, ws) and S.same_bits(w, ww) and S.same_bits(g, wg)
    dst.close()


def test_close_shared_sources():
    for gt, _ in _SRC.values():
        gt.close()
    _SRC.clear()
