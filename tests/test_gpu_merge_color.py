"""vh_merge_color on the GPU, compared per block key: the voxels bit for bit with a twin dst that received plain vh_merge, the colour
words with tests/merge_color_ref.py applied to the downloaded pre-state of dst and the downloaded src model, and both of src's
volumes unchanged.  64x48 frames of the synthetic room with a colour image per frame (tests/merge_color_cases.py); that every
colour branch is populated for these inputs is checked without a GPU in tests/test_merge_color_ref_cpu.py and again here."""
import ctypes as C

import numpy as np
import pytest

import color_ref as CR
import deintegrate_cases as DC
import merge_cases as MC
import merge_color_cases as CC
import merge_color_ref as M
import merge_ref as R
import mesh_models as MM

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
W, H = MC.W, MC.H
NEAREST, TRILINEAR = 0, 1
INVALID = 1


def owned(keys, gt):
    keys = sorted(keys)
    if not keys:
        return set()
    h = MM.hash_block(np.array(keys, np.int64), gt.params.numBuckets)
    lo, hi = gt.bucket_range
    return {k for k, b in zip(keys, np.asarray(h).tolist()) if lo <= b < hi}


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


_SRC = {}


def source(vh, torch, oracle, sem=1, colors=True, **over):
    """A src context fused and coloured by CC.SRC_COLORS, and its snapshot; one per configuration for the module (only read)."""
    key = (sem, colors, tuple(sorted(over.items())))
    if key not in _SRC:
        options = {k: over.pop(k) for k in list(over) if k == "overflow_list"}
        gt = CC.table(vh, MC.SRC_KW, sem, **over)
        for name, value in options.items():
            gt.set_option(name, value)
        frames = DC.frames(oracle)
        for _ in range(3 if options else 1):                                     # (three times over, so that chains can form)
            for i in sorted(CC.SRC_COLORS):
                gt.integrate_depth(frames[i][0], CC.dev(torch, frames[i][1]), DC.k_inv())
        if colors:
            CC.fuse(torch, gt, oracle, CC.SRC_COLORS, depth=False)
        snap = CC.snapshot(gt)
        assert snap["counters"]["heap_exhausted"] == 0 and 50 < len(CC.model(snap)) < 512 and snap["has_color"] == colors
        _SRC[key] = (gt, snap)
    return _SRC[key]


def fused_dst(vh, torch, oracle, sem=1, colors=True, **over):
    options = {k: over.pop(k) for k in list(over) if k == "overflow_list"}
    gt = CC.table(vh, MC.DST_KW, sem, **over)
    for name, value in options.items():
        gt.set_option(name, value)
    if colors:
        CC.fuse(torch, gt, oracle, CC.DST_COLORS)
    else:
        frames = DC.frames(oracle)
        for i in sorted(CC.DST_COLORS):
            gt.integrate_depth(frames[i][0], CC.dev(torch, frames[i][1]), DC.k_inv())
    return gt


def merge_and_check(oracle, dst, twin, src, src_snap, T, mode, weight_max=255):
    """One vh_merge_color into dst and one vh_merge into its twin (built the same way).  Returns (stats, the rule's colour
    counts, post snapshot)."""
    pre = CC.snapshot(dst)
    stats = dst.merge(src, T, mode, colors=True, color_weight_max=weight_max)
    post = CC.snapshot(dst)
    CC.unchanged(src_snap, CC.snapshot(src))                                     # src's two volumes are only read
    twin_stats = twin.merge(src, T, mode)
    tpost = CC.snapshot(twin)
    got, plain = CC.model(post), CC.model(tpost)
    assert stats == twin_stats and stats["unplaced"] == 0
    assert got.keys() == plain.keys() and keys_of(post["compact"]) == keys_of(tpost["compact"])
    assert post["counters"]["occupied"] == tpost["counters"]["occupied"] == stats["blocks"]
    for k in got:                                                                # the voxels: vh_merge's bits
        assert np.array_equal(got[k][0].view(U), plain[k][0].view(U)) and np.array_equal(got[k][1].view(U), plain[k][1].view(U)), k
    src_model, pre_model = CC.model(src_snap), CC.model(pre)
    vs_s, vs_d = F(src.params.voxelSize), F(dst.params.voxelSize)
    cand, _ = R.candidates(src_model.keys(), T, vs_s, vs_d)
    present = owned(cand, dst) & set(got)
    assert keys_of(post["compact"]) == sorted(present)
    # (the voxels are the twin's, and vh_merge is held to merge_ref.apply by tests/test_gpu_merge.py: the rule's geometry pass,
    # a second sampling of every voxel, is not repeated here)
    want, _, cstats = M.apply(CC.with_new_blocks(pre_model, got.keys()), src_model, sorted(present), oracle.invert4x4(T), vs_s,
                              vs_d, dst.params.truncation, dst.params.integrationWeightMax, mode, weight_max,
                              merged={k: (v[0], v[1]) for k, v in plain.items()})
    print(f"merge_color: {stats}; colour {cstats}")
    assert want.keys() == got.keys()
    for k in want:
        bad = np.nonzero(got[k][2] != want[k][2])[0]
        assert len(bad) == 0, (k, len(bad), bad[:4], got[k][2][bad[:4]], want[k][2][bad[:4]])
    # no word outside the blocks the table holds
    inside = np.zeros(len(post["color"]), bool)
    tab = post["table"]
    inside[(tab["ptr"][tab["ptr"] != -1].astype(np.int64)[:, None] + np.arange(512)).ravel()] = True
    assert not post["color"][~inside].any()
    return stats, cstats, post


# ---- 1. the identity copy, and the volume that appears ----------------------------------------------------------------------------
def test_identity_nearest_into_an_empty_model_copies_both_volumes(oracle, vh, torch_cuda):
    src, src_snap = source(vh, torch_cuda, oracle)
    dst, twin = CC.table(vh, MC.DST_KW), CC.table(vh, MC.DST_KW)
    assert not dst.has_color()
    stats, cstats, post = merge_and_check(oracle, dst, twin, src, src_snap, MC.IDENTITY, NEAREST, 255)
    assert dst.has_color() and not twin.has_color()                               # dst without colour, src with: the volume appears
    src_model, got = CC.model(src_snap), CC.model(post)
    copied = 0
    for k, (s, w, c) in src_model.items():
        valid = (w > 0) & (s == s)
        assert np.array_equal(got[k][0][valid].view(U), s[valid].view(U)) and np.array_equal(got[k][1][valid].view(U), w[valid].view(U))
        assert np.array_equal(got[k][2][valid], c[valid]) and not got[k][2][~valid].any()
        copied += int((valid & (c != 0)).sum())
    assert copied == cstats["fresh"] > 1000 and cstats["combined"] == 0
    dst.close()
    twin.close()


# ---- 2. into a fused, coloured dst: every branch, both semantics, the cap -----------------------------------------------------------
@pytest.mark.parametrize("sem,name,transform,ratio,mode,weight_max", CC.SEM_CASES, ids=[f"sem{c[0]}-{c[1]}" for c in CC.SEM_CASES])
def test_into_a_fused_coloured_model(oracle, vh, torch_cuda, sem, name, transform, ratio, mode, weight_max):
    src, src_snap = source(vh, torch_cuda, oracle, sem)
    dst, twin = fused_dst(vh, torch_cuda, oracle, sem), fused_dst(vh, torch_cuda, oracle, sem)
    stats, cstats, post = merge_and_check(oracle, dst, twin, src, src_snap, CC.TRANSFORMS[transform], mode, weight_max)
    assert stats["allocated"] > 0 and stats["blocks"] > stats["allocated"]
    need = ["fresh", "combined", "no_sample", "kept"] + (["capped"] if weight_max < 5 else [])
    assert all(cstats[n] > 0 for n in need), cstats
    top = int(CR.count(post["color"]).max())
    assert top == 3 if weight_max == 3 else top <= 5                              # (src's counts reach 4, dst's are 1)
    dst.close()
    twin.close()


# ---- 3. other voxel sizes, the nearest sample under a rotation, the half-voxel shift --------------------------------------------------
@pytest.mark.parametrize("name,ratio,mode", MC.REGRID, ids=[f"{n}-x{r}-{'trilinear' if m else 'nearest'}" for n, r, m in MC.REGRID])
def test_regrid_and_modes(oracle, vh, torch_cuda, name, ratio, mode):
    src, src_snap = source(vh, torch_cuda, oracle)
    over = dict(voxelSize=float(F(MC.VS * ratio)), **({"numVoxelBlocks": 1 << 15, "numBuckets": 1 << 13} if ratio < 1 else {}))
    dst, twin = CC.table(vh, MC.DST_KW, **over), CC.table(vh, MC.DST_KW, **over)
    stats, cstats, post = merge_and_check(oracle, dst, twin, src, src_snap, MC.TRANSFORMS[name], mode, 255)
    assert cstats["fresh"] > 500 and cstats["no_sample"] > 0
    dst.close()
    twin.close()


# ---- 4. a src without colour ---------------------------------------------------------------------------------------------------------
def test_src_without_colour_is_plain_merge(oracle, vh, torch_cuda):
    torch = torch_cuda
    src, src_snap = source(vh, torch, oracle, colors=False)
    dst, twin = fused_dst(vh, torch, oracle, colors=False), fused_dst(vh, torch, oracle, colors=False)
    a = dst.merge(src, CC.CLOSE, TRILINEAR, colors=True, color_weight_max=7)
    b = twin.merge(src, CC.CLOSE, TRILINEAR)
    assert a == b and not dst.has_color() and not src.has_color()                 # nothing allocated in dst
    got, plain = CC.model(CC.snapshot(dst)), CC.model(CC.snapshot(twin))
    assert got.keys() == plain.keys()
    for k in got:
        assert np.array_equal(got[k][0].view(U), plain[k][0].view(U)) and np.array_equal(got[k][1].view(U), plain[k][1].view(U))
    dst.close()
    twin.close()
    # a coloured dst keeps its words; a view table as src carries none
    dst = fused_dst(vh, torch, oracle)
    before = {k: v[2] for k, v in CC.model(CC.snapshot(dst)).items()}
    dst.merge(src, CC.CLOSE, TRILINEAR, colors=True)
    after = CC.model(CC.snapshot(dst))
    assert all(np.array_equal(after[k][2], c) for k, c in before.items())
    assert not any(v[2].any() for k, v in after.items() if k not in before)
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), W, H, 1)
    ball = MC.shell()
    view.import_view(torch.from_numpy(MM.view_records(ball)).cuda(), len(ball))
    fresh = CC.table(vh, MC.DST_KW, voxelSize=0.02)
    st = fresh.merge(view, MC.IDENTITY, NEAREST, colors=True)
    assert st["source_blocks"] == len(ball) and not fresh.has_color()
    for t in (dst, view, fresh):
        t.close()


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------
def test_dst_as_two_shards_and_src_as_a_shard(oracle, vh, torch_cuda):
    torch = torch_cuda
    src, src_snap = source(vh, torch, oracle)
    whole, twin = CC.table(vh, MC.DST_KW), CC.table(vh, MC.DST_KW)
    _, _, post_whole = merge_and_check(oracle, whole, twin, src, src_snap, MC.OBLIQUE, TRILINEAR, 3)
    want = CC.model(post_whole)
    n = MC.DST_KW["numBuckets"]
    union = {}
    for rng in ((0, n // 2), (n // 2, n)):
        shard, stwin = CC.table(vh, MC.DST_KW, bucket_range=rng), CC.table(vh, MC.DST_KW, bucket_range=rng)
        _, cstats, post = merge_and_check(oracle, shard, stwin, src, src_snap, MC.OBLIQUE, TRILINEAR, 3)
        part = CC.model(post)
        assert cstats["fresh"] > 0 and not set(part) & set(union)
        union.update(part)
        shard.close()
        stwin.close()
    assert union.keys() == want.keys()
    for k in want:
        assert all(np.array_equal(np.asarray(a).view(U), np.asarray(b).view(U)) for a, b in zip(union[k], want[k])), k
    whole.close()
    twin.close()
    # src as a shard: the blocks of the other half are simply absent, for colour as for the TSDF
    rng = (0, MC.SRC_KW["numBuckets"] // 2)
    half, htwin = CC.table(vh, MC.SRC_KW, bucket_range=rng), CC.table(vh, MC.SRC_KW, bucket_range=rng)
    merge_and_check(oracle, half, htwin, src, src_snap, MC.IDENTITY, NEAREST, 255)
    half_snap = CC.snapshot(half)
    assert 0 < len(CC.model(half_snap)) < len(CC.model(src_snap))
    dst, twin = CC.table(vh, MC.DST_KW), CC.table(vh, MC.DST_KW)
    stats, cstats, _ = merge_and_check(oracle, dst, twin, half, half_snap, CC.CLOSE, TRILINEAR, 255)
    assert stats["source_blocks"] == len(CC.model(half_snap)) and cstats["fresh"] > 0
    for t in (half, htwin, dst, twin):
        t.close()


# ---- 6. the overflow list on either side ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_overflow", [False, True])
def test_overflow_list(oracle, vh, torch_cuda, src_overflow):
    src, src_snap = (source(vh, torch_cuda, oracle, 1, overflow_list=1, numBuckets=64, bucketSize=2) if src_overflow
                     else source(vh, torch_cuda, oracle))
    if src_overflow:
        assert (src_snap["table"]["offset"] != 0).any()
    # 256 slots for the source's keys, some buckets the home of three: chains form, several rounds, all placed
    dst, twin = CC.table(vh, MC.DST_KW, numBuckets=128, bucketSize=2), CC.table(vh, MC.DST_KW, numBuckets=128, bucketSize=2)
    dst.set_option("overflow_list", 1)
    twin.set_option("overflow_list", 1)
    stats, cstats, post = merge_and_check(oracle, dst, twin, src, src_snap, MC.IDENTITY, TRILINEAR, 255)
    assert stats["rounds"] > 1 and (post["table"]["offset"] != 0).any() and cstats["fresh"] > 0
    dst.close()
    twin.close()


# ---- 7. ordering ---------------------------------------------------------------------------------------------------------------------------
def test_pending_frames_and_a_stream_of_its_own(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    results = []
    for eager in (False, True):
        src, dst = CC.table(vh, MC.SRC_KW), CC.table(vh, MC.DST_KW)
        if not eager:
            stream = torch.cuda.Stream()
            src.set_stream(stream)
            src.set_option("pipeline", 1)
            dst.set_option("pipeline", 1)
        images = [CC.dev(torch, frames[i][1]) for i in range(3)]
        colours = [CC.dev(torch, CC.image(i)) for i in range(3)]
        torch.cuda.synchronize()
        # colour from the first frame of each, then a depth frame that stays pending where frames are pipelined
        src.integrate_depth_color(frames[0][0], images[0], DC.k_inv(), colours[0], CC.BAND, 255)
        src.integrate_depth(frames[1][0], images[1], DC.k_inv())
        dst.integrate_depth_color(frames[2][0], images[2], DC.k_inv(), colours[2], CC.BAND, 255)
        dst.integrate_depth(frames[1][0], images[1], DC.k_inv())
        if eager:
            src.synchronize()
            dst.synchronize()
        stats = dst.merge(src, CC.CLOSE, TRILINEAR, colors=True)                  # no synchronisation of ours in between
        results.append((stats, CC.model(CC.snapshot(dst)), CC.model(CC.snapshot(src))))
        src.close()
        dst.close()
    (sa, a, srca), (sb, b, srcb) = results
    assert sa == sb and sa["allocated"] > 0
    for x, y in ((a, b), (srca, srcb)):
        assert x.keys() == y.keys()
        for k in x:
            assert all(np.array_equal(np.asarray(p).view(U), np.asarray(q).view(U)) for p, q in zip(x[k], y[k])), k
    assert sum(int((v[2] != 0).sum()) for v in a.values()) > 1000


# ---- 8. afterwards: the merged model is an ordinary coloured model --------------------------------------------------------------------------
def test_collection_sampling_and_the_mesh(oracle, vh, torch_cuda):
    torch = torch_cuda
    src, src_snap = source(vh, torch, oracle)
    dst = fused_dst(vh, torch, oracle)
    dst.merge(src, CC.CLOSE, TRILINEAR, colors=True)
    before = CC.snapshot(dst)
    dst.garbage_collect(float("inf"))
    snap = CC.snapshot(dst)
    freed = set(CC.model(before)) - set(CC.model(snap))
    assert len(freed) > 0 and snap["counters"]["last_freed"] == len(freed)
    held = np.zeros(len(snap["color"]), bool)
    tab = snap["table"]
    held[(tab["ptr"][tab["ptr"] != -1].astype(np.int64)[:, None] + np.arange(512)).ravel()] = True
    assert not snap["color"][~held].any() and snap["color"][held].any()            # zero colour in the freed blocks
    m = CC.model(snap)
    field = CR.ColorField(m)
    vs = dst.params.voxelSize
    keys = np.array(sorted(m), np.int64)
    rng = np.random.RandomState(43)
    pts = ((keys[rng.randint(0, len(keys), 4096)] * 8 + rng.uniform(-1, 9, (4096, 3))) * vs).astype(F)
    for mode in (NEAREST, TRILINEAR):
        want = CR.sample(field, pts, vs, mode)
        got = dst.sample_color(CC.dev(torch, pts), mode)
        dst.synchronize()
        assert (want != 0).sum() > 100 and np.array_equal(got.cpu().numpy(), want)
    verts, faces, colors = dst.extract_mesh_indexed(colors=True)
    near, tri = CR.sample(field, verts, vs, NEAREST), CR.sample(field, verts, vs, TRILINEAR)
    assert len(verts) > 100 and (tri != 0).sum() >= 100
    assert np.array_equal(colors, np.where(tri != 0, tri, near))
    dst.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle, vh, torch_cuda):
    torch = torch_cuda
    src, src_snap = source(vh, torch, oracle)
    dst = fused_dst(vh, torch, oracle)
    bare = fused_dst(vh, torch, oracle, colors=False)
    pre, bare_pre = CC.snapshot(dst), CC.snapshot(bare)
    lib = vh.load()
    fp = C.POINTER(C.c_float)

    def call(d, s, T, mode, weight_max=255):
        m = None if T is None else np.ascontiguousarray(np.asarray(T, F).reshape(16)).ctypes.data_as(fp)
        return lib.vh_merge_color(d, s, m, mode, weight_max, None)

    nan = MC.OBLIQUE.copy()
    nan[1, 2] = np.nan
    singular = np.zeros((4, 4), F)
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), W, H, 1)
    ball = MC.shell()
    view.import_view(torch.from_numpy(MM.view_records(ball)).cuda(), len(ball))
    for d in (dst, bare):
        for weight_max in (0, 256, -1):
            assert call(d._h, src._h, MC.IDENTITY, 1, weight_max) == INVALID
        assert call(None, src._h, MC.IDENTITY, 1) == INVALID and call(d._h, None, MC.IDENTITY, 1) == INVALID
        assert call(d._h, src._h, None, 1) == INVALID and call(d._h, d._h, MC.IDENTITY, 1) == INVALID
        for mode in (-1, 2):
            assert call(d._h, src._h, MC.IDENTITY, mode) == INVALID
        for T in (nan, singular):
            assert call(d._h, src._h, T, 1) == INVALID
    assert call(view._h, src._h, MC.IDENTITY, 1) == INVALID                        # dst holds an imported view
    with pytest.raises(vh.VoxelHashError, match="invalid argument"):
        dst.merge(src, MC.IDENTITY, colors=True, color_weight_max=0)
    CC.unchanged(pre, CC.snapshot(dst))
    CC.unchanged(bare_pre, CC.snapshot(bare))                                      # (no volume was allocated by a refused call)
    CC.unchanged(src_snap, CC.snapshot(src))
    for t in (dst, bare, view):
        t.close()


def test_close_shared_sources():
    for gt, _ in _SRC.values():
        gt.close()
    _SRC.clear()
