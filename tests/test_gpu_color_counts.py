"""The colour arithmetic of vh_integrate_color, vh_deintegrate_color and vh_merge_color at every sample count, 0..255, on the
crafted words of tests/color_count_cases.py: after every call the colour volume is downloaded and every word compared, bit for
bit, with the float32 rule (tests/color_ref.py, tests/merge_color_ref.py) and with the integer form of tests/color_count_ref.py
applied to the set the reference itself samples; nothing is excluded.  The coverage conditions -- every (count, old byte) pair,
every tie, every pair a reciprocal-multiply division would get wrong -- are conditions on the inputs, computed from the
reference's own `take` mask and asserted in each test; tests/test_color_count_ref_cpu.py proves them on the oracle's model and
shows that such a division is rejected by each of these inputs and by none the suite fused before."""
import numpy as np
import pytest

import color_count_cases as K
import color_count_ref as X
import color_ref as CR
import deintegrate_cases as DC
import merge_cases as MC
import merge_color_cases as CC
import merge_color_ref as M
import merge_ref as R
import stream_cases as SC

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
I = np.int64
NEAREST, TRILINEAR = 0, 1


@pytest.fixture(scope="module")
def rooms(oracle, vh, torch_cuda):
    """room(sem, **params) -> (chunk, voxel size): the three-frame room fused on the GPU and taken out whole, once each."""
    made = {}

    def room(sem, **kw):
        key = (sem, tuple(sorted(kw.items())))
        if key not in made:
            gt = CC.table(vh, DC.KW, sem, **kw)
            for pose, d16, _ in DC.frames(oracle):
                gt.integrate_depth(pose, CC.dev(torch_cuda, d16), DC.k_inv())
            gt.synchronize()
            assert gt.counters()["heap_exhausted"] == 0
            vs = float(gt.params.voxelSize)
            chunk = gt.stream_out(SC.EVERYTHING)
            assert chunk["selected"] == len(chunk["keys"]) and 50 < len(chunk["keys"]) < 400 and len(gt.allocated()) == 0
            gt.close()
            made[key] = (chunk, vs)
        return made[key]

    return room


def put(vh, gt, chunk):
    """Whatever the context holds goes out, `chunk` comes in, and every record is placed."""
    if len(gt.allocated()):
        gt.stream_out(SC.EVERYTHING)
    res = gt.stream_in(chunk)
    assert (res["status"] == vh.STREAM_PLACED).all() and res["placed"] == len(chunk["keys"]), res
    return gt


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


def frame_call(oracle, torch, gt, kind, sem, frame, sensor, image, cap=255, cov=None, zeros=False):
    """One colour call on the crafted context against both references; returns (words before, words after, pixels) of the
    sampled voxels."""
    pre = CC.snapshot(gt)
    entries, at, take, pixel = K.frame_take(oracle, pre, gt.params.voxelSize, sem, frame, sensor)
    assert (pre["vox"]["weight"][at] > 0).all() and take.sum() > 10000            # every voxel of a listed block holds something
    proj, inv, src = DC.projection(sem), oracle.invert4x4(frame[0]), K.depth_source(frame, sensor)
    before = pre["color"][at]
    if kind == "add":
        want, stats = CR.integrate(pre["color"], pre["vox"], entries, gt.params, sem, proj, inv, src, image, K.BAND, cap)
        assert stats["sampled"] == take.sum()
    else:
        want, stats = M.deintegrate(pre["color"], pre["vox"], entries, gt.params, sem, proj, inv, src, image, K.BAND)
        assert not zeros or ((before == 0) & take).any()                          # words of 0 under the frame: they stay 0
        take &= CR.count(before) > 0
        assert stats["removed"] == take.sum()
        print(f"removal: {stats}")
    words, pixels = before[take], image.reshape(-1)[pixel[take]]
    exact = pre["color"].copy()
    exact[at[take]] = X.blend_exact(words, pixels, cap) if kind == "add" else X.unblend_exact(words, pixels)
    assert np.array_equal(want, exact)                                            # the two references, on this input
    if cov is not None:
        cov.add(words, pixels)
    d16, verts, rgba = CC.dev(torch, frame[1]), CC.dev(torch, frame[2]), CC.dev(torch, image)
    if kind == "remove":
        gt.deintegrate_color(frame[0], d16, DC.k_inv(), rgba, K.BAND)
    elif sensor:
        gt.integrate_color(frame[0], d16, DC.k_inv(), rgba, K.BAND, cap)
    else:
        gt.integrate_color_map(frame[0], verts, rgba, K.BAND, cap)
    post = CC.snapshot(gt)
    for name in ("table", "heap", "vox"):                                         # the hash table, the heap, the SDF volume: unchanged
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    a, b = post["counters"], pre["counters"]
    assert a["heap_counter"] == b["heap_counter"] and a["epoch"] == b["epoch"] and a["occupied"] == len(entries)
    assert keys_of(post["compact"]) == keys_of(entries)
    bad = np.nonzero(post["color"] != want)[0]
    assert len(bad) == 0, (len(bad), bad[:4], pre["color"][bad[:4]], post["color"][bad[:4]], want[bad[:4]])
    return words, post["color"][at][take], pixels


def run_rounds(oracle, vh, torch, rooms, kind, sem, sensor, seed, most, **fill):
    room, vs = rooms(sem)
    gt = CC.table(vh, DC.KW, sem)
    cov = K.FrameCoverage(kind)
    emptied = 0
    for frame, chunk, image in K.frame_rounds(oracle, room, vs, kind, sem, sensor, seed, most, **fill):
        put(vh, gt, chunk)
        before, after, _ = frame_call(oracle, torch, gt, kind, sem, frame, sensor, image, 255, cov, zeros=kind == "remove")
        if kind == "remove":
            ones = (CR.count(before) == 1) & ((before & U(0xFFFFFF)) != 0)        # a count of 1 over bytes that are not 0:
            assert not after[ones].any()                                          # the whole word goes, not its count only
            emptied += int(ones.sum())
    print(cov.report())
    assert kind != "remove" or emptied >= 86                                      # (256 (1, old) pairs, three to a word)
    gt.close()
    return cov


# ---- 1. the add --------------------------------------------------------------------------------------------------------------------
def test_add_at_every_count_and_every_tie(oracle, vh, torch_cuda, rooms):
    cov = run_rounds(oracle, vh, torch_cuda, rooms, "add", 1, True, K.SEED_ADD, K.MOST_ROUNDS)
    cov.check_full()                                                              # counts 0, 254 and 255 included
    assert np.isin(K.codes(*cov.rcp.T), cov.codes).all()                          # every reciprocal discriminator was sampled


@pytest.mark.parametrize("cap", K.CAPS)
def test_add_under_a_cap(oracle, vh, torch_cuda, rooms, cap):
    room, vs = rooms(1)
    frame = DC.frames(oracle)[1]
    chunk, image = K.craft_frame(oracle, room, vs, 1, frame, True, K.SEED_CAPS + cap, counts=K.cap_counts(cap))
    gt = put(vh, CC.table(vh, DC.KW, 1), chunk)
    before, after, _ = frame_call(oracle, torch_cuda, gt, "add", 1, frame, True, image, cap)
    print(K.check_cap_counts(CR.count(before), cap))
    assert (CR.count(after) == np.minimum(CR.count(before) + 1, cap)).all()       # a count above the cap comes down at once
    gt.close()


@pytest.mark.parametrize("sem,sensor", K.OTHER_ADDS, ids=["vertex-map", "reference-semantics"])
def test_add_of_the_other_instantiations(oracle, vh, torch_cuda, rooms, sem, sensor):
    cov = run_rounds(oracle, vh, torch_cuda, rooms, "add", sem, sensor, K.SEED_ADD + 10, 1)
    cov.check_every_count(1000)


# ---- 2. the removal ------------------------------------------------------------------------------------------------------------------
def test_removal_at_every_count_tie_and_clamp(oracle, vh, torch_cuda, rooms):
    cov = run_rounds(oracle, vh, torch_cuda, rooms, "remove", 1, True, K.SEED_REMOVE, K.MOST_ROUNDS, zero=0.02)
    cov.check_full()


def test_one_image_in_and_out_again(oracle, vh, torch_cuda, rooms):
    room, vs = rooms(1)
    frame = DC.frames(oracle)[1]
    chunk, image = K.craft_frame(oracle, room, vs, 1, frame, True, K.SEED_INOUT, counts=np.arange(254), plain_empty=True)
    gt = put(vh, CC.table(vh, DC.KW, 1), chunk)
    before, added, _ = frame_call(oracle, torch_cuda, gt, "add", 1, frame, True, image, 255)
    assert (np.bincount(CR.count(before), minlength=254)[:254] > 0).all() and CR.count(before).max() == 253
    again, back, _ = frame_call(oracle, torch_cuda, gt, "remove", 1, frame, True, image)
    assert np.array_equal(again, added)                                           # (the same voxels: every count is >= 1 now)
    print(K.check_restored(before, back))
    gt.close()


# ---- 3. merging ------------------------------------------------------------------------------------------------------------------------
def merge_call(oracle, vh, dst_chunk, src_chunk, kw, T, mode, cap):
    """vh_merge_color of a crafted src into a crafted dst, and vh_merge into a twin of dst: the voxels are the twin's, the words
    both references'.  Returns (dst words before, samples (rgb, count), colour stats) over the voxels that take the step."""
    dst, twin, src = [put(vh, CC.table(vh, dict(MC.DST_KW, **kw)), c) for c in (dst_chunk, dict(dst_chunk, colors=None), src_chunk)]
    pre, src_snap = CC.snapshot(dst), CC.snapshot(src)
    stats = dst.merge(src, T, mode, colors=True, color_weight_max=cap)
    post = CC.snapshot(dst)
    CC.unchanged(src_snap, CC.snapshot(src))                                      # src's two volumes are only read
    assert stats == twin.merge(src, T, mode) and stats["unplaced"] == 0
    got, plain = CC.model(post), CC.model(CC.snapshot(twin))
    assert got.keys() == plain.keys()
    for k in got:                                                                 # the voxels: vh_merge's bits
        assert np.array_equal(got[k][0].view(U), plain[k][0].view(U)) and np.array_equal(got[k][1].view(U), plain[k][1].view(U)), k
    src_model, pre_model = CC.model(src_snap), CC.with_new_blocks(CC.model(pre), got.keys())
    vs = F(dst.params.voxelSize)
    present = sorted(R.candidates(src_model.keys(), T, vs, vs)[0] & set(got))
    assert keys_of(post["compact"]) == present
    Tinv = oracle.invert4x4(T)
    want, _, cstats = M.apply(pre_model, src_model, present, Tinv, vs, vs, dst.params.truncation, dst.params.integrationWeightMax,
                              mode, cap, merged={k: (v[0], v[1]) for k, v in plain.items()})
    step, rgb, cnt = K.merge_take(src_model, pre_model, present, Tinv, vs, mode)
    words = np.stack([pre_model[k][2] for k in present])
    exact = words.copy()
    exact[step] = X.combine_exact(words[step], rgb[step], cnt[step], cap)
    assert np.array_equal(exact, np.stack([want[k][2] for k in present]))         # the two references, on this input
    print(f"merge_color: {stats}; colour {cstats}")
    assert want.keys() == got.keys()
    for k in want:
        bad = np.nonzero(got[k][2] != want[k][2])[0]
        assert len(bad) == 0, (k, len(bad), bad[:4], pre_model[k][2][bad[:4]], got[k][2][bad[:4]], want[k][2][bad[:4]])
    for t in (dst, twin, src):
        t.close()
    return words[step], rgb[step], cnt[step], cstats, present, Tinv, step


@pytest.mark.parametrize("cap", [255, 100])
def test_identity_nearest_merge_at_every_pair_of_counts(oracle, vh, torch_cuda, rooms, cap):
    room, vs = rooms(1)
    cov = K.MergeCoverage()
    for rnd in range(K.merge_rounds(room)):
        dst, src = K.craft_merge(room, rnd)
        words, rgb, cnt, cstats, *_ = merge_call(oracle, vh, dst, src, {}, MC.IDENTITY, NEAREST, cap)
        cov.add(words, rgb, cnt)
        assert all(cstats[n] > 0 for n in ("fresh", "combined", "capped", "kept")), cstats
    print(cov.report())
    cov.check_full()


@pytest.fixture(scope="module")
def fine(oracle, rooms):
    """The room at voxelSize 2^-5 with the words of the half-voxel cases: (src chunk, dst chunk, voxel size)."""
    room, vs = rooms(1, voxelSize=K.FINE_VS)
    assert vs == K.FINE_VS
    dst = K.craft_frame(oracle, room, vs, 1, DC.frames(oracle)[0], True, K.SEED_FINE + 1, plain_empty=True)[0]
    return K.fine_words(room, K.SEED_FINE), dst, vs


def test_half_voxel_trilinear_merge(oracle, vh, torch_cuda, fine):
    src, dst, vs = fine
    words, rgb, cnt, cstats, present, Tinv, step = merge_call(oracle, vh, dst, src, K.FINE_KW, K.half_shift(), TRILINEAR,
                                                              K.FINE_CAP)
    t = K.half_weights(present, Tinv, vs).reshape(len(present), 512, 3)
    print(K.check_half_voxel(t[step], CR.count(words), cnt, K.FINE_CAP))
    assert all(cstats[n] > 0 for n in ("fresh", "combined", "capped"))


# ---- 4. reading back -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [NEAREST, TRILINEAR], ids=["nearest", "trilinear"])
def test_a_count_never_leaks_into_a_sample(vh, torch_cuda, fine, mode):
    src, _, vs = fine
    gt = put(vh, CC.table(vh, DC.KW, 1, voxelSize=vs), src)
    field = CR.ColorField(K.chunk_model(src))
    g = (np.asarray(src["keys"], I)[::4, None, :] * 8 + K.LOCAL[None, :, :]).reshape(-1, 3)
    stored = CR.count(field.words(g))
    assert all((stored == c).sum() > 100 for c in (1, 2, 254, 255))
    for name, pts in (("lattice", g.astype(F) * F(vs)), ("half-lattice", (g.astype(F) + F(0.5)) * F(vs))):
        assert np.array_equal((pts / F(vs)).astype(F), g.astype(F) + F(0.0 if name == "lattice" else 0.5))      # exactly there
        want = CR.sample(field, pts, vs, mode)
        got = gt.sample_color(CC.dev(torch_cuda, pts), mode)
        gt.synchronize()
        got = got.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, len(bad), pts[bad[:4]], got[bad[:4]], want[bad[:4]])
        assert (want != 0).sum() > 1000 and np.isin(got >> U(24), (0, 255)).all() and not got[(got >> U(24)) == 0].any()
        print(f"{name}: {len(pts)} points, {(want != 0).sum()} with a colour")
        if name == "lattice" and mode == NEAREST:                                 # the voxel's own bytes under 0xFF, whatever its count
            assert np.array_equal(got, (field.words(g) & U(0xFFFFFF)) | U(0xFF000000))
    gt.close()
