"""No GPU: the float32 colour rules of tests/color_ref.py and tests/merge_color_ref.py against the integer forms of
tests/color_count_ref.py over every input (so the kernels have two independent references that agree), the sizes of the tie and
reciprocal-discriminator sets, the add-then-remove bound, and -- on the oracle's room model -- the coverage conditions of every
crafted input of tests/test_gpu_color_counts.py together with the power check: a copy of the rule whose division is a multiply
by the float32 reciprocal is rejected by every crafted input and by none of the inputs tests/test_gpu_color.py fuses."""
import numpy as np
import pytest

import color_count_cases as K
import color_count_ref as X
import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as D
import merge_color_cases as CC
import merge_color_ref as M
import merge_ref as R
import mesh_models as MM

F = np.float32
U = np.uint32
I = np.int64
NEAREST, TRILINEAR = 0, 1
OLD, NEW = [a.reshape(-1) for a in np.meshgrid(np.arange(256, dtype=I), np.arange(256, dtype=I), indexing="ij")]


def grid_words(w):
    """All (old, new) of one count in channel 0, two other mixes of the same bytes in channels 1 and 2."""
    words = CR.pack(OLD, 255 - OLD, (OLD * 7 + NEW * 13) & 255, np.full(len(OLD), w))
    pixels = CR.pack(NEW, (NEW * 5 + OLD) & 255, 255 - NEW, (OLD ^ NEW) & 255)                  # (byte 3: noise)
    return words, pixels


# ---- the rule with its division as a reciprocal multiply: what the tests must be able to reject ------------------------------------
def _rcp(num, den):
    return (num.astype(F) * (F(1.0) / den.astype(F)).astype(F)).astype(F)


def blend_rcp(word, pixel, weight_max):
    word, pixel = np.asarray(word, U), np.asarray(pixel, U)
    w = CR.count(word)
    out = np.minimum(w + U(1), U(weight_max)) << U(24)
    for k, old, new in zip((0, 8, 16), CR.channels(word), CR.channels(pixel)):
        f = _rcp(((old.astype(F) * w.astype(F)).astype(F) + new.astype(F)).astype(F), w + U(1))
        out = out | ((f + F(0.5)).astype(F).astype(U) << U(k))
    return out.astype(U)


def unblend_rcp(word, pixel):
    word, pixel = np.asarray(word, U), np.asarray(pixel, U)
    w = CR.count(word)
    out = (w - U(1)) << U(24)
    with np.errstate(all="ignore"):
        for k, old, new in zip((0, 8, 16), CR.channels(word), CR.channels(pixel)):
            f = _rcp(((old.astype(F) * w.astype(F)).astype(F) - new.astype(F)).astype(F), np.maximum(w, U(2)) - U(1))
            f = np.minimum(np.maximum(f, F(0.0)), F(255.0)).astype(F)
            out = out | ((f + F(0.5)).astype(F).astype(U) << U(k))
    return np.where(w == 1, U(0), out).astype(U)


def combine_rcp(word, rgb, w_s, weight_max):
    word, rgb, w_s = np.asarray(word, U), np.asarray(rgb, U), np.asarray(w_s, U)
    w_d = CR.count(word)
    cap = U(weight_max)
    fresh = rgb | (np.minimum(w_s, cap) << U(24))
    mixed = np.minimum(w_d + w_s, cap) << U(24)
    for k, old, new in zip((0, 8, 16), CR.channels(word), CR.channels(rgb)):
        f = _rcp(((old.astype(F) * w_d.astype(F)).astype(F) + (new.astype(F) * w_s.astype(F)).astype(F)).astype(F), w_d + w_s)
        mixed = mixed | ((f + F(0.5)).astype(F).astype(U) << U(k))
    return np.where(w_d == 0, fresh, mixed).astype(U)


# ---- 1. the float32 rules are exact round-half-up, everywhere ----------------------------------------------------------------------
@pytest.mark.parametrize("cap", [255, 254, 100, 1])
def test_blend_is_exact_on_all_triples(cap):
    ties = 0
    for w in range(256):
        words, pixels = grid_words(w)
        assert np.array_equal(CR.blend(words, pixels, cap), X.blend_exact(words, pixels, cap)), w
        ties += int(((2 * (OLD * w + NEW)) % (2 * (w + 1)) == w + 1).sum())
    print(f"cap {cap}: 2^24 (old, w, new) triples in channel 0, {ties} of them ties")
    assert ties > 100000


def test_unblend_is_exact_on_all_triples():
    clamped = 0
    for w in range(1, 256):
        words, pixels = grid_words(w)
        assert np.array_equal(M.unblend(words, pixels), X.unblend_exact(words, pixels)), w
        if w > 1:
            clamped += int(((OLD * w - NEW < 0) | (OLD * w - NEW > 255 * (w - 1))).sum())
    print(f"removal: {255 * 65536} (old, w, new) triples in channel 0, {clamped} of them clamped")
    assert clamped > 100000
    words = CR.pack(OLD, NEW, 7, 0)                                               # a count of 0: nothing to take out
    assert np.array_equal(X.unblend_exact(words, words), words)


@pytest.mark.parametrize("cap", [255, 100])
def test_combine_is_exact(cap):
    rng = np.random.default_rng(3)
    wd, ws = [a.reshape(-1) for a in np.meshgrid(np.arange(0, 256), np.arange(1, 256), indexing="ij")]
    wd, ws = np.repeat(wd, 64), np.repeat(ws, 64)                                 # every (wd, ws), the fresh branch included
    words = K.draw_words(rng, len(wd), None) & U(0xFFFFFF) | (wd.astype(U) << U(24))
    rgb = rng.integers(0, 1 << 24, len(wd)).astype(U)
    assert np.array_equal(M.combine(words, rgb, ws, cap), X.combine_exact(words, rgb, ws, cap))
    t = X.ties_combine()                                                          # every tie, in each channel in turn
    for ch in range(3):
        words = (rng.integers(0, 1 << 24, len(t)).astype(U) & ~U(255 << 8 * ch)) | (t[:, 4].astype(U) << U(8 * ch)) | (t[:, 2].astype(U) << U(24))
        rgb = (rng.integers(0, 1 << 24, len(t)).astype(U) & ~U(255 << 8 * ch)) | (t[:, 5].astype(U) << U(8 * ch))
        assert ((t[:, 4] * t[:, 2] + t[:, 5] * t[:, 3]) == t[:, 1]).all() and (t[:, 2] + t[:, 3] == t[:, 0]).all()
        assert np.array_equal(M.combine(words, rgb, t[:, 3], cap), X.combine_exact(words, rgb, t[:, 3], cap))


# ---- 2. the sets a test must cover ---------------------------------------------------------------------------------------------------
def test_tie_and_discriminator_sets():
    sets = {"add": (X.ties_add(), X.rcp_discriminators_add()), "remove": (X.ties_remove(), X.rcp_discriminators_remove()),
            "combine": (X.ties_combine(), X.rcp_discriminators_combine())}
    for name, (ties, rcp) in sets.items():
        print(f"{name}: {len(ties)} ties, {len(rcp)} reciprocal discriminators, the smallest count with one: {rcp[:, 0].min()}")
        assert len(rcp) > 0 and rcp[:, 0].min() > 8                               # (combine: the column is wd + ws; counts <= 4: <= 8)
        assert len(np.unique(ties[:, :2], axis=0)) == len(ties)
    assert len(sets["add"][0]) == 128 * 255 and len(sets["remove"][0]) == 127 * 255 and len(sets["combine"][0]) == 255 * 255
    # the copies of the rule above are what the discriminators describe: they differ from the rule exactly there
    for w in (int(sets["add"][1][:, 0].min()), int(sets["add"][1][:, 0].max())):
        words, pixels = grid_words(w)
        differ = CR.channels(blend_rcp(words, pixels, 255))[0] != CR.channels(CR.blend(words, pixels, 255))[0]
        listed = np.isin(K.codes(w, OLD * w + NEW), K.codes(*sets["add"][1].T))
        assert np.array_equal(differ, listed) and differ.any()
    t = sets["combine"][1]
    assert ((t[:, 4] * t[:, 2] + t[:, 5] * t[:, 3]) == t[:, 1]).all() and (t[:, 2] + t[:, 3] == t[:, 0]).all()
    words, rgb = CR.pack(t[:, 4], 0, 0, t[:, 2]), CR.pack(t[:, 5], 0, 0, 0)
    assert (combine_rcp(words, rgb, t[:, 3], 255) != M.combine(words, rgb, t[:, 3], 255)).all()


# ---- 3. add, then remove -----------------------------------------------------------------------------------------------------------------
def test_remove_after_add_restores_below_the_cap():
    worst = 0
    for w in range(0, 256):
        words, pixels = grid_words(w)
        if w == 0:
            words = np.zeros_like(words)                                          # (a count of 0 is the word 0 in a model)
        back = M.unblend(CR.blend(words, pixels, 255), pixels)
        assert (CR.count(back) == (w if w < 255 else 254)).all(), w               # at the cap a sample was forgotten
        if w <= 253:
            for a, b in zip(CR.channels(back), CR.channels(words)):
                worst = max(worst, int(np.abs(a.astype(I) - b.astype(I)).max()))
    print(f"add then remove, counts 0..253: the largest channel difference is {worst}")
    assert worst <= 1


# ---- 4. the crafted inputs of tests/test_gpu_color_counts.py: coverage and power, on the oracle's model ----------------------------------
@pytest.fixture(scope="module")
def rooms(oracle):
    return {sem: K.host_room(oracle, sem) for sem in (0, 1)}


def run_frames(oracle, room, vs, kind, sem, sensor, seed, most, cap=255, **fill):
    """The rounds of a frame goal on the host: (coverage, samples on which the reciprocal copy differs from the rule)."""
    cov, rejected = K.FrameCoverage(kind), 0
    for frame, chunk, image in K.frame_rounds(oracle, room, vs, kind, sem, sensor, seed, most, **fill):
        state = K.host_state(chunk)
        entries, at, take, pixel = K.frame_take(oracle, state, vs, sem, frame, sensor)
        words = state["color"][at]
        if kind == "remove":
            assert ((words == 0) & take).any()                                    # words of 0 under the frame
            take &= CR.count(words) > 0
        words, pixels = words[take], image.reshape(-1)[pixel[take]]
        cov.add(words, pixels)
        if kind == "add":
            exact, rule, copy = X.blend_exact(words, pixels, cap), CR.blend(words, pixels, cap), blend_rcp(words, pixels, cap)
        else:
            exact, rule, copy = X.unblend_exact(words, pixels), M.unblend(words, pixels), unblend_rcp(words, pixels)
        assert np.array_equal(exact, rule)
        rejected += int((copy != exact).sum())
    print(cov.report(), f"; the reciprocal copy differs on {rejected} samples")
    return cov, rejected


def test_crafted_add_covers_everything(oracle, rooms):
    cov, rejected = run_frames(oracle, *rooms[1], "add", 1, True, K.SEED_ADD, K.MOST_ROUNDS)
    cov.check_full()
    assert rejected > 0


@pytest.mark.parametrize("sem,sensor", K.OTHER_ADDS)
def test_crafted_add_of_the_other_instantiations(oracle, rooms, sem, sensor):
    cov, rejected = run_frames(oracle, *rooms[sem], "add", sem, sensor, K.SEED_ADD + 10, 1)
    cov.check_every_count(1000)
    assert rejected > 0


def test_crafted_removal_covers_everything(oracle, rooms):
    cov, rejected = run_frames(oracle, *rooms[1], "remove", 1, True, K.SEED_REMOVE, K.MOST_ROUNDS, zero=0.02)
    cov.check_full()
    assert rejected > 0


@pytest.mark.parametrize("cap", K.CAPS)
def test_crafted_cap_rounds(oracle, rooms, cap):
    room, vs = rooms[1]
    frame = DC.frames(oracle)[1]
    chunk, image = K.craft_frame(oracle, room, vs, 1, frame, True, K.SEED_CAPS + cap, counts=K.cap_counts(cap))
    state = K.host_state(chunk)
    entries, at, take, pixel = K.frame_take(oracle, state, vs, 1, frame, True)
    words, pixels = state["color"][at][take], image.reshape(-1)[pixel[take]]
    print(K.check_cap_counts(CR.count(words), cap))
    exact = X.blend_exact(words, pixels, cap)
    assert np.array_equal(exact, CR.blend(words, pixels, cap)) and (CR.count(exact) <= cap).all()
    if cap > 4:                                                                   # (below a count of 5 nothing tells the two apart)
        assert (blend_rcp(words, pixels, cap) != exact).any()


def test_crafted_merge_covers_everything(oracle, rooms):
    room, vs = rooms[1]
    cov, rejected = K.MergeCoverage(), 0
    for rnd in range(K.merge_rounds(room)):
        dst, src = K.craft_merge(room, rnd)
        dm, sm = K.chunk_model(dst), K.chunk_model(src)
        keys = sorted(dm)
        step, rgb, cnt = K.merge_take(sm, dm, keys, np.eye(4, dtype=F), vs, NEAREST)
        words = np.stack([dm[k][2] for k in keys])
        cov.add(words[step], rgb[step], cnt[step])
        for cap in (255, 100):
            exact = X.combine_exact(words[step], rgb[step], cnt[step], cap)
            assert np.array_equal(exact, M.combine(words[step], rgb[step], cnt[step], cap))
            n = int((combine_rcp(words[step], rgb[step], cnt[step], cap) != exact).sum())
            assert n > 0
            rejected += n
        assert ((words != 0) & ~step).any()                                       # the `kept` branch
    print(cov.report(), f"; the reciprocal copy differs on {rejected} samples")
    cov.check_full()


def test_crafted_half_voxel_merge(oracle):
    room, vs = K.host_room(oracle, 1, voxelSize=K.FINE_VS)
    assert vs == K.FINE_VS and 64 < len(room["keys"]) < 400
    src, dst = K.fine_words(room, K.SEED_FINE), K.craft_frame(oracle, room, vs, 1, DC.frames(oracle)[0], True, K.SEED_FINE + 1, plain_empty=True)[0]
    sm, dm = K.chunk_model(src), K.chunk_model(dst)
    keys = sorted(dm)
    Tinv = oracle.invert4x4(K.half_shift())
    held = np.array(sorted(set(keys) | R.candidates(keys, K.half_shift(), F(vs), F(vs))[0]), I)
    load = np.bincount(np.asarray(MM.hash_block(held, K.FINE_KW["numBuckets"]))).max()
    print(f"{len(keys)} blocks, {len(held)} with the candidates, at most {load} keys to a bucket")
    assert load < oracle.default_params().bucketSize                              # every candidate finds a slot
    step, rgb, cnt = K.merge_take(sm, dm, keys, Tinv, vs, TRILINEAR)
    words = np.stack([dm[k][2] for k in keys])
    t = K.half_weights(keys, Tinv, vs).reshape(len(keys), 512, 3)
    print(K.check_half_voxel(t[step], CR.count(words[step]), cnt[step], K.FINE_CAP))
    exact = X.combine_exact(words[step], rgb[step], cnt[step], K.FINE_CAP)
    assert np.array_equal(exact, M.combine(words[step], rgb[step], cnt[step], K.FINE_CAP))
    assert (combine_rcp(words[step], rgb[step], cnt[step], K.FINE_CAP) != exact).any()


def test_crafted_in_and_out(oracle, rooms):
    room, vs = rooms[1]
    frame = DC.frames(oracle)[1]
    chunk, image = K.craft_frame(oracle, room, vs, 1, frame, True, K.SEED_INOUT, counts=np.arange(254), plain_empty=True)
    state = K.host_state(chunk)
    entries, at, take, pixel = K.frame_take(oracle, state, vs, 1, frame, True)
    words, pixels = state["color"][at][take], image.reshape(-1)[pixel[take]]
    assert (np.bincount(CR.count(words), minlength=254)[:254] > 0).all() and CR.count(words).max() == 253
    added = X.blend_exact(words, pixels, 255)
    back = X.unblend_exact(added, pixels)
    print(K.check_restored(words, back))
    assert (blend_rcp(words, pixels, 255) != added).any() or (unblend_rcp(added, pixels) != back).any()


# ---- 5. the gap: what the suite fused before could not tell the two divisions apart ---------------------------------------------------------
def test_the_inputs_of_test_gpu_color_do_not_reject_the_reciprocal(oracle):
    """The schedule of tests/test_gpu_color.py's first test (three frames, one image each, weight_max 2) and the removal of
    tests/test_gpu_color_lifecycle.py's kind (the last frame taken back out), on the oracle's model."""
    frames = DC.frames(oracle)
    proj = DC.projection(1)
    ot = DC.oracle_table(oracle, 1)
    color = np.zeros(ot.params.numVoxelBlocks * 512, U)
    samples = 0
    for i, (pose, d16, verts) in enumerate(frames):
        ot.integrate(pose, verts)
        tab, vox = ot.hash_table().copy(), ot.sdf_blocks().copy()
        inv = oracle.invert4x4(pose)
        entries = tab[D.visible_entries(tab, ot.params, 1, proj, pose, inv, DC.W, DC.H)]
        at = entries["ptr"].astype(I)[:, None] + np.arange(512)[None, :]
        ok, s, sx, sy = CR.surface_samples(entries, ot.params, 1, proj, inv, (d16, DC.k_inv()))
        with np.errstate(invalid="ignore"):
            take = (vox["weight"][at] > 0) & ok & (np.abs(s) <= F(CC.BAND))
        words, pixels = color[at][take], CC.image(i)[sy[take], sx[take]]
        assert np.array_equal(blend_rcp(words, pixels, 2), CR.blend(words, pixels, 2))
        samples += int(take.sum())
        color, _ = CR.integrate(color, vox, entries, ot.params, 1, proj, inv, (d16, DC.k_inv()), CC.image(i), CC.BAND, 2)
    take &= CR.count(color[at]) > 0                                              # the last frame taken back out
    words, pixels = color[at][take], CC.image(2)[sy[take], sx[take]]
    assert np.array_equal(unblend_rcp(words, pixels), M.unblend(words, pixels))
    assert samples > 3000 and CR.count(color).max() == 2
    ot.close()
    # and of the merge cases: counts of at most 4 on either side
    wd, ws = [a.reshape(-1) for a in np.meshgrid(np.arange(1, 5), np.arange(1, 5), indexing="ij")]
    for a, b in zip(wd.tolist(), ws.tolist()):
        words, rgb = CR.pack(OLD, 0, 0, a), CR.pack(NEW, 0, 0, 0)
        assert np.array_equal(combine_rcp(words, rgb, np.full(len(OLD), b), 255), M.combine(words, rgb, np.full(len(OLD), b), 255))
