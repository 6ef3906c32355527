"""tests/merge_color_ref.py, the executable form of vh_merge_color's and vh_deintegrate_color's rules, without a GPU: the rule on
ball shells and on the room frames, the identity copy, the removal's properties, and a condition on the inputs of
tests/test_gpu_merge_color.py -- every colour branch is populated by the rule alone for the cases the GPU tests merge."""
import numpy as np
import pytest

import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as D
import merge_cases as MC
import merge_color_cases as CC
import merge_color_ref as M
import merge_ref as R

F = np.float32
U = np.uint32
BIG = 1e9


def inverse(T):
    return np.linalg.inv(np.asarray(T, np.float64)).astype(F)


@pytest.fixture(scope="module")
def ball():
    """A ball shell with a colour word per voxel: a count of 1..4, no colour on one voxel in seven."""
    rng = np.random.default_rng(8)
    out = {}
    for k, (s, w) in MC.shell().items():
        c = (rng.integers(0, 1 << 24, 512, dtype=np.uint64).astype(U) | (rng.integers(1, 5, 512).astype(U) << U(24))).astype(U)
        c[rng.integers(0, 7, 512) == 0] = 0
        out[k] = (s, w, c)
    return out


def test_nearest_identity_copies_every_word(ball):
    vs = F(2.0 ** -5)
    keys, _ = R.candidates(ball.keys(), MC.IDENTITY, vs, vs)
    out, gstats, cstats = M.apply(CC.with_new_blocks({}, keys), ball, keys, MC.IDENTITY, vs, vs, BIG, 255.0, R.NEAREST, 255)
    copied = 0
    for k, (s, w, c) in ball.items():
        valid = w > 0
        assert np.array_equal(out[k][0][valid].view(U), s[valid].view(U)) and np.array_equal(out[k][1][valid].view(U), w[valid].view(U))
        assert np.array_equal(out[k][2][valid], c[valid]) and not out[k][2][~valid].any()      # a dead voxel gives no colour
        copied += int((valid & (c != 0)).sum())
    assert cstats["fresh"] == copied > 1000 and cstats["combined"] == 0 and cstats["capped"] == 0
    assert cstats["no_sample"] == gstats["fresh"] - copied > 0
    # a cap below the counts binds, and only on the count
    capped, _, cs = M.apply(CC.with_new_blocks({}, keys), ball, keys, MC.IDENTITY, vs, vs, BIG, 255.0, R.NEAREST, 2)
    assert cs["capped"] > 0
    for k in ball:
        assert np.array_equal(capped[k][2] & U(0xFFFFFF), out[k][2] & U(0xFFFFFF))
        assert np.array_equal(CR.count(capped[k][2]), np.minimum(CR.count(out[k][2]), 2))


def test_the_geometry_is_merge_refs_and_the_colour_follows_the_tsdf_step(ball):
    vs = F(MC.VS)
    Tinv = inverse(MC.HALF_SHIFT)
    keys, _ = R.candidates(ball.keys(), MC.HALF_SHIFT, vs, vs)
    dst = {k: (v[0], v[1], np.where(v[1] > 0, CR.pack(9, 99, 199, 2), U(0)).astype(U)) for i, (k, v) in enumerate(sorted(ball.items()))
           if i % 2 == 0}
    before = CC.with_new_blocks(dst, keys)
    out, gstats, cstats = M.apply(before, ball, keys, Tinv, vs, vs, 3.0, 1.5, R.TRILINEAR, 3)
    want, wstats = R.apply(M.geometry(before), M.geometry(ball), keys, Tinv, vs, vs, 3.0, 1.5, R.TRILINEAR)
    assert gstats == wstats
    for k in want:
        assert np.array_equal(out[k][0].view(U), want[k][0].view(U)) and np.array_equal(out[k][1].view(U), want[k][1].view(U))
    assert all(n > 0 for n in cstats.values()), cstats
    assert cstats["fresh"] + cstats["combined"] + cstats["no_sample"] == gstats["fresh"] + gstats["combined"]
    s, w = R.samples(M.geometry(ball), sorted(keys), Tinv, vs, vs, R.TRILINEAR)
    for i, k in enumerate(sorted(keys)):
        took = (s[i] == s[i]) & (w[i] > 0)
        assert np.array_equal(out[k][2][~took], before[k][2][~took])                          # no TSDF step, no colour step
        assert (CR.count(out[k][2]) <= 3).all()
    # the uniform dst colour mixed with a uniform src colour stays between the two, per channel
    flat = {k: (v[0], v[1], np.full(512, CR.pack(100, 0, 255, 4), U)) for k, v in ball.items()}
    mixed, _, cs = M.apply(before, flat, keys, Tinv, vs, vs, 3.0, 1.5, R.TRILINEAR, 255)
    for k in mixed:
        changed = mixed[k][2] != before[k][2]
        r, g, b = CR.channels(mixed[k][2][changed])
        assert ((r >= 9) & (r <= 100) & (g <= 99) & (b >= 199)).all()
    assert cs["combined"] > 0 and cs["no_sample"] == 0
    # (6 * 9 + 4 * 100) / ... the weighted mean, rounded at one half: (2 * 9 + 4 * 100) / 6 = 69.67 -> 70
    assert int(M.combine(CR.pack(9, 99, 199, 2), CR.pack(100, 0, 255, 0), 4, 255)) == int(CR.pack(70, 33, 236, 6))
    assert int(M.combine(U(0), CR.pack(1, 2, 3, 0), 200, 7)) == int(CR.pack(1, 2, 3, 7))


# ---- a condition on the GPU tests' inputs ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rooms(oracle):
    return {sem: (CC.oracle_model(oracle, sem, CC.SRC_COLORS, **MC.SRC_KW), CC.oracle_model(oracle, sem, CC.DST_COLORS, **MC.DST_KW))
            for sem in (0, 1)}


@pytest.mark.parametrize("sem,name,transform,ratio,mode,weight_max", CC.SEM_CASES, ids=[f"sem{c[0]}-{c[1]}" for c in CC.SEM_CASES])
def test_every_colour_branch_is_populated_for_the_gpu_cases(oracle, rooms, sem, name, transform, ratio, mode, weight_max):
    src, dst = rooms[sem]
    assert 50 < len(src) < 512 and max(int(CR.count(v[2]).max()) for v in src.values()) == 4
    T = CC.TRANSFORMS[transform]
    vs_s, vs_d = F(MC.VS), F(MC.VS * ratio)
    keys, _ = R.candidates(src.keys(), T, vs_s, vs_d)
    before = CC.with_new_blocks(dst, keys)
    out, gstats, cstats = M.apply(before, src, sorted(keys), oracle.invert4x4(T), vs_s, vs_d, 1.0, 255.0, mode, weight_max)
    print(f"sem {sem} {name}: geometry {gstats}; colour {cstats}")
    need = ["fresh", "combined", "no_sample", "kept"] + (["capped"] if weight_max < 5 else [])
    assert all(cstats[n] > 0 for n in need), cstats
    assert max(int(CR.count(v[2]).max()) for v in out.values()) <= weight_max


# ---- the removal ---------------------------------------------------------------------------------------------------------------
def test_removing_the_last_sample_lands_within_one():
    rng = np.random.default_rng(9)
    n = 200000
    before = (rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(U) | (rng.integers(1, 254, n).astype(U) << U(24))).astype(U)
    pixel = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    back = M.unblend(CR.blend(before, pixel, 255), pixel)
    assert np.array_equal(CR.count(back), CR.count(before))
    worst = 0
    for a, b in zip(CR.channels(back), CR.channels(before)):
        worst = max(worst, int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()))
    assert worst == 1                                                      # within 1, and the bound is reached
    # one sample into nothing and out again: nothing
    assert not M.unblend(CR.blend(np.zeros(1000, U), pixel[:1000], 255), pixel[:1000]).any()
    assert int(M.unblend(CR.pack(200, 100, 0, 1), CR.pack(1, 2, 3, 0))) == 0
    # the clamp: (10 * 2 - 255) / 1 < 0 -> 0; (250 * 2 - 0) / 1 > 255 -> 255; (3 * 2 - 1) / 1 = 5
    assert int(M.unblend(CR.pack(10, 250, 3, 2), CR.pack(255, 0, 1, 77))) == int(CR.pack(0, 255, 5, 1))
    assert M.clamped(CR.pack(10, 250, 3, 2), CR.pack(255, 0, 1, 77)) == 2


def test_removal_on_the_room_frames(oracle):
    sem = 1
    ot = DC.oracle_table(oracle, sem)
    frames = DC.frames(oracle)
    for pose, _, verts in frames:
        ot.integrate(pose, verts)
    tab, vox = ot.hash_table().copy(), ot.sdf_blocks().copy()
    proj = DC.projection(sem)
    color = np.zeros(len(vox), U)
    history = []
    for i, (pose, d16, _) in enumerate(frames):
        inv = oracle.invert4x4(pose)
        entries = tab[D.visible_entries(tab, ot.params, sem, proj, pose, inv, DC.W, DC.H)]
        history.append(color)
        color, _ = CR.integrate(color, vox, entries, ot.params, sem, proj, inv, (d16, DC.k_inv()), CC.image(i), CC.BAND, 255)
    # the last frame out again: counts as before it, every channel within 1
    back, stats = M.deintegrate(color, vox, entries, ot.params, sem, proj, inv, (d16, DC.k_inv()), CC.image(2), CC.BAND)
    assert stats["removed"] > 1000 and stats["emptied"] > 0 and stats["swept"] == 0, stats
    assert np.array_equal(CR.count(back), CR.count(history[2]))
    assert not back[history[2] == 0].any()
    for a, b in zip(CR.channels(back), CR.channels(history[2])):
        assert int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()) <= 1
    # another image than the one that was fused: the clamp is reached
    _, wrong = M.deintegrate(color, vox, entries, ot.params, sem, proj, inv, (d16, DC.k_inv()), CC.image(7), CC.BAND)
    assert wrong["clamped"] > 0
    # a voxel that holds nothing loses its word, whatever the frame says
    hollow = vox.copy()
    at = int(np.nonzero(color)[0][0])
    hollow["weight"][at] = 0.0
    swept, st = M.deintegrate(color, hollow, entries, ot.params, sem, proj, inv, (d16, DC.k_inv()), CC.image(2), CC.BAND)
    assert st["swept"] == 1 and swept[at] == 0
    ot.close()
