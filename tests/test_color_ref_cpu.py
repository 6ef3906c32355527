"""The colour rule without a GPU: properties of tests/color_ref.py (include/voxelhash.h, "the model in colour") on the oracle's
model of the small room scenes (tests/deintegrate_cases.py)."""
import numpy as np
import pytest

import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as R

F = np.float32
U = np.uint32
VS = DC.KW["voxelSize"]


def image(seed):
    """A colour image that differs per pixel and per seed; byte 3 is noise the rule must ignore."""
    return np.random.default_rng(seed).integers(0, 1 << 32, (DC.H, DC.W), dtype=np.uint64).astype(U)


@pytest.fixture(scope="module")
def scene(oracle):
    """The oracle's model of the three frames (PINHOLE), its table, volume and the compact set of frame 1's pose."""
    ot = DC.oracle_table(oracle, 1)
    frames = DC.frames(oracle)
    for pose, _, verts in frames:
        ot.integrate(pose, verts)
    pose, d16, verts = frames[1]
    proj, inv = DC.projection(1), oracle.invert4x4(pose)
    tab, vox = ot.hash_table().copy(), ot.sdf_blocks().copy()
    entries = tab[R.visible_entries(tab, ot.params, 1, proj, pose, inv, DC.W, DC.H)]
    out = dict(params=ot.params, proj=proj, inv=inv, tab=tab, vox=vox, entries=entries, src=(d16, DC.k_inv()), pose=pose)
    yield out
    ot.close()


def fuse(sc, color, rgba, band, weight_max, vox=None):
    return CR.integrate(color, sc["vox"] if vox is None else vox, sc["entries"], sc["params"], 1, sc["proj"], sc["inv"], sc["src"],
                        rgba, band, weight_max)


def test_identical_samples_leave_the_colour_unchanged():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 1 << 24, 4096, dtype=np.uint64).astype(U)
    for w in (0, 1, 2, 7, 100, 254, 255):
        got = CR.blend(rgb | U(w << 24), rgb | U(0xAB000000), 255)         # (byte 3 of the pixel is ignored)
        assert np.array_equal(got & U(0xFFFFFF), rgb)
        assert (CR.count(got) == min(w + 1, 255)).all()


def test_the_cap_makes_a_window():
    word = CR.pack(10, 20, 30, 0)
    seen = []
    for value in (100, 100, 200, 0, 255):
        word = CR.blend(word, CR.pack(value, value, value, 0), 2)
        seen.append((int(word & U(255)), int(CR.count(word))))
    # w: 0 -> 1 -> 2 -> 2 ..., and at the cap each step is (2 * old + in) / 3
    assert seen == [(100, 1), (100, 2), (133, 2), (89, 2), (144, 2)]


def test_rounding_at_one_half():
    # (1 * 1 + 2) / 2 = 1.5 -> 2; (0 * 1 + 1) / 2 = 0.5 -> 1; (2 * 3 + 0) / 4 = 1.5 -> 2; (2 * 3 + 4) / 4 = 2.5 -> 3
    assert int(CR.blend(CR.pack(1, 0, 2, 1), CR.pack(2, 1, 0, 0), 255)) == int(CR.pack(2, 1, 1, 2))
    assert int(CR.blend(CR.pack(2, 2, 2, 3), CR.pack(0, 4, 1, 0), 255)) & 0xFFFFFF == int(CR.pack(2, 3, 2, 0))
    assert int(CR.blend(CR.pack(2, 0, 0, 1), CR.pack(0, 0, 0, 0), 255)) == int(CR.pack(1, 0, 0, 2))


def test_a_uniform_image_gives_uniform_colours(scene):
    empty = np.zeros(len(scene["vox"]), U)
    rgba = np.full((DC.H, DC.W), 0x00C86432, U)
    one, stats = fuse(scene, empty, rgba, 1.5 * VS, 255)
    assert stats["sampled"] > 1000 and stats["rejected"] > 0
    assert set(np.unique(one).tolist()) == {0, 0x01C86432}
    two, _ = fuse(scene, one, rgba, 1.5 * VS, 255)
    assert set(np.unique(two).tolist()) == {0, 0x02C86432}
    assert np.array_equal(one != 0, two != 0)
    # voxels that hold nothing never receive colour, blocks outside the list are untouched
    assert not one[~(scene["vox"]["weight"] > 0)].any()
    listed = np.zeros(len(one), bool)
    listed[(scene["entries"]["ptr"].astype(np.int64)[:, None] + np.arange(512)).ravel()] = True
    marked = np.where(listed, one, U(7))
    again, _ = fuse(scene, marked, rgba, 1.5 * VS, 0)
    assert (again[~listed] == 7).all()


def test_a_larger_band_colours_a_superset(scene):
    empty = np.zeros(len(scene["vox"]), U)
    rgba = image(3)
    thin, st = fuse(scene, empty, rgba, 0.5 * VS, 255)
    wide, sw = fuse(scene, empty, rgba, 3.0 * VS, 255)
    assert 0 < st["sampled"] < sw["sampled"]
    assert not ((thin != 0) & (wide == 0)).any()
    assert np.array_equal(wide[thin != 0], thin[thin != 0])                # and the same colour where both have one


def test_the_sweep_clears_what_holds_nothing_and_adds_nothing(scene):
    empty = np.zeros(len(scene["vox"]), U)
    one, _ = fuse(scene, empty, image(4), 3.0 * VS, 255)
    vox = scene["vox"].copy()
    at = int(scene["entries"]["ptr"][0])
    coloured = np.nonzero(one[at:at + 512])[0]
    assert len(coloured) > 0
    vox["weight"][at + coloured[0]] = 0.0                                   # as a de-integration leaves it
    swept, stats = fuse(scene, one, image(5), 3.0 * VS, 0, vox)
    assert stats == dict(swept=1, rejected=stats["rejected"], sampled=0)
    want = one.copy()
    want[at + coloured[0]] = 0
    assert np.array_equal(swept, want)


def model_with(colour_of):
    """Two blocks side by side in x, every voxel valid, the colour word of voxel g given by colour_of(gx, gy, gz)."""
    model = {}
    for key in ((0, 0, 0), (1, 0, 0)):
        lin = np.arange(512)
        g = np.stack([key[0] * 8 + (lin & 7), key[1] * 8 + ((lin >> 3) & 7), key[2] * 8 + (lin >> 6)], 1)
        model[key] = (np.full(512, 0.01, F), np.ones(512, F), colour_of(g).astype(U))
    return model


def test_a_trilinear_sample_of_a_uniform_field_is_that_colour():
    word = CR.pack(17, 0, 255, 9)
    model = model_with(lambda g: np.full(len(g), word, U))
    rng = np.random.default_rng(6)
    pts = (rng.random((500, 3)) * np.array([14.0, 6.0, 6.0]) + 0.5).astype(F) * F(VS)
    for mode in (CR.NEAREST, CR.TRILINEAR):
        got = CR.sample(model, pts, VS, mode)
        assert (got == CR.pack(17, 0, 255, 255)).all()


def test_sampling_edges():
    ramp = model_with(lambda g: CR.pack(g[:, 0] * 10, 255 - g[:, 1], g[:, 2], 1))
    # halfway between voxels 3 and 4 in x: (30 + 40) / 2 = 35; across the block face 7 | 8: 75
    p = np.array([[3.5, 2.0, 2.0], [7.5, 2.0, 2.0]], F) * F(VS)
    got = CR.sample(ramp, p, VS, CR.TRILINEAR)
    assert [int(w) & 255 for w in got] == [35, 75] and (CR.count(got) == 255).all()
    # one uncoloured corner: no trilinear sample, the nearest of a coloured neighbour stays
    key = (0, 0, 0)
    s, w, c = ramp[key]
    c = c.copy()
    c[(2 << 6) | (2 << 3) | 4] = 0                                          # voxel (4, 2, 2)
    holed = dict(ramp)
    holed[key] = (s, w, c)
    assert int(CR.sample(holed, p[:1], VS, CR.TRILINEAR)[0]) == 0
    assert int(CR.sample(holed, np.array([[3.2, 2.0, 2.0]], F) * F(VS), VS, CR.NEAREST)[0]) != 0
    assert int(CR.sample(holed, np.array([[3.9, 2.0, 2.0]], F) * F(VS), VS, CR.NEAREST)[0]) == 0
    # real black is not "none"; an absent block, NaN and out-of-domain points have none
    black = model_with(lambda g: np.full(len(g), CR.pack(0, 0, 0, 1), U))
    q = np.array([[1.0, 1.0, 1.0], [40.0, 1.0, 1.0], [np.nan, 1.0, 1.0], [1.0, 3e30, 1.0]], F) * F(VS)
    for mode in (CR.NEAREST, CR.TRILINEAR):
        assert CR.sample(black, q, VS, mode).tolist() == [0xFF000000, 0, 0, 0]
    # the camera-frame form: z == 0 is no point
    pose = np.eye(4, dtype=F)
    pose[0, 3] = F(VS)
    cam = np.array([[0.0, VS, VS, 1.0], [0.0, VS, 0.0, 1.0]], F)
    assert CR.sample_map(black, pose, cam, VS, CR.NEAREST).tolist() == [0xFF000000, 0]
