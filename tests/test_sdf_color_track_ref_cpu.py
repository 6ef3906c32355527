"""The joint shape + colour alignment rule (tests/sdf_color_track_ref.py) pinned without a GPU: without a photometric row it is
tests/sdf_track_ref.py exactly, and on a flat textured wall, where the geometric system has three exactly zero columns and
takes no step, the photometric rows bring the in-plane pose back."""
import numpy as np

import color_ref as CR
import mesh_models as mm
import sample_ref as sr
import sdf_color_track_ref as cref
import sdf_track_ref as ref

F, U = np.float32, np.uint32
VS = 0.02
THRES = 0.25
POSE = ref.se3_exp([0.4, -0.3, 0.2, 0.3, -0.2, 0.25])


def noise_case(seed=7, n=1500):
    """mm.every_configuration() with random colour words (one in twenty with count 0: two cells in three have eight counted
    corners), points in the cells of its blocks (every 7th pixel without one) and an image of noise."""
    rng = np.random.RandomState(seed)
    plain = mm.every_configuration()
    words = {k: np.where(rng.uniform(size=512) < 0.05, 0, 1 << 24).astype(U) * rng.randint(1, 256, 512).astype(U)
             | rng.randint(0, 1 << 24, 512).astype(U) for k in plain}
    coloured = {k: (v[0], v[1], words[k]) for k, v in plain.items()}
    keys = np.array(list(plain), np.int64)
    world = (keys[rng.randint(0, len(keys), n)] * 8 + rng.uniform(0, 8, (n, 3))) * VS
    inv = np.linalg.inv(POSE)
    inp = np.concatenate([world @ inv[:3, :3].T + inv[:3, 3], np.ones((n, 1))], 1).astype(F)
    inp[::7] = 0
    rgba = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return plain, coloured, inp, rgba


def same_system(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


def test_without_a_photometric_row_it_is_the_geometric_rule():
    plain, coloured, inp, rgba = noise_case()
    blank = {k: (v[0], v[1], np.zeros(512, U)) for k, v in plain.items()}
    q, s, g, kept, _ = ref.pixels(plain, inp, POSE, VS, THRES)
    want_maps, want = ref.maps(q, s, g, kept), ref.system(q, s, g, kept)
    assert want[3] > 100
    # the joint rule does form rows on the coloured model: the variants below are not equal to it for want of colour
    px = cref.pixels(coloured, inp, rgba, POSE, VS, THRES, 0.1, 0.5)
    assert px[6].sum() > 20 and cref.system(*px, 0.1)[3] == want[3] + px[6].sum()
    for model, weight in ((coloured, 0.0), (blank, 0.1), (plain, 0.1)):
        px = cref.pixels(model, inp, rgba, POSE, VS, THRES, weight, 0.5)
        assert not px[6].any()
        got_maps = cref.maps(*px)
        assert all(sr.same_bits(a, b) for a, b in zip(got_maps[:3], want_maps))
        assert np.isnan(got_maps[3]).all() and not got_maps[4].any()
        assert same_system(cref.system(*px, weight), want)
        a = cref.align(model, inp, rgba, POSE, VS, THRES, weight, 0.5, 3)
        b = ref.align(plain, inp, POSE, VS, THRES, 3)
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and same_system(a[1], b[1])


def test_what_has_no_photometric_row():
    plain, coloured, inp, rgba = noise_case()
    q, s, g, kept, e, gC, photo = cref.pixels(coloured, inp, rgba, POSE, VS, THRES, 0.1, 0.3)
    field = CR.ColorField(coloured)
    i = np.floor((q / F(VS)).astype(F)).astype(np.int64)
    counts = np.stack([CR.count(field.words(i + np.array([c & 1, (c >> 1) & 1, c >> 2]))) for c in range(8)], 1)
    has = kept & (counts > 0).all(1)
    assert not photo[~kept].any() and np.isnan(e[~has]).all() and np.isfinite(e[has]).all()
    with np.errstate(invalid="ignore"):
        assert (photo == (has & (np.abs(e) < F(0.3)))).all()
    assert (kept & ~has).sum() > 20 and (has & ~photo).sum() > 20 and photo.sum() > 20
    # the model intensity is vh_sample_color's sample to the rounding of its bytes: |C - Y(sample)| <= 0.5 / 255 + rounding
    words = CR.sample(coloured, q[has], VS)
    assert (words != 0).all()
    C = e[has] + cref.luminance(rgba[has])
    assert np.abs(C - cref.luminance(words)).max() < 0.5 / 255 + 1e-6
    maps = cref.maps(q, s, g, kept, e, gC, photo)
    assert np.isnan(maps[3][~photo]).all() and not maps[4][~photo].any() and np.isfinite(maps[4][photo]).all()


# ---- the textured wall --------------------------------------------------------------------------------------------------------
WALL_Z = 1.007                 # between two voxel layers
W, H, FX = 160, 120, 140.0


def texture(x, y):
    """A smooth colour over the wall's plane, 8 bits per channel: (r, g, b) uint32."""
    r = 128 + 100 * np.sin(7.0 * x + 0.3) * np.cos(5.0 * y)
    g = 128 + 100 * np.sin(4.0 * x - 6.0 * y + 1.0)
    b = 128 + 100 * np.cos(6.5 * y - 0.7) * np.cos(3.0 * x + 0.2)
    return [np.rint(c).astype(U) for c in (r, g, b)]


def wall_model():
    """The plane z = WALL_Z in the blocks x -5..4, y -4..3, z 5..6: sdf = WALL_Z - z of the voxel, weight 1, the texture at the
    voxel's (x, y) with count 1."""
    i = np.arange(512)
    local = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    model = {}
    for k in mm.cube_keys((-5, -4, 5), (5, 4, 7)):
        gv = np.array(k) * 8 + local
        r, g, b = texture(gv[:, 0] * VS, gv[:, 1] * VS)
        model[k] = ((WALL_Z - gv[:, 2] * VS).astype(F), np.ones(512, F), CR.pack(r, g, b, 1))
    return model


def wall_frame(pose):
    """What a camera at `pose` (moved in the wall's plane and rolled about its normal only) sees of the wall: the float4 vertex
    map and the colour image."""
    v, u = np.mgrid[0:H, 0:W]
    rays = np.stack([(u - W / 2 + 0.5) / FX, (v - H / 2 + 0.5) / FX, np.ones((H, W))], -1).reshape(-1, 3)
    cam = rays * WALL_Z                                    # the camera's z axis is the wall's normal: depth WALL_Z everywhere
    world = cam @ pose[:3, :3].T + pose[:3, 3]
    r, g, b = texture(world[:, 0], world[:, 1])
    return np.concatenate([cam, np.ones((len(cam), 1))], 1).astype(F), CR.pack(r, g, b, 255)


def in_plane_error(pose, truth):
    d = np.linalg.inv(truth) @ pose
    return float(np.hypot(d[0, 3], d[1, 3])), float(np.degrees(abs(np.arctan2(d[1, 0], d[0, 0]))))


def test_a_textured_wall_is_tracked_where_geometry_alone_is_singular():
    model = wall_model()
    truth = ref.se3_exp([0.030, -0.022, 0.0, 0.0, 0.0, np.radians(1.2)])       # 37 mm in the plane, 1.2 degrees of roll
    inp, rgba = wall_frame(truth)
    start = np.eye(4)
    plain = {k: (v[0], v[1]) for k, v in model.items()}
    JTJ, JTr, err, count = ref.build_system(plain, inp, start, VS, 0.08)
    assert count == W * H and err != 0
    assert not JTJ[:, [0, 1, 5]].any() and not JTJ[[0, 1, 5], :].any()          # x, y and roll: exactly zero columns
    pose, _, steps = ref.align(plain, inp, start, VS, 0.08, 15)
    assert steps == 0 and np.array_equal(pose, start)
    e0 = in_plane_error(start, truth)
    for weight in (0.05, 0.1, 1.0):
        got, last, steps = cref.align(model, inp, rgba, start, VS, 0.08, weight, 0.2, 15)
        e1 = in_plane_error(got, truth)
        print(f"wall, color_weight {weight}: start {1e3 * e0[0]:.2f} mm / {e0[1]:.3f} deg, after {steps} rounds "
              f"{1e3 * e1[0]:.3f} mm / {e1[1]:.4f} deg, rows {last[3]} of {2 * W * H}")
        assert steps == 15 and last[3] > 1.5 * W * H
        assert e1[0] <= 0.5 * e0[0] and e1[1] <= 0.5 * e0[1]                  # the project's criterion for an Align
