"""The point-to-SDF alignment rule (tests/sdf_track_ref.py) pinned without a GPU: on a model whose sdf is linear the trilinear
sample reproduces the field, so Gauss-Newton from a known small twist must come back to the pose; and the four reasons a
pixel is not kept."""
import numpy as np

import mesh_models as mm
import sample_ref as sr
import sdf_track_ref as ref

F = np.float32
VS = 0.02
AT = 0.31                     # the three planes x = AT, y = AT, z = AT: through the cell layer 15 | 16, across a block face


def three_planes():
    """Three slabs of 2 x 2 x 2 blocks, each holding the signed distance (metres) to its own plane: x - AT in the blocks
    (1..2, 3..4, 3..4), y - AT in (3..4, 1..2, 3..4), z - AT in (3..4, 3..4, 1..2).  No two slabs share a face, so every cell
    with eight valid corners lies in one linear field."""
    i = np.arange(512)
    local = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    model = {}
    for axis in range(3):
        lo, hi = [3, 3, 3], [5, 5, 5]
        lo[axis], hi[axis] = 1, 3
        for k in mm.cube_keys(lo, hi):
            g = np.array(k)[axis] * 8 + local[:, axis]
            model[k] = ((g * VS - AT).astype(F), np.ones(512, F))
    return model


def plane_points(rng, n, spread=0.0):
    """World points on the three planes (or within `spread` of them), over the middle of each slab."""
    out = []
    for axis in range(3):
        p = rng.uniform(27 * VS, 37 * VS, (n, 3))
        p[:, axis] = AT + rng.uniform(-spread, spread, n)
        out.append(p)
    return np.concatenate(out)


def camera_map(world, pose):
    """The float4 input map (one row) that `pose` moves onto the world points."""
    inv = np.linalg.inv(pose)
    cam = world @ inv[:3, :3].T + inv[:3, 3]
    return np.concatenate([cam, np.ones((len(cam), 1))], 1).astype(F)


TRUE = ref.se3_exp([0.4, -0.3, 0.2, 0.3, -0.2, 0.25]) @ np.diag([1.0, 1.0, 1.0, 1.0])


def test_the_trilinear_sample_reproduces_a_linear_field():
    model = three_planes()
    world = plane_points(np.random.RandomState(1), 200, spread=0.05)
    s, w, g = sr.sample(model, world.astype(F), VS, sr.TRILINEAR)
    assert (w == 1).all()
    for axis in range(3):
        rows = slice(200 * axis, 200 * (axis + 1))
        want = world[rows, axis].astype(F).astype(np.float64) - AT
        assert np.abs(s[rows] - want).max() < 2e-6            # a few ulps of 0.5 m in the corner values
        normal = np.zeros(3)
        normal[axis] = 1
        assert np.abs(g[rows] - normal).max() < 1e-4          # differences of two such values over 0.02


def test_align_recovers_a_known_twist():
    model = three_planes()
    world = plane_points(np.random.RandomState(2), 300)
    inp = camera_map(world, TRUE)
    start = ref.se3_exp([0.006, -0.004, 0.005, 0.004, -0.003, 0.005]) @ TRUE
    assert np.abs(start[:3, 3] - TRUE[:3, 3]).max() > 3e-3
    first = ref.build_system(model, inp, start, VS, 0.08)
    assert first[3] == len(world)
    got, last, steps = ref.align(model, inp, start, VS, 0.08, 10)
    assert steps == 10 and last[3] == len(world)
    err = np.abs(got - TRUE).max()
    print(f"pose error after 10 rounds: {err:.3e} (start {np.abs(start - TRUE).max():.3e})")
    # measured on the CPU: 2.9e-08 (the float32 input points and the float32 copy of the pose set the floor); 10 x that
    assert err < 2.9e-7


def test_what_is_not_kept():
    model = three_planes()
    world = np.array([[AT, 0.62, 0.66],           # kept
                      [AT, 0.63, 0.67],           # (its input row is zeroed below: z == 0, no point)
                      [AT, 2.00, 0.66],           # outside the model: no sample
                      [AT + 0.05, 0.62, 0.66],    # |s| = 0.05 >= 0.03
                      [AT + 0.02, 0.62, 0.66]])   # |s| = 0.02: kept
    inp = camera_map(world, TRUE)
    inp[1] = 0
    q, s, g, kept, sampled = ref.pixels(model, inp, TRUE, VS, 0.03)
    assert kept.tolist() == [True, False, False, False, True]
    assert sampled.tolist() == [True, False, False, True, True]
    assert np.isnan(s[1]) and np.isnan(s[2]) and abs(s[3] - 0.05) < 1e-5
    points, sdf, grad = ref.maps(q, s, g, kept)
    assert (points[1] == 0).all() and (points[2] != 0).all()
    assert np.isnan(sdf[[1, 2, 3]]).all() and (grad[[1, 2, 3]] == 0).all() and abs(grad[0, 0] - 1) < 1e-4
    assert ref.system(q, s, g, kept)[3] == 2
    # a non-finite gradient: cells of mm.non_finite() with eight valid corners, one of them +-inf
    model = mm.non_finite()
    rng = np.random.RandomState(3)
    p = np.concatenate([rng.uniform(-9, 9, (4000, 3)) * VS, np.ones((4000, 1))], 1).astype(F)
    q, s, g, kept, sampled = ref.pixels(model, p, np.eye(4), VS, 10.0)
    bad = sampled & ~np.isfinite(g).all(1)
    print(f"non_finite: sampled {sampled.sum()}, with a non-finite gradient {bad.sum()}, kept {kept.sum()}")
    assert bad.sum() >= 20 and not kept[bad].any()
    assert (kept == (sampled & ~bad & (np.abs(s) < 10))).all() and kept.sum() > 500
