"""The rule of the block silhouettes (tests/blocks_ref.py) against answers written by hand and against a scalar restatement;
the oracle's vho_render_blocks against the rule, bit for bit, on every crafted case (tests/blocks_cases.py) -- which shows that
the oracle's screen box and depth pre-test remove nothing on these inputs; and every condition a case claims, asserted on the
rule's masks alone.  No GPU."""
import numpy as np
import pytest

import blocks_cases as bc
import blocks_ref as br
import mesh_models as mm

F = np.float32
EYE = np.eye(4, dtype=F)


def at(eye, R=np.eye(3)):
    return bc.pose_of(R, eye)


# ---- 1. answers written by hand ----------------------------------------------------------------------------------------
def test_one_cube_head_on():
    """Block (0, 0, 6) = [0, 0.16]^2 x [0.96, 1.12] from (0.08, 0.08, 0), 5x5 pixels 0.04 apart in tangent.  The middle 3x3
    (tangents up to 0.04: 0.045 m off the axis at the back face, the cube reaches 0.08) enter through the front face and leave
    through the back face: the two face depths exactly.  The outer pixels (tangent 0.08: 0.077 m at the front face) still enter
    through the front face and leave through a side at depth 0.08 / 0.08 = 1."""
    f, b, kept = br.render([(0, 0, 6)], 0.02, 5, 5, 25.0, 25.0, 2.0, 2.0, at((0.08, 0.08, 0.0)), 0.1, 5.0)
    lo, hi = br.cubes([(0, 0, 6)], 0.02)
    assert lo[0, 2] == F(48.0) * F(0.02) and hi[0, 2] == F(56.0) * F(0.02)
    inner = np.zeros((5, 5), bool)
    inner[1:4, 1:4] = True
    assert (f[inner] == lo[0, 2]).all() and (b[inner] == hi[0, 2]).all()
    assert (f[~inner] == lo[0, 2]).all() and np.allclose(b[~inner], 1.0, atol=1e-6)
    assert kept.shape == (1, 5, 5) and kept.all()
    # from half a metre off to the side nothing is hit
    f, b, kept = br.render([(0, 0, 6)], 0.02, 5, 5, 25.0, 25.0, 2.0, 2.0, at((0.7, 0.08, 0.0)), 0.1, 5.0)
    assert not f.any() and not b.any() and not kept.any()


def test_camera_on_a_face_and_the_plus_zero_rule():
    """The camera centre on the cube's front face z = 0.96, looking in: the entry depth is (0.96 - 0.96) / 1 = 0, clipped to
    t_min.  Looking AWAY from there (d_z = -1) with t_min = 0: t = (lo - o) / d = 0 / -1 = -0 and (hi - o) / d = -0.16, so tFar =
    -0, which is not below t_min = 0: the cube is kept and both images hold +0, never -0.  On the back face looking back: entry
    fmin(0.16, -0) = -0, stored as +0; exit the cube's depth."""
    lo, hi = br.cubes([(0, 0, 6)], 0.02)
    zf, zb = lo[0, 2], hi[0, 2]
    one = ([(0, 0, 6)], 0.02, 1, 1, 50.0, 50.0, 0.0, 0.0)
    f, b, _ = br.render(*one, at((0.08, 0.08, zf)), 0.1, 5.0)
    assert f[0, 0] == F(0.1) and b[0, 0] == zb - zf
    f, b, kept = br.render(*one, at((0.08, 0.08, zf), bc.YAW180), 0.0, 5.0)
    assert kept.all() and f.view(np.uint32)[0, 0] == 0 and b.view(np.uint32)[0, 0] == 0
    f, b, kept = br.render(*one, at((0.08, 0.08, zb), bc.YAW180), 0.0, 5.0)
    assert kept.all() and f.view(np.uint32)[0, 0] == 0 and b[0, 0] == zb - zf
    # with any t_min above 0 the cube behind the face is not kept
    assert not br.render(*one, at((0.08, 0.08, zf), bc.YAW180), 1e-6, 5.0)[2].any()


def test_cube_behind_the_camera_and_the_depth_range():
    key = [(0, 0, 6)]
    args = (0.02, 3, 3, 50.0, 50.0, 1.0, 1.0)
    f, b, kept = br.render(key, *args, at((0.08, 0.08, 2.0)), 0.1, 5.0)                 # 0.88 m behind
    assert not f.any() and not b.any() and not kept.any()
    f, b, kept = br.render(key, *args, at((0.08, 0.08, 2.0), bc.YAW180), 0.1, 5.0)      # turned round: 0.88 .. 1.04 in front
    assert kept.all() and np.allclose(f, 0.88, atol=1e-6) and np.allclose(b, 1.04, atol=1e-6)
    f, b, kept = br.render(key, *args, EYE.copy(), 0.1, 0.95)                           # wholly beyond t_max
    assert not kept.any() and not b.any()
    f, b, kept = br.render(key, *args, at((0.08, 0.08, 0.0)), 0.1, 1.0)                 # cut by t_max
    assert kept.all() and (b == F(1.0)).all() and (f == F(48.0) * F(0.02)).all()
    f, b, kept = br.render(key, *args, at((0.08, 0.08, 0.0)), 1.0, 5.0)                 # cut by t_min
    assert kept.all() and (f == F(1.0)).all()
    f, b, kept = br.render(key, *args, at((0.08, 0.08, 0.0)), 1.2, 5.0)                 # wholly nearer than t_min
    assert not kept.any() and not f.any()


def test_keys_wrap_and_scale():
    lo, hi = br.cubes([(-3, 1 << 28, (1 << 28) - 1)], 0.5)
    assert lo.tolist() == [[-12.0, -2.0 ** 30, 2.0 ** 30]] and hi[0, 0] == -8.0     # 8 * 2^28 wraps to -2^31; 2^31 - 8 rounds to 2^31


# ---- 2. the vectorised rule against the scalar restatement -------------------------------------------------------------
@pytest.mark.parametrize("name", ["shape_7x5", "near_plane_1_corner", "camera_inside", "t_max_cut", "shape_1x9"])
def test_scalar_restatement(name):
    c = bc.case(name)
    keys = c.keys[:: max(1, len(c.keys) // 12)]
    W, H = min(c.W, 9), min(c.H, 6)
    for v in c.views:
        a = br.render(keys, c.voxel_size, W, H, c.fx, c.fy, c.cx, c.cy, v.pose, v.t_min, v.t_max, batch=5)
        b = br.render_scalar(keys, c.voxel_size, W, H, c.fx, c.fy, c.cx, c.cy, v.pose, v.t_min, v.t_max)
        assert br.same_bits(a[0], b[0]) and br.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a zero direction component (pixel column 0 with cx = 0 under the identity attitude) takes the inside test
    a = br.render([(0, 0, 3), (1, 0, 3)], 0.02, 2, 2, 10.0, 10.0, 0.0, 0.0, at((0.16, 0.05, 0.0)), 0.1, 5.0)
    b = br.render_scalar([(0, 0, 3), (1, 0, 3)], 0.02, 2, 2, 10.0, 10.0, 0.0, 0.0, at((0.16, 0.05, 0.0)), 0.1, 5.0)
    assert br.same_bits(a[0], b[0]) and br.same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[2][:, 0, 0].all()                                                   # on the shared face: inside both (lo <= o <= hi)


# ---- 3. every condition, on the rule alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.names())
def test_conditions(name):
    c = bc.case(name)
    for i in range(len(c.views)):
        facts = bc.check(c, i, *c.expected(i))
        r = facts["regions"]
        print(f"{name} view {i}: blocks={facts['blocks']} kept={facts['kept']} nonzero={facts['nonzero']}/{facts['pixels']} "
              f"regions={r.shape[1]}x{r.shape[0]} max={int(r.max())} " + " ".join(f"{k}={v}" for k, v in facts.items()
                                                                                  if k in ("corners", "at_t_max")))
    # the crafted table holds the keys: no bucket of the case's table is overrun
    mm.place(c.model(), c.table["numBuckets"], c.table["bucketSize"], c.table["numVoxelBlocks"])


def test_the_cases_reach_what_they_name():
    kinds = {n.split("_")[0] for n in bc.names()}
    assert {"shape", "rounds", "chunks", "calls", "far"} <= kinds
    assert [bc.case(f"rounds_{n}").views[0].conditions["kept"] for n in bc.ROUNDS] == [256, 257, 512, 513]     # 1, 2, 2, 3 rounds of 256
    assert [bc.case(f"chunks_{n}").views[0].conditions["kept"] for n in bc.CHUNKS] == [1024, 1025, 2049]      # 1, 2, 3 chunks of 1024
    shapes = [(bc.case(n).W, bc.case(n).H) for n in bc.names() if n.startswith("shape")]
    assert shapes == bc.SHAPES and any(w % 16 and w > 16 for w, _ in shapes) and any(w < 8 and h < 8 for w, h in shapes)


# ---- 4. the oracle against the rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.names())
def test_oracle_equals_the_rule(oracle, name):
    c = bc.case(name)
    ot = oracle.OracleTable(oracle.default_params(**c.table), c.W, c.H, 1)
    ot.set_raycast_intrinsics(c.fx, c.fy, c.cx, c.cy)
    assert ot.insert_blocks(c.keys) == len(c.keys)
    for i, v in enumerate(c.views):
        front, back, _ = c.expected(i)
        of, ob = ot.render_blocks(v.pose, v.t_min, v.t_max)
        assert br.same_bits(of, front), (name, i, int((of.view(np.uint32) != front.view(np.uint32)).sum()))
        assert br.same_bits(ob, back), (name, i, int((ob.view(np.uint32) != back.view(np.uint32)).sum()))
    ot.close()
