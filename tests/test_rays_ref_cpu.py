"""tests/rays_ref.py (the rule of vh_cast_rays in numpy) pinned without a GPU: with the rays of pinhole_rays and the shared
plane it gives the bits of tests/raycast_ref.py on every crafted view of tests/raycast_cases.py; along each ray (no plane) it
gives facts computed by hand; every kind of refusal is refused."""
import numpy as np
import pytest

import raycast_cases as rc
import rays_ref
from raycast_ref import F

U = np.uint32


def case_rays(vh, case):
    return vh.pinhole_rays(case.pose, case.focal, case.focal, case.cx, case.cy, case.W, case.H, *case.t)


def case_plane(oracle, case):
    return np.asarray(oracle.invert4x4(case.pose), F).reshape(4, 4)[2]


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_shared_plane_gives_the_raycast_bits(vh, oracle, case):
    depth, normals, record = rc.reference(case, oracle)
    t, status, voxel, normal, rec = rays_ref.cast(case.model, rc.VS, case_rays(vh, case), case_plane(oracle, case))
    found = record["found"].reshape(-1)
    assert np.array_equal(status, found.astype(np.int32)) and np.array_equal(rec["found"], found)
    assert np.isnan(t[~found]).all() and (depth.reshape(-1)[~found] == 0).all()          # its 0 for a miss <-> NaN
    assert rc.same_image(t[found], depth.reshape(-1)[found], case.nan)
    assert np.array_equal(voxel[found], record["hit"].reshape(-1, 3)[found]) and (voxel[~found] == 0).all()
    assert np.array_equal(rec["first"][found], record["first"].reshape(-1, 3)[found])
    assert np.array_equal(rec["start"], record["start"].reshape(-1, 3))
    for k in ("events", "candidates", "tie_xy", "tie_xz", "tie_yz", "tie_xyz", "inactive", "starts_in_allocated", "ends_in_allocated",
              "tmax_equals_event"):
        assert np.array_equal(rec[k], record[k].reshape(-1)), k
    T = case.pose
    with np.errstate(all="ignore"):
        cam = np.stack([(T[0, i] * normal[:, 0] + T[1, i] * normal[:, 1]) + T[2, i] * normal[:, 2] for i in range(3)], 1)
    assert rc.same_image(cam, normals.reshape(-1, 4)[:, :3], case.nan)
    assert (normal[~found] == 0).all() and found.mean() > 0.02


# ---- along each ray: facts computed by hand ----
def ramp_wall():
    """Blocks (-1..0, -1..0, 2): sdf = (19.5 - z) * 0.25 at voxel z = 16..23, weight 1: the zero level at z = 19.5 voxels, that is,
    between the centres of voxels 19 (sdf +0.125) and 20 (-0.125), in the world at 19.5 * VS."""
    i = np.arange(512)
    sdf = ((19.5 - (16 + (i >> 6))) * 0.25).astype(F)
    return {(kx, ky, 2): (sdf.copy(), np.ones(512, F)) for kx in (-1, 0) for ky in (-1, 0)}


def test_axis_aligned_rays_hit_the_ramp_at_the_analytic_t():
    """A ray along +z from the centre of voxel (x, y, z0): the centre of voxel z projects to t = (z - z0) * VS / |D| exactly (all
    powers of two), the pair is voxels 19 -> 20 with sdf +-1/8, so t = t19 + ((t20 - t19) * 1/8) / (1/4) = (19.5 - z0) * VS / |D|."""
    model = ramp_wall()
    vs = F(rc.VS)
    rays = []
    for x, y, z0, d in ((0, 0, 4, 1.0), (-3, 5, 0, 1.0), (2, -7, -12, 1.0), (0, 0, 4, 2.0), (-3, 5, 0, 0.5), (5, 5, 8, 4.0)):
        rays.append([x * vs, y * vs, z0 * vs, 0.0, 0.0, 0.0, d, 1.0])
    rays = np.array(rays, F)
    t, status, voxel, normal, rec = rays_ref.cast(model, rc.VS, rays)
    want = np.array([(19.5 - r[2] / vs) * vs / r[6] for r in rays], F)
    assert (status == 1).all() and np.array_equal(t.view(U), want.view(U))
    assert np.array_equal(voxel, [[round(float(r[0] / vs)), round(float(r[1] / vs)), 20] for r in rays])
    assert np.array_equal(normal, np.tile(np.array([0, 0, -1], F), (len(rays), 1)))       # towards positive sdf
    assert (rec["inactive"] == 2).all()
    # scaling D by 2 halves t exactly
    twice = rays.copy()
    twice[:, 4:7] *= 2
    t2 = rays_ref.cast(model, rc.VS, twice)[0]
    assert np.array_equal((t2 * F(2)).view(U), t.view(U))
    # the same along -z from behind: the ray meets negative sdf first and never sees + -> -
    back = rays[:3].copy()
    back[:, 2], back[:, 6] = 40 * vs, -1.0
    assert (rays_ref.cast(model, rc.VS, back)[1] == 0).all()
    # ending before the pair's second voxel: crossings are taken while t < t_max, the crossing into voxel 20 (grid coordinate 20, from 4.5) is at 15.5 * VS for ray 0
    short = rays[:1].copy()
    for t_max, st in ((F(15.5) * vs, 0), (np.nextafter(F(15.5) * vs, F(1)), 1)):
        short[0, 7] = t_max
        assert rays_ref.cast(model, rc.VS, short)[1][0] == st


def test_oblique_rays_scale_with_the_direction(vh, oracle):
    """Scaling D by a power of two scales every crossing time and every sample parameter exactly: t halves, the walk is the same."""
    case = rc.BY_NAME["noise general"]
    rays = case_rays(vh, case)[::7]
    t, status, voxel, normal, rec = rays_ref.cast(case.model, rc.VS, rays)
    half = rays.copy()
    half[:, 4:7] *= 2
    half[:, 3] /= 2
    half[:, 7] /= 2
    t2, status2, voxel2, normal2, rec2 = rays_ref.cast(case.model, rc.VS, half)
    assert (status == 1).mean() > 0.25 and np.array_equal(status, status2) and np.array_equal(voxel, voxel2)
    assert rays_ref.same_bits(t2 * F(2), t) and np.array_equal(normal.view(U), normal2.view(U))
    assert np.array_equal(rec["events"], rec2["events"])
    # and the parameter along the ray is not the camera depth: it differs from the shared-plane answer off the optical axis
    depth = rays_ref.cast(case.model, rc.VS, rays, case_plane(oracle, case))[0]
    hit = status == 1
    assert (np.abs(t[hit] - depth[hit]) > 1e-3).mean() > 0.5


# ---- refusals ----
def refusals():
    """(name, ray) for every kind of refusal, each one change away from a good ray."""
    vs = rc.VS
    good = np.array([0.1, 0.2, 0.05, 0.0, 0.3, -0.2, 1.0, 0.5], F)
    out = []
    for i in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            r = good.copy()
            r[i] = bad
            out.append((f"float {i} = {bad}", r))
    for t0, t1 in ((0.5, 0.5), (0.5, 0.25), (0.0, -1.0)):
        r = good.copy()
        r[3], r[7] = t0, t1
        out.append((f"t_max {t1} <= t_min {t0}", r))
    r = good.copy()
    r[4:7] = 0
    out.append(("D = 0", r))
    r = good.copy()
    r[4:7] = (1e-30, 0, 0)
    out.append(("dd underflows to 0", r))
    r = good.copy()
    r[7] = 2.0 * (1 << 22) * vs                  # twice the step bound along z
    out.append(("step bound", r))
    r = good.copy()
    r[4:7] *= 1 << 23                            # the same through the direction's length
    out.append(("step bound by |D|", r))
    r = good.copy()
    r[2] = 2.0 * (1 << 23) * vs                  # |G| twice the reach bound
    out.append(("reach by the origin", r))
    r = good.copy()
    r[3], r[7] = -2.0 * (1 << 23) * vs, -2.0 * (1 << 23) * vs + 1.0      # a short ray far along itself
    out.append(("reach by t", r))
    return good, out


def test_every_kind_of_refusal():
    good, bad = refusals()
    model = ramp_wall()
    rays = np.stack([good] + [r for _, r in bad] + [good])
    t, status, voxel, normal, rec = rays_ref.cast(model, rc.VS, rays)
    assert status[0] != -1 and status[-1] != -1
    for (name, _), st in zip(bad, status[1:-1]):
        assert st == -1, name
    refused = status == -1
    assert np.isnan(t[refused]).all() and (voxel[refused] == 0).all() and (normal[refused] == 0).all() and rec["refused"][refused].all()
    # half the bounds are accepted (tests stay a factor of two away from either)
    ok = good.copy()
    ok[7] = 0.5 * (1 << 22) * rc.VS / 1.2
    assert rays_ref.accepted(ok[None], rc.VS)[0][0]
    ok = good.copy()
    ok[2] = 0.5 * (1 << 23) * rc.VS
    assert rays_ref.accepted(ok[None], rc.VS)[0][0]
