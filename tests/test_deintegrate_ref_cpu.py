"""The de-integration rule without a GPU: tests/deintegrate_ref.py against the oracle's TSDF update (sign = +1, bit for bit),
and the rule's own cases (sign = -1): round trip to empty, the three branches of a partial removal, the weight cap."""
import os
import re

import numpy as np
import pytest

import deintegrate_cases as DC
import deintegrate_ref as R
from voxelhashing_demo_amd import synth

F = np.float32
I4 = np.eye(4, dtype=np.float32)
POSE = synth.yaw_pose(5.0, (0.1, 0.0, 0.05))              # the golden scenes' non-identity pose
TSDF_KW = dict(truncation=0.04, truncScale=0.02, integrationWeightSample=10)      # golden "tsdf_variants_pin_f3"

GOLDEN_CASES = [(sem, "I", flags, "inside") for sem in (0, 1) for flags in (0, 1, 2, 3)] + \
               [(0, "P", 0, "inside"), (1, "P", 3, "inside"), (1, "I", 0, "outside"), (1, "I", 3, "outside")]


def bits(v):
    return np.ascontiguousarray(v).view(np.uint32)


@pytest.mark.parametrize("sem,pose_name,flags,scene", GOLDEN_CASES)
def test_plus_one_is_the_oracles_update(oracle, sem, pose_name, flags, scene):
    """The numpy form of the sample computation (on the device it is stated once, tsdf_apply in vh_integrate.hip, for the
    update and for the removal) and combineVoxel against OracleTable.integrate_depth_map on the golden scenes
    (640x480 spheres, 2^17 buckets): first into an empty model, then onto stored weights."""
    pose = I4 if pose_name == "I" else POSE
    verts = synth.sphere_inside_scene() if scene == "inside" else synth.sphere_outside_scene()
    kw = dict(numBuckets=1 << 17, numVoxelBlocks=4096)
    if flags:
        kw.update(TSDF_KW)
    ot = oracle.OracleTable(oracle.default_params(**kw), 640, 480, sem)
    proj = DC.projection(sem, 640, 480)
    ot.set_projection(proj)
    ot.set_integrate_flags(flags)
    inv = oracle.invert4x4(pose)
    for frame in range(2):
        ot.set_pose(pose)
        ot.reset_mutexes()
        ot.alloc_blocks(verts)
        n = ot.flatten()
        assert n > 20                                                      # (the outside sphere: 44 blocks)
        entries, pre = ot.compact().copy(), ot.sdf_blocks().copy()
        vis = R.visible_entries(ot.hash_table(), ot.params, sem, proj, pose, inv, 640, 480)
        assert np.array_equal(ot.hash_table()[vis], entries)              # the block set: table order, like the oracle's flatten
        ot.integrate_depth_map(verts)
        want, stats = R.apply_frame(pre, entries, ot.params, sem, proj, inv, pose, verts[..., 2], flags, +1)
        assert stats["updated"] > 1000
        assert np.array_equal(bits(want), bits(ot.sdf_blocks())), (frame, stats)
    assert (entries["pos"] < 0).any()                                     # blocks at negative coordinates were among them
    ot.close()


def test_sensor_arithmetic_is_preprocess(oracle):
    """depth_source = (uint16 image, K^-1) gives the camera z of vh_preprocess's vertex map, bit for bit."""
    _, d16, verts = DC.frames(oracle)[1]
    sy, sx = np.mgrid[0:DC.H, 0:DC.W]
    z = R._depth_at((d16, DC.k_inv()), sx, sy)
    assert np.array_equal(bits(z), bits(verts[..., 2]))
    assert (d16 == 0).any() and (z > 0).any()


def model_of(oracle, sem, flags, which, **kw):
    ot = DC.oracle_table(oracle, sem, flags, **kw)
    for i in which:
        pose, _, verts = DC.frames(oracle)[i]
        ot.integrate(pose, verts)
    return ot


def remove(oracle, ot, sem, flags, i, sensor=True):
    """The rule applied to the oracle's model: (voxels after, stats, entries) for frame i taken out."""
    pose, d16, verts = DC.frames(oracle)[i]
    proj, inv = DC.projection(sem), oracle.invert4x4(pose)
    tab = ot.hash_table()
    entries = tab[R.visible_entries(tab, ot.params, sem, proj, pose, inv, DC.W, DC.H)]
    src = (d16, DC.k_inv()) if sensor else verts[..., 2]
    out, stats = R.apply_frame(ot.sdf_blocks().copy(), entries, ot.params, sem, proj, inv, pose, src, flags, -1)
    return out, stats, entries


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("flags", [0, 3])
def test_round_trip_to_empty(oracle, sem, flags):
    ot = model_of(oracle, sem, flags, [1])
    assert (ot.sdf_blocks()["weight"] > 0).sum() > 1000
    out, stats, entries = remove(oracle, ot, sem, flags, 1)
    assert len(entries) == len(ot.allocated())                            # the frame's own view sees every block it allocated
    assert stats["reset"] == (ot.sdf_blocks()["weight"] > 0).sum() and stats["partial"] == 0
    assert not bits(out).any()                                            # every voxel {+0, +0}
    ot.close()


@pytest.mark.parametrize("sem", [0, 1])
def test_middle_frame_out_of_three(oracle, sem):
    """Frames 0, 1, 2 in, frame 1 out: the scene reaches all three branches, and where the removal is the algebraic
    inverse -- blocks that existed when frame 1 went in -- it gives the model of frames 0 and 2 up to fp32 rounding."""
    ot = model_of(oracle, sem, 0, [0, 1, 2])
    out, stats, entries = remove(oracle, ot, sem, 0, 1)
    assert stats["untouched"] > 0 and stats["reset"] > 0 and stats["partial"] > 0, stats
    assert 2 < len(entries) <= 512
    # sensor image and vertex map are the same frame
    out_v, stats_v, _ = remove(oracle, ot, sem, 0, 1, sensor=False)
    assert stats_v == stats and np.array_equal(bits(out), bits(out_v))
    # against the model that never saw frame 1.  Error bound: weights are 0.1 .. 0.3, |sdf| <= truncation = 1, every operation
    # is within 2^-24 relative, and the subtraction amplifies by at most ow / nw <= 3: well below 1e-5.
    early = model_of(oracle, sem, 0, [0, 1])
    known = {tuple(p) for p in early.allocated()["pos"].tolist()}
    two = model_of(oracle, sem, 0, [0, 2])
    two_by_pos = {tuple(e["pos"].tolist()): int(e["ptr"]) for e in two.allocated()}
    compared = 0
    for e in entries:
        key = tuple(e["pos"].tolist())
        if key not in known or key not in two_by_pos:
            continue
        a = out[int(e["ptr"]):int(e["ptr"]) + 512]
        b = two.sdf_blocks()[two_by_pos[key]:two_by_pos[key] + 512]
        assert np.array_equal(a["weight"] > 0, b["weight"] > 0), key
        assert np.abs(a["weight"] - b["weight"]).max() <= 1e-5 and np.abs(a["sdf"] - b["sdf"]).max() <= 1e-5, key
        compared += 1
    assert compared > 2
    for t in (ot, early, two):
        t.close()


def test_weight_cap_follows_the_rule_not_the_inverse(oracle):
    """integrationWeightMax = 0.25: three frames saturate a voxel at 0.25 (not 0.3); taking one out leaves 0.25 - 0.1 and
    ((os * 0.25) - (s * 0.1)) / that -- the rule -- not the two-frame model's 0.2."""
    sem = 1
    ot = model_of(oracle, sem, 0, [1, 1, 1], integrationWeightMax=0.25)
    pre = ot.sdf_blocks().copy()
    capped = np.nonzero(pre["weight"] == F(0.25))[0]
    assert len(capped) > 1000
    out, stats, entries = remove(oracle, ot, sem, 0, 1)
    assert stats["partial"] >= len(capped)             # (a block that lost its bucket in frame 1 came later and holds less)
    nw = F(0.25) - F(0.1)
    assert np.array_equal(bits(out["weight"][capped]), np.full(len(capped), bits(np.array([nw]))[0]))
    assert nw != F(0.1) + F(0.1)
    # the sdf by the rule, voxel by voxel in scalar float32, with the sample recomputed from the frame
    pose, d16, _ = DC.frames(oracle)[1]
    ok, s, cw = R.frame_samples(entries, ot.params, sem, DC.projection(sem), oracle.invert4x4(pose), (d16, DC.k_inv()), 0)
    at = entries["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
    checked = 0
    for b, v in zip(*np.nonzero(ok & (pre["weight"][at] == F(0.25)))):
        os_, sv = pre["sdf"][at[b, v]], s[b, v]
        want = F(F(F(os_ * F(0.25)) - F(sv * F(0.1))) / nw)
        assert bits(np.array([want]))[0] == bits(out["sdf"][at[b, v]:at[b, v] + 1])[0]
        checked += 1
    assert checked == len(capped)
    ot.close()


def test_bindings_name_the_three_calls():
    from test_abi import declared_functions
    from voxelhashing_demo_amd import _lib
    names = sorted(_lib.SIGNATURES)
    for n in ("vh_deintegrate", "vh_deintegrate_depth", "vh_reintegrate_depth"):
        assert n in names
    assert names == declared_functions()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voxelhash.h")).read()
    assert re.search(r"taking a frame back out", header)
