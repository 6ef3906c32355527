"""The TSDF update on crafted depth and stored voxels (tests/tsdf_cases.py), every kernel site that inlines tsdf_apply
(vh_integrate.hip) against the rule of tests/deintegrate_ref.py applied to the downloaded pre-state: every voxel of the volume,
every bit, no tolerance; where a case holds non-finite values the NaNs must stand at the same voxels.  The allocated keys must be
the oracle's.  tests/test_tsdf_cases_cpu.py pins the rule to the oracle on the same cases and checks that the inputs reach the
edges they aim at.

Forms: the step-level calls (also with two workgroups striding over the list), the four-kernel and the fused frame with either
walk, pipelined batches of three frames, the frame from the sensor image, two shards with float and uint16 packets (stepwise
and batched), and the three removal calls."""
import numpy as np
import pytest

import tsdf_cases as TC
from test_gpu_deintegrate import dev, snapshot
from test_tsdf_cases_cpu import (MULTI, MULTI_SIZE, assert_same_voxels, expected_by_rule, key_set, load_oracle, oracle_multi,
                                 oracle_run)
from voxelhashing_demo_amd import dist as vdist

pytestmark = pytest.mark.gpu
FORMS = {"four-kernel-reference-walk": (0, 3), "four-kernel-indexed-walk": (0, 4), "fused-reference-walk": (1, 3),
         "fused-indexed-walk": (1, 4)}
PLACED = 0


def set_up(t, c):
    t.set_projection(c.proj)
    t.set_option("depth_truncation", c.flags & 1)
    t.set_option("weight_sample", (c.flags >> 1) & 1)


def loaded_table(vh, c, form=None, **options):
    gt = vh.SDFHashtable(c.params(vh), c.W, c.H, c.sem)
    set_up(gt, c)
    if form is not None:
        gt.set_option("fused_frame", FORMS[form][0])
        gt.set_option("flatten_variant", FORMS[form][1])
    for k, v in options.items():
        gt.set_option(k, v)
    st = gt.stream_in(c.chunk())
    assert st["placed"] == len(c.blocks) and (st["status"] == PLACED).all()
    return gt


def check_loaded(c, pre, mine=lambda key: True):
    """The downloaded pre-state holds the crafted voxels, bit for bit (NaNs as NaNs)."""
    tab = pre["table"]
    where = {tuple(e["pos"].tolist()): int(e["ptr"]) for e in tab[tab["ptr"] != -1]}
    assert set(where) == {k for k in c.blocks if mine(k)}
    for k, p in where.items():
        for f, want in zip(("sdf", "weight"), c.blocks[k]):
            got = pre["vox"][f][p:p + 512]
            nan = np.isnan(want)
            assert np.array_equal(nan, np.isnan(got)) and np.array_equal(want.view(np.uint32)[~nan], got.view(np.uint32)[~nan]), (k, f)


def check(oracle, c, gt, pre, steps, keysets, what, sign=+1):
    """The volume after the call(s) against the rule from the downloaded pre-state; the allocated keys against the oracle's."""
    post = snapshot(gt)
    assert gt.counters()["heap_exhausted"] == 0
    assert key_set(post["table"][post["table"]["ptr"] != -1]) == keysets[-1], what
    want, updated = expected_by_rule(oracle, c, gt.params, pre["vox"], post["table"], steps, keysets, sign)
    assert updated > 500
    assert_same_voxels(want, post["vox"], c, what)
    print(f"{c.name} [{what}]: {updated} voxel updates compared over the whole volume of {len(post['vox'])} voxels")
    return post


SINGLE = [n for f in "abcdef" for n in TC.names(f)]
WHOLE = [n for f in "abcf" for n in TC.names(f)]


# ---- 1. the step-level calls: integrate_kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 2], ids=["default-grid", "two-workgroups"])
@pytest.mark.parametrize("name", SINGLE)
def test_step_level_update(oracle, vh, torch_cuda, name, grid):
    """set_pose / reset_mutexes / alloc_blocks / flatten / integrate_depth_map; the update is given a plane of its own where
    the case has one (family d: non-finite depth, which allocation never sees)."""
    c = TC.case(oracle, name)
    runs = oracle_run(oracle, c)
    gt = loaded_table(vh, c, **({"integrate_grid": grid} if grid else {}))
    for k, f in enumerate(c.frames):
        pre = snapshot(gt)
        if k == 0:
            check_loaded(c, pre)
        gt.set_pose(f.pose)
        gt.reset_mutexes()
        gt.alloc_blocks(dev(torch_cuda, f.verts))
        n = gt.flatten()
        assert n == len(runs[k]["entries"])
        gt.integrate_depth_map(dev(torch_cuda, f.depth_verts()))
        check(oracle, c, gt, pre, [[f]], [runs[k]["keys"]], f"step-level, frame {k}")
    gt.close()


# ---- 2. whole frames: integrate_kernel again, the fused frame's walk and its integrate_block on new entries -----------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", WHOLE)
def test_whole_frames(oracle, vh, torch_cuda, name, form):
    c = TC.case(oracle, name)
    runs = oracle_run(oracle, c)
    gt = loaded_table(vh, c, form)
    for k, f in enumerate(c.frames):
        pre = snapshot(gt)
        gt.integrate(f.pose, dev(torch_cuda, f.verts))
        check(oracle, c, gt, pre, [[f]], [runs[k]["keys"]], f"{form}, frame {k}")
    gt.close()


# ---- 3. pipelined batches: the two sites that read the frame before's parameters, depth and list -----------------------------
@pytest.mark.parametrize("walk", [3, 4], ids=["reference-walk", "indexed-walk"])
@pytest.mark.parametrize("name", TC.names("f"))
def test_pipelined_batch_of_three(oracle, vh, torch_cuda, name, walk):
    """Three frames with different poses and planes in one vh_integrate_batch: a launch that took a neighbouring frame's pose,
    plane or list would change a voxel."""
    c = TC.case(oracle, name)
    runs = oracle_run(oracle, c)
    gt = loaded_table(vh, c, fused_frame=1, flatten_variant=walk, pipeline=1)
    gt.set_profiling(True)
    pre = snapshot(gt)
    bufs = [dev(torch_cuda, f.verts) for f in c.frames]
    gt.integrate_batch([f.pose for f in c.frames], bufs)
    check(oracle, c, gt, pre, [[f] for f in c.frames], [r["keys"] for r in runs], f"pipelined batch, walk {walk}")
    assert gt.kernel_times()["frame_pipelined_ms"] > 0
    gt.close()


# ---- 4. the frame from the sensor image: DepthSensor in the frame kernels ----------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS) + ["pipelined"])
@pytest.mark.parametrize("name", TC.names("e"))
def test_frames_from_the_sensor_image(oracle, vh, torch_cuda, name, form):
    c = TC.case(oracle, name)
    runs = oracle_run(oracle, c)
    f = c.frames[0]
    d16, kinv = f.sensor
    if form == "pipelined":
        gt = loaded_table(vh, c, fused_frame=1, flatten_variant=3, pipeline=1)
    else:
        gt = loaded_table(vh, c, form)
    pre = snapshot(gt)
    if form == "pipelined":
        gt.integrate_depth_batch([f.pose], [dev(torch_cuda, d16)], kinv)
    else:
        gt.integrate_depth(f.pose, dev(torch_cuda, d16), kinv)
    check(oracle, c, gt, pre, [[f]], [runs[0]["keys"]], f"integrate_depth, {form}")
    gt.close()


# ---- 5. two shards: integrate_block_multi, float and uint16 packets ----------------------------------------------------------
@pytest.mark.parametrize("calls", ["batched", "stepwise"])
@pytest.mark.parametrize("name,batch", MULTI)
def test_two_shards_two_cameras(oracle, vh, torch_cuda, name, batch, calls):
    """Two cameras per frame, one or two frames per exchange, on two bucket-range shards: each shard against the rule applied
    camera by camera, in camera order, over each camera's own visible set of the shard's table."""
    torch = torch_cuda
    t, keysets = oracle_multi(oracle, name, batch)
    W, H = MULTI_SIZE
    sensor = t.frames[0].sensor is not None
    world = 2
    plan = vdist.ShardPlan(t.table["numBuckets"], world)
    shards = [vdist.HipShard(t.params(vh), W, H, t.sem, plan, r, W * H, batch=batch, batched_calls=(calls == "batched"),
                             sensor_k_inv=t.frames[0].sensor[1] if sensor else None) for r in range(world)]
    pres = []
    for r, sh in enumerate(shards):
        set_up(sh.table, t)
        sh.table.stream_in(t.chunk())
        pres.append(snapshot(sh.table))
    lo_hi = [plan.bucket_range(r) for r in range(world)]
    owner = lambda key, r: lo_hi[r][0] <= oracle.hash_block(*key, t.table["numBuckets"]) < lo_hi[r][1]
    for r in range(world):
        check_loaded(t, pres[r], lambda key: owner(key, r))
    cam = lambda r: [t.steps[b][r] for b in range(batch)]                  # camera r's frames
    vdist.loopback_step(shards, [[f.pose for f in cam(r)] for r in range(world)],
                        [[dev(torch, f.verts) for f in cam(r)] for r in range(world)],
                        [[dev(torch, f.sensor[0]) for f in cam(r)] for r in range(world)] if sensor else None)
    total = 0
    for r, sh in enumerate(shards):
        mine = [{k for k in ks if owner(k, r)} for ks in keysets]
        assert len(mine[-1]) > 8
        check(oracle, t, sh.table, pres[r], t.steps, mine, f"shard {r}, {calls}, {'uint16' if sensor else 'float'} packets")
        assert sh.table.counters()["bin_overflow"] == 0
        total += len(mine[-1])
    assert total == len(keysets[-1])
    for sh in shards:
        sh.table.close()


# ---- 6. the removal: deintegrate_kernel ---------------------------------------------------------------------------------------
R_PLANE = [n for n in TC.names("r") if not n.startswith("r-e")]
R_SENSOR = [n for n in TC.names("r") if n.startswith("r-e")]


@pytest.mark.parametrize("grid", [0, 2], ids=["default-grid", "two-workgroups"])
@pytest.mark.parametrize("name", R_PLANE)
def test_deintegrate_from_a_plane(oracle, vh, torch_cuda, name, grid):
    """vh_deintegrate on stored weights that leave the floor and its neighbours, on special depths and on non-finite values."""
    c = TC.case(oracle, name)
    f = c.frames[0]
    gt = loaded_table(vh, c, **({"integrate_grid": grid} if grid else {}))
    pre = snapshot(gt)
    check_loaded(c, pre)
    gt.deintegrate(f.pose, dev(torch_cuda, f.depth_verts()))
    post = check(oracle, c, gt, pre, [[f]], [set(c.blocks)], "deintegrate", sign=-1)
    assert np.array_equal(post["table"], pre["table"])
    gt.close()


@pytest.mark.parametrize("name", R_SENSOR)
def test_deintegrate_and_reintegrate_from_the_sensor_image(oracle, vh, torch_cuda, name):
    c = TC.case(oracle, name)
    f = c.frames[0]
    d16, kinv = f.sensor
    gt = loaded_table(vh, c)
    pre = snapshot(gt)
    gt.deintegrate_depth(f.pose, dev(torch_cuda, d16), kinv)
    mid = check(oracle, c, gt, pre, [[f]], [set(c.blocks)], "deintegrate_depth", sign=-1)
    assert np.array_equal(mid["table"], pre["table"])
    gt.close()
    # out at the old pose, in again at another: the removal by the rule from the pre-state, the update by the rule from that
    new = TC.Frame(TC.SECOND_CAMERA, f.verts, sensor=f.sensor)
    ot = load_oracle(oracle, c)
    ot.integrate(new.pose, new.verts)
    keys = key_set(ot.allocated())
    assert ot.last_stats["heap_exhausted"] == 0 and len(keys) > len(c.blocks)
    ot.close()
    gt = loaded_table(vh, c)
    pre = snapshot(gt)
    gt.reintegrate_depth(f.pose, new.pose, dev(torch_cuda, d16), kinv)
    post = snapshot(gt)
    assert key_set(post["table"][post["table"]["ptr"] != -1]) == keys
    out, n_out = expected_by_rule(oracle, c, gt.params, pre["vox"], pre["table"], [[f]], [set(c.blocks)], -1)
    want, n_in = expected_by_rule(oracle, c, gt.params, out, post["table"], [[new]], [keys], +1)
    assert n_out > 500 and n_in > 500
    assert_same_voxels(want, post["vox"], c, "reintegrate_depth")
    print(f"{c.name} [reintegrate_depth]: {n_out} removals and {n_in} updates compared over the whole volume")
    gt.close()
