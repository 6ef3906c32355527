"""vh_deintegrate / vh_deintegrate_depth / vh_reintegrate_depth on the GPU against tests/deintegrate_ref.py applied to the
downloaded pre-state: hash table, heap, heap counter, compact set, `occupied` and every voxel bit.  64x48 images of the
synthetic room, at most 512 blocks (tests/deintegrate_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC
import deintegrate_ref as R
from voxelhashing_demo_amd import dist as vdist
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint32
W, H = DC.W, DC.H


def table(vh, sem, flags=0, width=W, height=H, **kw):
    p = dict(DC.KW)
    p.update(kw)
    gt = vh.SDFHashtable(vh.default_params(**p), width, height, sem)
    gt.set_projection(DC.projection(sem, width, height))
    gt.set_option("depth_truncation", flags & 1)
    gt.set_option("weight_sample", (flags >> 1) & 1)
    return gt


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(torch, gt, frames, which, sensor=True):
    for i in which:
        pose, d16, verts = frames[i]
        if sensor:
            gt.integrate_depth(pose, dev(torch, d16), DC.k_inv(gt.width, gt.height))
        else:
            gt.integrate(pose, dev(torch, verts))


def snapshot(gt):
    gt.synchronize()
    c = gt.counters()
    return dict(table=gt.hash_table(), heap=gt.heap(), vox=gt.sdf_blocks(), heap_counter=c["heap_counter"], occupied=c["occupied"],
                compact=gt.compact(), epoch=c["epoch"])


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


def expected(oracle, gt, pre, sem, flags, pose, src):
    """(voxels, entries, stats) by the rule from the downloaded pre-state."""
    proj, inv = DC.projection(sem, gt.width, gt.height), oracle.invert4x4(pose)
    idx = R.visible_entries(pre["table"], gt.params, sem, proj, pose, inv, gt.width, gt.height)
    entries = pre["table"][idx]
    vox, stats = R.apply_frame(pre["vox"], entries, gt.params, sem, proj, inv, pose, src, flags, -1)
    return vox, entries, stats, idx


def check_against_rule(gt, pre, want_vox, entries):
    post = snapshot(gt)
    assert np.array_equal(post["table"], pre["table"])                    # the hash table, the heap and its counter: unchanged
    assert np.array_equal(post["heap"], pre["heap"])
    assert post["heap_counter"] == pre["heap_counter"] and post["epoch"] == pre["epoch"]
    assert post["occupied"] == len(entries)                               # the compact list: the blocks the call touched
    got = post["compact"]
    assert keys_of(got) == keys_of(entries) and sorted(got["ptr"].tolist()) == sorted(entries["ptr"].tolist())
    assert np.array_equal(post["vox"].view(U), want_vox.view(U))          # every voxel bit
    return post


def by_key(snap):
    tab = snap["table"]
    return {tuple(e["pos"].tolist()): snap["vox"][int(e["ptr"]):int(e["ptr"]) + 512].view(U) for e in tab[tab["ptr"] != -1]}


def same_model(a, b):
    """Two contexts hold the same model (block ids may differ: the heap is handed out by atomics)."""
    assert np.array_equal(a["table"]["pos"], b["table"]["pos"]) and np.array_equal(a["table"]["offset"], b["table"]["offset"])
    assert np.array_equal(a["table"]["ptr"] != -1, b["table"]["ptr"] != -1)
    assert a["heap_counter"] == b["heap_counter"] and a["occupied"] == b["occupied"]
    assert keys_of(a["compact"]) == keys_of(b["compact"])
    ka, kb = by_key(a), by_key(b)
    assert ka.keys() == kb.keys()
    for k in ka:
        assert np.array_equal(ka[k], kb[k]), k


# ---- 1. the three-frame case -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("sensor", [False, True], ids=["vertex-map", "uint16"])
def test_middle_frame_out_of_three(oracle, vh, torch_cuda, sem, sensor):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, verts = frames[1]
    gt = table(vh, sem)
    fuse(torch, gt, frames, [0, 1, 2], sensor)
    pre = snapshot(gt)
    assert gt.counters()["heap_exhausted"] == 0
    want, entries, stats, _ = expected(oracle, gt, pre, sem, 0, pose, (d16, DC.k_inv()) if sensor else verts[..., 2])
    assert stats["untouched"] > 0 and stats["reset"] > 0 and stats["partial"] > 0, stats
    print(f"sem {sem}: {len(entries)} blocks, {stats}")
    if sensor:
        gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    else:
        gt.deintegrate(pose, dev(torch, verts))
    post = check_against_rule(gt, pre, want, entries)
    if sensor:                                                            # == vh_preprocess + vh_deintegrate
        twin = table(vh, sem)
        fuse(torch, twin, frames, [0, 1, 2], True)
        pos = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        nrm = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        vh.preprocess(dev(torch, d16), DC.k_inv(), pos, nrm)
        torch.cuda.synchronize()
        twin.deintegrate(pose, pos)
        same_model(post, snapshot(twin))
        twin.close()
    gt.close()


# ---- 2. the options of the update ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_flag_combinations(oracle, vh, torch_cuda, flags):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    gt = table(vh, 1, flags, truncation=0.3, truncScale=0.05)
    fuse(torch, gt, frames, [0, 1, 2])
    pre = snapshot(gt)
    want, entries, stats, _ = expected(oracle, gt, pre, 1, flags, pose, (d16, DC.k_inv()))
    assert stats["reset"] > 0 and stats["partial"] > 0, stats
    gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    check_against_rule(gt, pre, want, entries)
    gt.close()


# ---- 3. the stride loop and the empty list ------------------------------------------------------------------------------
def test_two_workgroups_stride_over_the_list_and_an_empty_view(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    gt = table(vh, 1)
    gt.set_option("integrate_grid", 2)
    fuse(torch, gt, frames, [0, 1, 2])
    pre = snapshot(gt)
    # a pose that sees no block: nothing changes, occupied == 0
    want, entries, stats, _ = expected(oracle, gt, pre, 1, 0, DC.NOWHERE, (d16, DC.k_inv()))
    assert len(entries) == 0
    gt.deintegrate_depth(DC.NOWHERE, dev(torch, d16), DC.k_inv())
    post = check_against_rule(gt, pre, want, entries)
    assert post["occupied"] == 0 and np.array_equal(post["vox"].view(U), pre["vox"].view(U))
    # two workgroups over many blocks
    want, entries, stats, _ = expected(oracle, gt, post, 1, 0, pose, (d16, DC.k_inv()))
    assert len(entries) > 2 and stats["reset"] + stats["partial"] > 0
    gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    check_against_rule(gt, post, want, entries)
    gt.close()


# ---- 4. the overflow list ------------------------------------------------------------------------------------------------
def test_chained_entries_are_processed(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    nb, bs = 32, 2                                                        # (few buckets: that is what makes chains)
    gt = table(vh, 1, numBuckets=nb, bucketSize=bs, attachedLinkedListSize=8)
    gt.set_option("overflow_list", 1)
    for _ in range(6):                                                    # (a bucket takes one new entry per frame)
        fuse(torch, gt, frames, [0, 1, 2])
    pre = snapshot(gt)
    want, entries, stats, idx = expected(oracle, gt, pre, 1, 0, pose, (d16, DC.k_inv()))
    chained = [int(i) for i in idx if oracle.hash_block(*[int(c) for c in pre["table"][i]["pos"]], nb) != i // bs]
    assert chained, "no chained entry is visible: the scene does not test the overflow list"
    assert stats["reset"] + stats["partial"] > 0
    gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    check_against_rule(gt, pre, want, entries)
    gt.close()


# ---- 5. a pending pipelined frame ----------------------------------------------------------------------------------------
def test_pending_pipelined_frame_is_launched_first(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    snaps = []
    for pipeline in (1, 0):
        gt = table(vh, 1)
        gt.set_option("pipeline", pipeline)
        gt.set_profiling(True)
        fuse(torch, gt, frames, [0, 1, 2])                                # pipelined: frame 2's commit + update are still pending
        gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
        snaps.append(snapshot(gt))
        assert (gt.kernel_times()["frame_pipelined_ms"] > 0) == bool(pipeline)
        gt.close()
    same_model(*snaps)
    # and the unpipelined one is the rule's (frame 2 is in the model the frame came out of)
    assert (snaps[0]["vox"]["weight"] > 0).sum() > 1000


# ---- 6. shards -----------------------------------------------------------------------------------------------------------
def test_two_shards_remove_from_their_own_blocks(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    world = 2
    params = vh.default_params(**DC.KW)
    plan = vdist.ShardPlan(DC.KW["numBuckets"], world)
    shards = [vdist.HipShard(params, W, H, 1, plan, r, W * H) for r in range(world)]
    full = table(vh, 1)
    for sh in shards:
        sh.table.set_projection(DC.projection(1))
    # two multi-camera frames: rank 0's camera sees frames 0 then 2, rank 1's camera frame 1 twice
    for a, b in ((0, 1), (2, 1)):
        cams = [frames[a], frames[b]]
        vdist.loopback_step(shards, [[c[0]] for c in cams], [[dev(torch, c[2])] for c in cams])
        vdist.reference_multi_camera_frame(full, [c[0] for c in cams], [dev(torch, c[2]) for c in cams])
    pre = snapshot(full)
    want, entries, stats, _ = expected(oracle, full, pre, 1, 0, pose, (d16, DC.k_inv()))
    assert stats["reset"] + stats["partial"] > 0
    full.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    post = check_against_rule(full, pre, want, entries)
    union, seen = {}, []
    for sh in shards:
        spre = snapshot(sh.table)
        swant, sentries, _, _ = expected(oracle, sh.table, spre, 1, 0, pose, (d16, DC.k_inv()))
        sh.table.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
        spost = check_against_rule(sh.table, spre, swant, sentries)
        assert len(sentries) > 0                                          # each shard has blocks of its own to remove from
        part = by_key(spost)
        assert not set(part) & set(union)
        union.update(part)
        seen += keys_of(sentries)
    whole = by_key(post)
    assert union.keys() == whole.keys() and sorted(seen) == keys_of(entries)
    for k in whole:
        assert np.array_equal(union[k], whole[k]), k
    for sh in shards:
        sh.table.close()
    full.close()


# ---- 7. in, out, collect -------------------------------------------------------------------------------------------------
def test_frame_in_frame_out_collect_leaves_nothing(oracle, vh, torch_cuda):
    torch = torch_cuda
    pose, d16, _ = DC.frames(oracle)[1]
    gt = table(vh, 1)
    gt.integrate_depth(pose, dev(torch, d16), DC.k_inv())
    assert len(gt.allocated()) > 20 and gt.mesh_count() > 0
    gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    gt.synchronize()
    assert not gt.sdf_blocks().view(U).any()                              # every voxel {+0, +0}
    gt.garbage_collect(0.0)
    gt.synchronize()
    assert len(gt.allocated()) == 0
    assert gt.counters()["heap_counter"] == gt.params.numVoxelBlocks - 1
    assert gt.mesh_count() == 0
    gt.close()


# ---- 8. the composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (37, 29)], ids=["64x48", "37x29"])
def test_reintegrate_is_out_then_in(oracle, vh, torch_cuda, size):
    torch = torch_cuda
    w, h = size
    frames = DC.frames(oracle, w, h)
    old, d16, _ = frames[1]
    new = synth.yaw_pose(9.0, (0.12, 0.01, 0.04))                         # the "corrected" pose
    kinv = DC.k_inv(w, h)
    a, b = table(vh, 1, width=w, height=h), table(vh, 1, width=w, height=h)
    for gt in (a, b):
        fuse(torch, gt, frames, [0, 1, 2])
    pre = snapshot(b)
    want, entries, stats, _ = expected(oracle, b, pre, 1, 0, old, (d16, kinv))
    assert len(entries) > 2 and stats["reset"] + stats["partial"] > 0
    a.reintegrate_depth(old, new, dev(torch, d16), kinv)
    b.deintegrate_depth(old, dev(torch, d16), kinv)
    check_against_rule(b, pre, want, entries)                             # (the uint16 path at this image size, by the rule)
    b.integrate_depth(new, dev(torch, d16), kinv)
    same_model(snapshot(a), snapshot(b))
    a.close()
    b.close()


# ---- 9. arguments --------------------------------------------------------------------------------------------------------
def test_argument_checks_and_the_view_refusal(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, verts = frames[1]
    L = vh.load()
    gt = table(vh, 1)
    fuse(torch, gt, frames, [0, 1])
    pre = snapshot(gt)
    p16 = np.ascontiguousarray(pose, np.float32).reshape(16)
    pp = p16.ctypes.data_as(C.POINTER(C.c_float))
    k = DC.k_inv().reshape(9).copy()
    kp = k.ctypes.data_as(C.POINTER(C.c_float))
    dd, dv = dev(torch, d16), dev(torch, verts)
    h = gt._h
    INVALID = 1
    assert L.vh_deintegrate(None, pp, dv.data_ptr()) == INVALID
    assert L.vh_deintegrate(h, None, dv.data_ptr()) == INVALID
    assert L.vh_deintegrate(h, pp, None) == INVALID
    assert L.vh_deintegrate_depth(None, pp, dd.data_ptr(), kp) == INVALID
    assert L.vh_deintegrate_depth(h, None, dd.data_ptr(), kp) == INVALID
    assert L.vh_deintegrate_depth(h, pp, None, kp) == INVALID
    assert L.vh_deintegrate_depth(h, pp, dd.data_ptr(), None) == INVALID
    assert L.vh_reintegrate_depth(None, pp, pp, dd.data_ptr(), kp) == INVALID
    assert L.vh_reintegrate_depth(h, None, pp, dd.data_ptr(), kp) == INVALID
    assert L.vh_reintegrate_depth(h, pp, None, dd.data_ptr(), kp) == INVALID
    assert L.vh_reintegrate_depth(h, pp, pp, None, kp) == INVALID
    assert L.vh_reintegrate_depth(h, pp, pp, dd.data_ptr(), None) == INVALID
    # the Python layer: dtype, size, device
    with pytest.raises(ValueError):
        gt.deintegrate_depth(pose, dd.to(torch.int32), k)
    with pytest.raises(ValueError):
        gt.deintegrate_depth(pose, dd[:-1], k)
    with pytest.raises(ValueError):
        gt.deintegrate_depth(pose, torch.from_numpy(d16), k)
    with pytest.raises(ValueError):
        gt.reintegrate_depth(pose, pose, dd[:-1], k)
    with pytest.raises(ValueError):
        gt.deintegrate(pose, dv.double())
    with pytest.raises(ValueError):
        gt.deintegrate(pose, dv[:-1])
    post = snapshot(gt)
    for name in ("table", "heap", "vox", "compact"):
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    assert post["heap_counter"] == pre["heap_counter"] and post["occupied"] == pre["occupied"]
    # a context that holds an imported view
    ot = DC.oracle_table(oracle, 1)
    for i in (0, 1):
        ot.integrate(frames[i][0], frames[i][2])
    records, n = ot.export_view(pose, 512)
    assert 0 < n <= 512
    view = vdist.HipViewTable(vh.default_params(**DC.KW), W, H, 1, 1, 512)
    view.recv[:n] = torch.from_numpy(records).cuda()
    torch.cuda.synchronize()
    view.table.import_view(view.recv, n)
    vpre = snapshot(view.table)
    assert (vpre["table"]["ptr"] != -1).sum() == n
    assert L.vh_deintegrate(view.table._h, pp, dv.data_ptr()) == INVALID
    assert L.vh_deintegrate_depth(view.table._h, pp, dd.data_ptr(), kp) == INVALID
    assert L.vh_reintegrate_depth(view.table._h, pp, pp, dd.data_ptr(), kp) == INVALID
    with pytest.raises(vh.VoxelHashError):
        view.table.deintegrate_depth(pose, dd, k)
    vpost = snapshot(view.table)
    assert np.array_equal(vpost["table"], vpre["table"]) and vpost["epoch"] == vpre["epoch"]
    torch.cuda.synchronize()
    assert np.array_equal(view.recv[:n].cpu().numpy(), records)
    view.table.close()
    ot.close()
    gt.close()


# ---- 10. C++ -------------------------------------------------------------------------------------------------------------
def test_cpp_program_takes_its_frame_back_out(vh, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "deintegrate_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "deintegrate_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    synth.sphere_inside_scene().tofile(tmp_path / "verts.bin")
    out = subprocess.run([str(exe), str(tmp_path / "verts.bin")], check=True, capture_output=True, text=True).stdout
    got = dict(kv.split("=") for kv in out.split())
    assert int(got["fused"]) > 1000 and int(got["left"]) == 0 and int(got["blocks"]) == 0, out
