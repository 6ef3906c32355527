"""Frame-to-frame ICP on the GPU (vh_icp_*, vh_depth_to_maps, computeCorrespondences) against the
oracle, and the frame-to-model loop (raycast -> maps -> Align -> integrate) against ground truth.
Per-pixel results (maps, residuals, pairing, count) are bit-exact; the 27 sums are fp32 tree sums
on the GPU and double sums in the oracle, compared at 1e-4 of the largest entry."""
import ctypes as C

import numpy as np
import pytest

from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
SUM_RTOL = 1e-4


def frame_pair(i, j, n):
    prims = synth.room_primitives()
    poses = synth.camera_loop(n)
    K = synth.K_matrix(W, H)
    v0 = synth.render_room_verts(poses[i], W, H, prims).numpy()
    v1 = synth.render_room_verts(poses[j], W, H, prims).numpy()
    T0, T1 = (np.asarray(poses[k], np.float64).reshape(4, 4) for k in (i, j))
    return K, v0, v1, np.linalg.inv(T0) @ T1


def maps_on_both(oracle, torch, depth, kinv):
    from voxelhashing_demo_amd import tracking
    po, no = oracle.depth_to_maps(depth, kinv)
    d = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    pg, ng = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 4), device="cuda")
    tracking.depth_to_maps(d, kinv, pg, ng)
    torch.cuda.synchronize()
    assert np.array_equal(pg.cpu().numpy().view(np.uint32), po.view(np.uint32))
    assert np.array_equal(ng.cpu().numpy().view(np.uint32), no.view(np.uint32))
    return po, no, pg, ng


def expected_layout(w, h, blocks=None):
    """vh_icp_create's rule: (round grid, one-launch grid, pixels per lane in registers -- 0: read again every round)."""
    npix = w * h
    most = -(-npix // 256)
    g = min(most, 512 if npix > 6 * 256 * 256 else 256) if blocks is None else max(1, min(most, blocks))
    slots = -(-npix // (g * 256))
    return (g, g, slots if slots <= 6 else 0)


def icp_layout(trk):
    """(round grid, one-launch grid, pixels per lane; -1: the chain of rounds) of a CameraTracking (vh_debug_icp_layout)."""
    from voxelhashing_demo_amd import _lib as L
    out = (C.c_int32 * 3)()
    L.check(L.load().vh_debug_icp_layout(trk._h, out), "vh_debug_icp_layout")
    return tuple(out)


def close_sums(got, want):
    JTJ, JTr, err, cnt = got
    oJTJ, oJTr, oerr, ocnt = want
    assert cnt == ocnt
    assert np.abs(JTJ - oJTJ).max() <= SUM_RTOL * np.abs(oJTJ).max()
    assert np.abs(JTr - oJTr).max() <= SUM_RTOL * max(np.abs(oJTr).max(), 1e-3 * np.sqrt(np.abs(oJTJ).max() * ocnt) * 0.08)
    assert abs(err - oerr) <= SUM_RTOL * max(abs(oerr), 0.08 * np.sqrt(ocnt))
    assert np.array_equal(JTJ, JTJ.T)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_linear_system_matches_oracle(oracle, vh, torch_cuda, flags):
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    K, v0, v1, true = frame_pair(100, 101, 250)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    p0, n0, g0, gn0 = maps_on_both(oracle, torch, v0[..., 2], kinv)
    p1, _, g1, _ = maps_on_both(oracle, torch, v1[..., 2], kinv)
    trk = tracking.CameraTracking(W, H, K, flags=flags)
    rng = np.random.default_rng(3)
    for delta in (np.eye(4), true, oracle.se3_exp(rng.normal(size=6) * 0.01) @ true):
        d32 = delta.astype(np.float32)
        want = oracle.icp_build_system(p1, p0, n0, d32, K, 0.08, flags)
        got = trk.build_system(g1, g0, gn0, d32)
        close_sums(got, want)
        assert want[3] > 50000
        # run to run reproducible (fixed summation order)
        again = trk.build_system(g1, g0, gn0, d32)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and got[2] == again[2]


def test_correspondence_maps_are_bit_exact(oracle, vh, torch_cuda):
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    K, v0, v1, true = frame_pair(100, 102, 250)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    p0, n0, g0, gn0 = maps_on_both(oracle, torch, v0[..., 2], kinv)
    p1, _, g1, _ = maps_on_both(oracle, torch, v1[..., 2], kinv)
    trk = tracking.CameraTracking(W, H, K)
    c = torch.full((H, W, 4), 7.0, device="cuda")
    cn = torch.full((H, W, 4), 7.0, device="cuda")
    r = torch.full((H, W), 7.0, device="cuda")
    for flags in (0, 3):
        trk.flags = flags
        oc, ocn, orr, oerr, ocnt = oracle.icp_correspondences(p1, p0, n0, np.eye(4), K, 0.08, flags)
        got = trk.correspondences(g1, g0, gn0, np.eye(4), c, cn, r)
        torch.cuda.synchronize()
        assert np.array_equal(c.cpu().numpy().view(np.uint32), oc.view(np.uint32))
        assert np.array_equal(cn.cpu().numpy().view(np.uint32), ocn.view(np.uint32))
        assert np.array_equal(r.cpu().numpy().view(np.uint32), orr.view(np.uint32))
        assert got[3] == ocnt and abs(got[2] - oerr) <= SUM_RTOL * max(abs(oerr), 0.08 * np.sqrt(ocnt))


def test_drop_in_compute_correspondences(oracle, vh, torch_cuda):
    """computeCorrespondences with SetCameraIntrinsic, the reference's calling sequence (CameraTracking.cpp:16,49)."""
    torch = torch_cuda
    Wd, Hd = 640, 480
    prims = synth.room_primitives()
    poses = synth.camera_loop(250)
    K = synth.K_matrix(Wd, Hd)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    z0 = synth.render_room_verts(poses[100], Wd, Hd, prims).numpy()[..., 2]
    z1 = synth.render_room_verts(poses[101], Wd, Hd, prims).numpy()[..., 2]
    p0, n0 = oracle.depth_to_maps(z0, kinv)
    p1, _ = oracle.depth_to_maps(z1, kinv)
    L = vh.load()
    kf, kif = np.ascontiguousarray(K, np.float32).reshape(9), kinv.reshape(9).copy()
    assert L.SetCameraIntrinsic(kf.ctypes.data_as(C.POINTER(C.c_float)), kif.ctypes.data_as(C.POINTER(C.c_float)))
    g = [torch.from_numpy(a).cuda() for a in (p1, p0, n0)]
    c, cn = torch.empty((Hd, Wd, 4), device="cuda"), torch.empty((Hd, Wd, 4), device="cuda")
    r = torch.empty((Hd, Wd), device="cuda")
    eye = np.eye(4, dtype=np.float32).reshape(16)
    err = L.computeCorrespondences(g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), c.data_ptr(), cn.data_ptr(),
                                   r.data_ptr(), eye.ctypes.data_as(C.POINTER(C.c_float)), Wd, Hd)
    oc, ocn, orr, oerr, ocnt = oracle.icp_correspondences(p1, p0, n0, np.eye(4), K, 0.08, 0)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), orr.view(np.uint32))
    assert np.array_equal(c.cpu().numpy().view(np.uint32), oc.view(np.uint32))
    assert abs(err - oerr) <= SUM_RTOL * max(abs(oerr), 0.08 * np.sqrt(ocnt))


def test_partial_sums_hand_off_while_another_kernel_holds_the_chip(oracle, vh, torch_cuda):
    """The last workgroup of an ICP round adds what all the others stored (records written as agent-scope stores, drained, then
    a ticket -- no cache write-back, vh_icp.hip).  Here a long kernel of another stream holds most workgroup
    slots of every XCD while 60 rounds run, so that a round's workgroups trickle in on whatever compute unit comes free: every
    round must still give the sums it gives on an idle chip, bit for bit (fixed summation order), and the oracle's within the
    fp32 tolerance."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    K, v0, v1, true = frame_pair(100, 101, 250)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    p0, n0, g0, gn0 = maps_on_both(oracle, torch, v0[..., 2], kinv)
    p1, _, g1, _ = maps_on_both(oracle, torch, v1[..., 2], kinv)
    trk = tracking.CameraTracking(W, H, K, flags=0)
    d32 = true.astype(np.float32)
    idle = trk.build_system(g1, g0, gn0, d32)
    close_sums(idle, oracle.icp_build_system(p1, p0, n0, d32, K, 0.08, 0))
    gt = vh.SDFHashtable(vh.default_params(numBuckets=1 << 10, numVoxelBlocks=64), 64, 48, 1)      # (only for vh_debug_occupy)
    hog, L = torch.cuda.Stream(), vh.load()
    for burst in range(6):
        assert L.vh_debug_occupy(gt._h, hog.cuda_stream, 1792, 20000) == 0                          # 20 ms of a nearly full chip
        for _ in range(10):
            got = trk.build_system(g1, g0, gn0, d32)
            assert np.array_equal(got[0], idle[0]) and np.array_equal(got[1], idle[1]) and got[2] == idle[2] and got[3] == idle[3]
    torch.cuda.synchronize()
    gt.close()


@pytest.mark.parametrize("flags", [0, 3])
def test_align_matches_oracle_and_truth(oracle, vh, torch_cuda, flags):
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    K, v0, v1, true = frame_pair(100, 101, 250)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    p0, n0, g0, gn0 = maps_on_both(oracle, torch, v0[..., 2], kinv)
    p1, _, g1, _ = maps_on_both(oracle, torch, v1[..., 2], kinv)
    want, oit, _, ocnt = oracle.icp_align(p1, p0, n0, K, 0.08, 20, flags)
    trk = tracking.CameraTracking(W, H, K, flags=flags)
    got = trk.Align(g1, g0, gn0)
    assert trk.iterations == oit == 20
    assert np.abs(got - want).max() < 2e-4             # fp32 sums feed 20 solves; pairings can flip by an ulp
    assert np.abs(got[:3, 3] - true[:3, 3]).max() < 5e-4 and np.abs(got[:3, :3] - true[:3, :3]).max() < 5e-4
    assert abs(trk.last[3] - ocnt) <= 0.001 * ocnt
    assert trk.getTransform() is trk.delta


def test_single_plane_is_singular_on_the_gpu_too(oracle, vh, torch_cuda):
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    K, v0, v1, true = frame_pair(10, 12, 500)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    _, _, g0, gn0 = maps_on_both(oracle, torch, v0[..., 2], kinv)
    _, _, g1, _ = maps_on_both(oracle, torch, v1[..., 2], kinv)
    trk = tracking.CameraTracking(W, H, K, flags=3)
    JTJ, JTr, err, cnt = trk.build_system(g1, g0, gn0, np.eye(4))
    ok, est = tracking.icp_solve(JTJ, JTr, np.zeros(6))
    ev = np.linalg.eigvalsh(JTJ)
    assert cnt > 50000 and ev[2] < 1e-5 * ev[5]
    # fp32 rounding may leave J^T J barely positive definite; then the step must at least be finite
    assert (not ok) or np.isfinite(est).all()


@pytest.mark.parametrize("normals", ["tsdf", "depth"])
def test_frame_to_model_tracking_loop(oracle, vh, torch_cuda, normals):
    """KinectFusion loop on the synthetic room: the pose of frame k comes from aligning its vertex
    map to a raycast of the model built from frames < k; only frame 0 uses the true pose.  The target's
    normals are the model's own (TSDF gradient at the hits, written by the raycast pass: vh_raycast_normals) or
    those calculateNormals derives from the raycast depth (CameraTrackingUtils.cu:75-113)."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    prims = synth.room_primitives()
    gt = synth.camera_loop(500)[200:212]
    K = synth.K_matrix(W, H)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    table = vh.SDFHashtable(vh.default_params(numBuckets=1 << 16, numVoxelBlocks=1 << 14), W, H, 1)
    trk = tracking.CameraTracking(W, H, K, flags=tracking.ICP_ABS_DISTANCE | tracking.ICP_NEED_TARGET)
    depth = torch.zeros((H, W), device="cuda")
    tp, tn, tn2 = (torch.empty((H, W, 4), device="cuda") for _ in range(3))
    pose = np.asarray(gt[0], np.float64).reshape(4, 4)
    verts = [synth.render_room_verts(p, W, H, prims).cuda() for p in gt]
    table.integrate(pose.astype(np.float32), verts[0])
    errs = []
    for k in range(1, len(gt)):
        if normals == "tsdf":
            table.raycast_normals(pose.astype(np.float32), depth, tn)
            tracking.depth_to_maps(depth, kinv, tp, tn2)
        else:
            table.raycast(pose.astype(np.float32), depth)
            tracking.depth_to_maps(depth, kinv, tp, tn)
        delta = trk.Align(verts[k], tp, tn).astype(np.float64)
        assert trk.last[3] > 0.5 * W * H
        pose = pose @ delta
        table.integrate(pose.astype(np.float32), verts[k])
        truth = np.asarray(gt[k], np.float64).reshape(4, 4)
        errs.append(np.abs(pose[:3, 3] - truth[:3, 3]).max())
    moved = np.abs(np.asarray(gt[-1], np.float64).reshape(4, 4)[:3, 3] - np.asarray(gt[0], np.float64).reshape(4, 4)[:3, 3]).max()
    assert moved > 0.1
    print(f"tracking drift with {normals} normals: {1e3 * max(errs):.2f} mm over {1e3 * moved:.0f} mm")
    assert max(errs) < 0.012, errs         # drift about 1 cm over 14 cm of travel (round 2's fixed-step march: 9.9 mm)


def test_fusion_loop_poses_equal_the_oracle_loop(oracle, vh, torch_cuda):
    """The closed loop bench.py times (tracking.FusionLoop; frame order of Application.cpp:73-90): per uint16 sensor frame
    vh_preprocess -> vh_icp_align against the model's raycast maps -> vh_integrate_depth at the tracked pose -> vh_raycast_maps.
    The same loop on the oracle (preprocess, icp_align, integrate, raycast + depth_to_maps) must track the same poses: the
    per-pixel work is bit-equal, the ICP sums are fp32 tree sums here and double sums there (2e-4 per Align, test above), and
    both stay on the synthetic truth."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    prims = synth.room_primitives()
    gt_poses = synth.camera_loop(500)[200:207]
    K = synth.K_matrix(W, H)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    d16 = [np.round(synth.render_room_verts(p, W, H, prims).numpy()[..., 2] * 5000.0).clip(0, 65535).astype(np.uint16) for p in gt_poses]
    kw = dict(numBuckets=1 << 16, numVoxelBlocks=1 << 14)
    flags = tracking.ICP_ABS_DISTANCE | tracking.ICP_NEED_TARGET
    # the library
    table = vh.SDFHashtable(vh.default_params(**kw), W, H, 1)
    loop = tracking.FusionLoop(table, K, kinv, flags=flags)
    dev = [torch.from_numpy(d).cuda() for d in d16]
    got = [loop.start(dev[0], gt_poses[0]).copy()]
    for k in range(1, len(gt_poses)):
        got.append(loop.step(dev[k]).copy())
        assert loop.trk.last[3] > 0.5 * W * H
    # the oracle, the same order of operations
    ot = oracle.OracleTable(oracle.default_params(**kw), W, H, 1)
    pose = np.asarray(gt_poses[0], np.float64).reshape(4, 4).copy()
    want = [pose.copy()]
    ot.integrate(pose.astype(np.float32), oracle.preprocess(d16[0], kinv)[0])
    mv, mn = oracle.depth_to_maps(ot.raycast(pose.astype(np.float32)), kinv)
    for k in range(1, len(gt_poses)):
        iv = oracle.preprocess(d16[k], kinv)[0]
        delta = oracle.icp_align(iv, mv, mn, K, 0.08, 20, flags)[0]
        pose = pose @ np.asarray(delta, np.float64).reshape(4, 4)
        want.append(pose.copy())
        ot.integrate(pose.astype(np.float32), iv)
        mv, mn = oracle.depth_to_maps(ot.raycast(pose.astype(np.float32)), kinv)
    for k in range(len(gt_poses)):
        truth = np.asarray(gt_poses[k], np.float64).reshape(4, 4)
        assert np.abs(got[k] - want[k]).max() < 1.5e-3, (k, np.abs(got[k] - want[k]).max())
        assert np.abs(got[k][:3, 3] - truth[:3, 3]).max() < 0.012 and np.abs(want[k][:3, 3] - truth[:3, 3]).max() < 0.012
    assert np.abs(np.asarray(gt_poses[-1])[:3, 3] - np.asarray(gt_poses[0])[:3, 3]).max() > 0.05
    loop.close()
    table.close()
    ot.close()


def test_raycast_maps_is_raycast_plus_depth_to_maps(oracle, vh, torch_cuda):
    torch = torch_cuda
    prims = synth.room_primitives()
    poses = synth.camera_loop(60)
    kw = dict(numBuckets=1 << 14, numVoxelBlocks=8192)
    ot = oracle.OracleTable(oracle.default_params(**kw), W, H, 1)
    gt = vh.SDFHashtable(vh.default_params(**kw), W, H, 1)
    for p in poses[:9:3]:
        v = synth.render_room_verts(p, W, H, prims).numpy()
        ot.integrate(p, v)
        gt.integrate(p, torch.from_numpy(v).cuda())
    depth = torch.empty((H, W), device="cuda")
    vm, nm = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 4), device="cuda")
    gt.raycast_maps(poses[6], depth, vm, nm)
    torch.cuda.synchronize()
    ref = ot.raycast(poses[6])
    fx, fy, cx, cy = (np.float32(a) for a in synth.intrinsics(W, H))
    one = np.float32(1.0)
    kinv = np.array([one / fx, 0, -cx / fx, 0, one / fy, -cy / fy, 0, 0, 1], np.float32)
    ov, on = oracle.depth_to_maps(ref, kinv)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(vm.cpu().numpy().view(np.uint32), ov.view(np.uint32))
    assert np.array_equal(nm.cpu().numpy().view(np.uint32), on.view(np.uint32))
    assert (on[..., :3] != 0).any(axis=-1).sum() > 10000


# (pixels per lane of the one-launch kernel: 1 on 192 workgroups, 2, 3, 4, 5, 6 in registers on 256 -- one instantiation each
# -- then 4 on 512 (800x560), and at 1280x960 the instantiation that reads the points again every round, on 512; the layout is
# asserted, so that the one-launch side is not the chain's fall-back.  Other sizes and grids: tests/test_gpu_icp_edges.py)
@pytest.mark.parametrize("size", [(256, 192), (320, 240), (480, 360), (512, 480), (640, 480), (800, 480), (800, 560), (1280, 960)])
def test_one_launch_align_equals_the_chain_of_rounds(vh, torch_cuda, size, monkeypatch):
    """vh_icp_align runs all rounds in ONE launch (icp_align_kernel: input points in registers, the estimate handed from
    round to round through memory, a grid-wide wait per round); VH_ICP_PERSISTENT=0 at vh_icp_create keeps the chain of
    one-launch rounds.  Same partition of the pixels, same order of additions, same solve: the transform, the last
    system and the round count are bit-equal -- for a full Align, for one cut short by max_iters, and for the two stop
    conditions (summed residual exactly 0, CameraTracking.cpp:52; singular system)."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    w, h = size
    prims, poses, K = synth.room_primitives(), synth.camera_loop(250), synth.K_matrix(w, h)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    v = {i: synth.render_room_verts(poses[i], w, h, prims, device="cuda") for i in (10, 12, 100, 101)}
    maps = {}
    for i in (10, 100):
        tp, tn = torch.empty_like(v[i]), torch.empty_like(v[i])
        tracking.depth_to_maps(v[i][..., 2].contiguous(), kinv, tp, tn)
        maps[i] = (tp, tn)
    nothing = torch.zeros_like(v[100])
    results = {}
    for form in ("one_launch", "chain"):
        if form == "chain":
            monkeypatch.setenv("VH_ICP_PERSISTENT", "0")
        out = []
        for flags in (0, 3):
            for iters in (20, 7, 1):
                trk = tracking.CameraTracking(w, h, K, flags=flags, max_iters=iters)
                assert icp_layout(trk) == (expected_layout(w, h) if form == "one_launch" else expected_layout(w, h)[:2] + (-1,))
                d = trk.Align(v[101], *maps[100]).copy()                          # a real step of the camera
                out.append((d, trk.last, trk.iterations))
                d = trk.Align(v[101], maps[100][0], nothing).copy()               # a target without normals: residual 0, stop
                out.append((d, trk.last, trk.iterations))
                assert trk.iterations == 0 and np.array_equal(d, np.eye(4, dtype=np.float32))
                d = trk.Align(v[12], *maps[10]).copy()                            # one flat wall: singular (or barely not)
                out.append((d, trk.last, trk.iterations))
                trk.close()
        results[form] = out
    assert results["one_launch"][0][2] == 20 and results["one_launch"][0][1][3] > 0.5 * w * h
    for a, b in zip(results["one_launch"], results["chain"]):
        assert a[2] == b[2]
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[1], b[1]))


def test_one_launch_align_gives_up_instead_of_hanging(vh, torch_cuda, monkeypatch):
    """The one-launch Align waits on its own grid; every wait is bounded.  With a limit of ONE poll (VH_ICP_SPIN_LIMIT at
    vh_icp_create) the workgroups give up before workgroup 0 can have solved: the call returns VH_ERR_TIMEOUT, leaves the
    caller's transform alone, and the next call on a workspace with the normal limit works -- nothing left over from the
    abandoned one gets in its way (the sequence numbers only grow)."""
    from voxelhashing_demo_amd import _lib as L
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    prims, poses, K = synth.room_primitives(), synth.camera_loop(250), synth.K_matrix(W, H)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    v0 = synth.render_room_verts(poses[100], W, H, prims, device="cuda")
    v1 = synth.render_room_verts(poses[101], W, H, prims, device="cuda")
    tp, tn = torch.empty_like(v0), torch.empty_like(v0)
    tracking.depth_to_maps(v0[..., 2].contiguous(), kinv, tp, tn)
    good = tracking.CameraTracking(W, H, K, flags=3)
    want = good.Align(v1, tp, tn).copy()
    monkeypatch.setenv("VH_ICP_SPIN_LIMIT", "1")
    hasty = tracking.CameraTracking(W, H, K, flags=3)
    monkeypatch.delenv("VH_ICP_SPIN_LIMIT")
    for _ in range(3):
        before = hasty.delta.copy()
        with pytest.raises(L.VoxelHashError, match="gave up"):
            hasty.Align(v1, tp, tn)
        assert np.array_equal(hasty.delta, before)
        assert np.array_equal(good.Align(v1, tp, tn), want)
    hasty.close()
    good.close()


def test_fusion_step_is_track_then_fuse(vh, torch_cuda):
    """vh_fusion_step (FusionLoop.step: one library call per frame) against the same five stages called one by one from
    Python (FusionLoop.track + FusionLoop.fuse): same poses (the 4x4 pose product is summed in a different order by numpy,
    so a pose may differ in its last float bit and the frames after it by that much), same model."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    prims = synth.room_primitives()
    gt_poses = synth.camera_loop(500)[200:206]
    K = synth.K_matrix(W, H)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    dev = [(synth.render_room_verts(p, W, H, prims, device="cuda")[..., 2] * 5000.0).round().clamp(0, 65535).to(torch.uint16)
           for p in gt_poses]
    kw = dict(numBuckets=1 << 16, numVoxelBlocks=1 << 14)
    flags = tracking.ICP_ABS_DISTANCE | tracking.ICP_NEED_TARGET
    tables = [vh.SDFHashtable(vh.default_params(**kw), W, H, 1) for _ in range(2)]
    loops = [tracking.FusionLoop(t, K, kinv, flags=flags) for t in tables]
    for lp in loops:
        lp.start(dev[0], gt_poses[0])
    for k in range(1, len(gt_poses)):
        a = loops[0].step(dev[k]).copy()
        loops[1].track(dev[k])
        loops[1].fuse(dev[k])
        b = loops[1].pose
        assert loops[0].trk.iterations == loops[1].trk.iterations == 20
        assert np.abs(a - b).max() < 1e-5, (k, np.abs(a - b).max())
        truth = np.asarray(gt_poses[k], np.float64).reshape(4, 4)
        assert np.abs(a[:3, 3] - truth[:3, 3]).max() < 0.012
    assert loops[0].frames == loops[1].frames == len(gt_poses)
    ca, cb = tables[0].counters(), tables[1].counters()
    assert abs(ca["allocated_total"] - cb["allocated_total"]) <= 0.01 * ca["allocated_total"]
    # a tracker on another stream than the table's is refused
    other = torch.cuda.Stream()
    stray = tracking.FusionLoop(tables[0], K, kinv, flags=flags)
    stray.trk._lib.vh_icp_set_stream(stray.trk._h, C.c_void_p(other.cuda_stream))
    stray.pose = loops[0].pose.copy()
    with pytest.raises(Exception, match="stream"):
        stray.step(dev[1])
    for lp in loops + [stray]:
        lp.close()
    for t in tables:
        t.close()


def test_one_launch_align_while_another_kernel_holds_the_chip(vh, torch_cuda):
    """The one-launch Align needs all its workgroups resident to finish a round.  Here a long kernel of another stream holds
    every workgroup slot of the chip (2 048 workgroups of 256 lanes) or most of them (1 792) for 20 ms at a time while Aligns
    are queued: their workgroups trickle in as slots come free, the ones that are there poll (bounded: ~1 s) -- every Align
    must end, without a time-out, with the transform it gives on an idle chip, bit for bit."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    w, h = 640, 480
    prims, poses, K = synth.room_primitives(), synth.camera_loop(250), synth.K_matrix(w, h)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    v0 = synth.render_room_verts(poses[100], w, h, prims, device="cuda")
    v1 = synth.render_room_verts(poses[101], w, h, prims, device="cuda")
    tp, tn = torch.empty_like(v0), torch.empty_like(v0)
    tracking.depth_to_maps(v0[..., 2].contiguous(), kinv, tp, tn)
    trk = tracking.CameraTracking(w, h, K, flags=3)
    idle = trk.Align(v1, tp, tn).copy()
    idle_last = trk.last
    gt = vh.SDFHashtable(vh.default_params(numBuckets=1 << 10, numVoxelBlocks=64), 64, 48, 1)      # (only for vh_debug_occupy)
    hog, L = torch.cuda.Stream(), vh.load()
    for burst, groups in enumerate((2048, 1792, 2048, 1792)):
        assert L.vh_debug_occupy(gt._h, hog.cuda_stream, groups, 20000) == 0
        for _ in range(12):
            got = trk.Align(v1, tp, tn)
            assert trk.iterations == 20
            assert np.array_equal(got.view(np.uint32), idle.view(np.uint32))
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(trk.last, idle_last))
    torch.cuda.synchronize()
    trk.close()
    gt.close()
