"""ICP at the image sizes and grids the benchmark never uses, against the double-precision oracle (oracle/vh_icp_oracle.c).

The one-launch Align (icp_align_kernel) is a grid-wide wait whose shape depends on the image: the grid (1..512 workgroups, or
VH_ICP_BLOCKS), the pixels a lane keeps in registers (1..6, one instantiation each) or the re-read loop (0), and how many of
workgroup 0's eight record parts have records at all (fewer than 8 workgroups, numBlocks % 256 in 1..7).  Each size here:
  - asserts the layout vh_icp_create chose (vh_debug_icp_layout), so that the one-launch path is what runs;
  - checks the maps ICP reads (vh_preprocess, vh_depth_to_maps) bit for bit;
  - checks the step API (vh_icp_build_system, vh_icp_correspondences) against the oracle;
  - checks ONE round of Align against the oracle: the sums within close_sums, the count exactly, and the transform against the
    oracle's solve of the GPU's own sums (a double solve of identical inputs: a float ulp or so);
  - checks the full Align bit-equal to the chain of rounds (VH_ICP_PERSISTENT=0) and, where the last system has at least 10^4
    pairs, within 2e-4 of the oracle's Align (below that, one pairing that flips by an ulp moves the result more than the fp32
    sums do: those sizes rest on the per-round check)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_icp import close_sums, expected_layout, icp_layout
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu

DIST = 0.08
FEW = [(1, 1), (16, 12), (32, 24), (40, 30), (42, 40), (257, 1), (1, 300)]        # fewer than 8 workgroups
ODD = [(64, 32), (80, 60), (161, 121), (321, 241), (641, 479)]                     # 8 workgroups; partial last slot
# one size per instantiation and grid: 1..6 pixels per lane on 256 workgroups (1 also on 1, and 256x256 is exactly 1),
# 4..6 on 512 (the grid rule gives 512 only above 6 pixels per lane of 256 workgroups), the re-read loop on 512
LAYOUTS = [(256, 256), (320, 240), (480, 360), (512, 480), (640, 480), (800, 480), (800, 560), (1024, 576), (1024, 768),
           (1025, 768), (1280, 960)]
SIZES = FEW + ODD + LAYOUTS
# VH_ICP_BLOCKS: numBlocks % 256 from 1 to 7 (and 8, 255: every part has records), re-read instantiation throughout
BLOCKS = [((320, 240), 1), ((320, 240), 7), ((320, 240), 9), ((1280, 960), 257), ((1280, 960), 263), ((1280, 960), 264),
          ((1280, 960), 511)]


def ident(size):
    return f"{size[0]}x{size[1]}"


def tracker(w, h, K, monkeypatch, flags=0, blocks=None, chain=False):
    """A CameraTracking whose layout is asserted: the one-launch Align on the grid of the rule, or the chain of rounds."""
    from voxelhashing_demo_amd import tracking
    with monkeypatch.context() as m:
        m.delenv("VH_ICP_PERSISTENT", raising=False)
        m.delenv("VH_ICP_BLOCKS", raising=False)
        if blocks is not None:
            m.setenv("VH_ICP_BLOCKS", str(blocks))
        if chain:
            m.setenv("VH_ICP_PERSISTENT", "0")
        trk = tracking.CameraTracking(w, h, K, flags=flags)
    want = expected_layout(w, h, blocks)
    got = icp_layout(trk)
    if chain:
        assert got == want[:2] + (-1,), (w, h, blocks, got)
    else:
        # -1 here would mean the occupancy query found the grid too large to be resident: the "one-launch" result would be
        # the chain's, and the bit-equality below would compare the chain with itself
        assert got == want, (w, h, blocks, got)
    return trk


class Scene:
    """The frame pair of test_gpu_icp (room, frames 100 -> 101) and the single-wall pair (10 -> 12) at one size, as oracle
    maps and as device maps (checked bit-equal on the way)."""

    def __init__(self, oracle, torch, w, h):
        from voxelhashing_demo_amd import tracking
        self.w, self.h = w, h
        prims, poses = synth.room_primitives(), synth.camera_loop(250)
        self.K = synth.K_matrix(w, h)
        self.kinv = np.linalg.inv(self.K.astype(np.float64)).astype(np.float32)
        self.o, self.g = {}, {}
        for i in (10, 12, 100, 101):
            z = np.ascontiguousarray(synth.render_room_verts(poses[i], w, h, prims).numpy()[..., 2])
            po, no = oracle.depth_to_maps(z, self.kinv)
            pg, ng = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w, 4), device="cuda")
            tracking.depth_to_maps(torch.from_numpy(z).cuda(), self.kinv, pg, ng)
            torch.cuda.synchronize()
            assert np.array_equal(pg.cpu().numpy().view(np.uint32), po.view(np.uint32))
            assert np.array_equal(ng.cpu().numpy().view(np.uint32), no.view(np.uint32))
            self.o[i], self.g[i] = (po, no), (pg, ng)
        T = {i: np.asarray(poses[i], np.float64).reshape(4, 4) for i in (100, 101)}
        self.true = np.linalg.inv(T[100]) @ T[101]
        # a fixed start off the truth by about 1 cm and 0.4 degrees
        self.start = oracle.se3_exp(np.array([0.008, -0.006, 0.01, 0.004, -0.007, 0.005])) @ self.true
        self.nothing = torch.zeros((h, w, 4), device="cuda")

    def step(self):        # (input, target, target normals) of the real step, oracle and device
        return (self.o[101][0], *self.o[100]), (self.g[101][0], *self.g[100])


_scenes = {}


def scene(oracle, torch, size):
    if size not in _scenes:
        if len(_scenes) > 4:
            _scenes.clear()
        _scenes[size] = Scene(oracle, torch, *size)
    return _scenes[size]


def check_one_round(oracle, trk, s, flags):
    """max_iters=1 from s.start: the system the GPU built at the start it used, and the step it took from that system."""
    from voxelhashing_demo_amd import tracking
    (op, ot, on), (gp, gt, gn) = s.step()
    start32 = s.start.astype(np.float32)
    T0 = tracking.se3_exp(tracking.se3_log(start32.astype(np.float64)))          # vh_icp_align's projection of the start
    S = T0.astype(np.float32)                                                     # the delta of round 0
    trk.flags, trk.max_iters = flags, 1
    got = trk.Align(gp, gt, gn, start=start32).copy()
    want = oracle.icp_build_system(op, ot, on, S, s.K, DIST, flags)
    close_sums(trk.last, want)
    JTJ, JTr, err, cnt = trk.last
    if err == 0.0:                                                                # stop before any solve
        assert trk.iterations == 0 and np.array_equal(got.view(np.uint32), S.view(np.uint32))
        return cnt
    ok, est = oracle.icp_solve(JTJ, JTr, oracle.se3_log(T0))
    ev = np.linalg.eigvalsh(JTJ)
    if ok and ev[0] > 1e-8 * ev[5]:
        # a well-posed system: LDL^T in one lane against Cholesky, series against closed-form SE3 maps, all in double
        assert trk.iterations == 1
        assert np.abs(got.astype(np.float64) - oracle.se3_exp(est)).max() <= 1e-6, np.abs(got - oracle.se3_exp(est)).max()
    elif trk.iterations == 0:                                                     # the device found it singular: start kept
        assert np.array_equal(got.view(np.uint32), S.view(np.uint32))
    else:                                                                         # rank-deficient, yet a pivot above 0
        assert np.isfinite(got).all()
    return cnt


def align_runs(trk, s, iters_list=(20, 7, 1), flags_list=(0, 3)):
    """Every Align of the sweep of test_gpu_icp.test_one_launch_align_equals_the_chain_of_rounds: (transform, last, rounds)."""
    out = []
    _, (gp, gt, gn) = s.step()
    for flags in flags_list:
        for iters in iters_list:
            trk.flags, trk.max_iters = flags, iters
            d = trk.Align(gp, gt, gn).copy()                                      # a real step of the camera
            out.append((d, trk.last, trk.iterations))
            d = trk.Align(gp, gt, s.nothing).copy()                               # a target without normals: residual 0, stop
            out.append((d, trk.last, trk.iterations))
            assert trk.iterations == 0 and np.array_equal(d, np.eye(4, dtype=np.float32))
            d = trk.Align(s.g[12][0], *s.g[10]).copy()                            # one flat wall: singular (or barely not)
            out.append((d, trk.last, trk.iterations))
    return out


def assert_bit_equal(runs_a, runs_b):
    assert len(runs_a) == len(runs_b)
    for a, b in zip(runs_a, runs_b):
        assert a[2] == b[2]
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[1], b[1]))


def check_against_oracle_align(oracle, s, runs, flags_list=(0, 3), per_flags=9):
    """The 20-round Align of each flags value (runs[k * per_flags]) against the oracle's, where it has 10^4 pairs or more."""
    (op, ot, on), _ = s.step()
    for k, flags in enumerate(flags_list):
        got, last, iters = runs[k * per_flags]
        if last[3] < 10000:
            continue
        want, oit, _, ocnt = oracle.icp_align(op, ot, on, s.K, DIST, 20, flags)
        assert iters == oit == 20
        assert np.abs(got - want).max() < 2e-4, (flags, np.abs(got - want).max())
        assert abs(last[3] - ocnt) <= 0.001 * ocnt


# ---- the maps ICP reads ----

INPUT_SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 11), (11, 2), (3, 3), (257, 1), (1, 300), (16, 12), (42, 40), (161, 121),
               (641, 479)]


@pytest.mark.parametrize("size", INPUT_SIZES, ids=ident)
def test_input_maps_are_bit_exact(oracle, vh, torch_cuda, size):
    """vh_preprocess (uint16, with holes and 65535) and vh_depth_to_maps (float metres, with holes) against the oracle: strips
    one pixel wide or high and 2 x N images have no interior, so every normal is zero."""
    from voxelhashing_demo_amd import tracking
    from voxelhashing_demo_amd.hashtable import preprocess
    torch = torch_cuda
    w, h = size
    K = synth.K_matrix(w, h)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    z = np.ascontiguousarray(synth.render_room_verts(synth.camera_loop(250)[100], w, h).numpy()[..., 2])
    rng = np.random.default_rng(w * 7919 + h)
    z[rng.random(z.shape) < 0.05] = 0.0
    z.reshape(-1)[(w * h) // 2] = 0.0
    d16 = np.round(z * 5000.0).clip(0, 65535).astype(np.uint16)
    d16[rng.random(d16.shape) < 0.03] = 65535
    d16.reshape(-1)[-1] = 65535
    opos, onrm = oracle.preprocess(d16, kinv)
    gpos, gnrm = torch.full((h, w, 4), 7.0, device="cuda"), torch.full((h, w, 4), 7.0, device="cuda")
    preprocess(torch.from_numpy(d16.view(np.int16)).cuda(), kinv, gpos, gnrm)      # (the same 16 bits)
    po, no = oracle.depth_to_maps(z, kinv)
    gp, gn = torch.full((h, w, 4), 7.0, device="cuda"), torch.full((h, w, 4), 7.0, device="cuda")
    tracking.depth_to_maps(torch.from_numpy(z).cuda(), kinv, gp, gn)
    torch.cuda.synchronize()
    assert np.array_equal(gpos.cpu().numpy().view(np.uint32), opos.view(np.uint32))
    assert np.array_equal(gnrm.cpu().numpy().view(np.uint32), onrm.view(np.uint32))
    assert np.array_equal(gp.cpu().numpy().view(np.uint32), po.view(np.uint32))
    assert np.array_equal(gn.cpu().numpy().view(np.uint32), no.view(np.uint32))
    if min(w, h) <= 2:
        assert not onrm.any() and not no.any()
    else:
        assert (d16 == 65535).any() and (d16 == 0).any()
    if w * h >= 100:
        assert (no[..., :3] != 0).any() or min(w, h) <= 2


# ---- the step API ----

@pytest.mark.parametrize("size", SIZES, ids=ident)
def test_step_api_matches_oracle(oracle, vh, torch_cuda, size, monkeypatch):
    """vh_icp_build_system and vh_icp_correspondences (icp_round_kernel on the round grid: its ticket and icp_sum_records) at the
    identity and at a start off the truth, flags 0 and 3."""
    torch = torch_cuda
    s = scene(oracle, torch, size)
    (op, ot, on), (gp, gt, gn) = s.step()
    w, h = size
    c, cn = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w, 4), device="cuda")
    r = torch.empty((h, w), device="cuda")
    trk = tracker(w, h, s.K, monkeypatch)
    for flags in (0, 3):
        trk.flags = flags
        for delta in (np.eye(4), s.start):
            d32 = delta.astype(np.float32)
            want = oracle.icp_build_system(op, ot, on, d32, s.K, DIST, flags)
            close_sums(trk.build_system(gp, gt, gn, d32), want)
            for t in (c, cn, r):
                t.fill_(7.0)
            oc, ocn, orr, oerr, ocnt = oracle.icp_correspondences(op, ot, on, d32, s.K, DIST, flags)
            got = trk.correspondences(gp, gt, gn, d32, c, cn, r)
            torch.cuda.synchronize()
            assert np.array_equal(c.cpu().numpy().view(np.uint32), oc.view(np.uint32))
            assert np.array_equal(cn.cpu().numpy().view(np.uint32), ocn.view(np.uint32))
            assert np.array_equal(r.cpu().numpy().view(np.uint32), orr.view(np.uint32))
            assert ocnt == want[3]
            close_sums(got, want)
    trk.close()


# ---- Align ----

@pytest.mark.parametrize("size", SIZES, ids=ident)
def test_one_round_of_align_matches_oracle(oracle, vh, torch_cuda, size, monkeypatch):
    """max_iters=1 from a start off the truth, one launch: the system of icp_align_kernel's record hand-off and workgroup 0's
    sum, and the transform of its one-lane solve."""
    s = scene(oracle, torch_cuda, size)
    trk = tracker(*size, s.K, monkeypatch)
    counts = [check_one_round(oracle, trk, s, flags) for flags in (0, 3)]
    # (a strip one pixel wide or high pairs nothing -- the reference keeps only targets at u > 0 and v > 0 -- so there the
    # round stops at a residual of 0: the hand-off and the stop of a grid of 1 or 2 workgroups)
    assert counts[0] > 0 or min(size) == 1
    trk.close()


@pytest.mark.parametrize("size", SIZES, ids=ident)
def test_align_one_launch_equals_chain_and_oracle(oracle, vh, torch_cuda, size, monkeypatch):
    """The full Align (20, 7 and 1 rounds; a real step, a target without normals, one flat wall) in one launch bit-equal to the
    chain of rounds, and the 20-round result against the oracle's Align where the system has 10^4 pairs or more."""
    s = scene(oracle, torch_cuda, size)
    runs = {}
    for chain in (False, True):
        trk = tracker(*size, s.K, monkeypatch, chain=chain)
        runs[chain] = align_runs(trk, s)
        trk.close()
    assert_bit_equal(runs[False], runs[True])
    check_against_oracle_align(oracle, s, runs[False])
    if size[0] * size[1] >= 300 * 200:
        assert runs[False][0][2] == 20 and runs[False][0][1][3] > 0.5 * size[0] * size[1]


@pytest.mark.parametrize("size,blocks", BLOCKS, ids=[f"{ident(sz)}-{b}" for sz, b in BLOCKS])
def test_align_on_icp_blocks_grids(oracle, vh, torch_cuda, size, blocks, monkeypatch):
    """VH_ICP_BLOCKS: grids whose last 256-record pass leaves some of workgroup 0's eight parts without a record (1, 7, 257, 263),
    and neighbours where none is left out (9, 264, 511).  One round against the oracle, the Align bit-equal to the chain on the
    same grid, and against the oracle's Align."""
    s = scene(oracle, torch_cuda, size)
    trk = tracker(*size, s.K, monkeypatch, blocks=blocks)
    for flags in (0, 3):
        check_one_round(oracle, trk, s, flags)
    runs = {False: align_runs(trk, s, iters_list=(20, 7))}
    trk.close()
    trk = tracker(*size, s.K, monkeypatch, blocks=blocks, chain=True)
    runs[True] = align_runs(trk, s, iters_list=(20, 7))
    trk.close()
    assert_bit_equal(runs[False], runs[True])
    check_against_oracle_align(oracle, s, runs[False], per_flags=6)
    assert runs[False][0][2] == 20


def test_align_arguments(oracle, vh, torch_cuda, monkeypatch):
    """max_iters: 0 returns the start projected onto SE3 with no round; 65536 is accepted, 65537 refused with the caller's
    transform untouched.  VH_ICP_STAMPS=1 (diagnostics) on a 200-round Align -- past the 64 rounds of stamps kept -- changes
    no bit of the result."""
    from voxelhashing_demo_amd import _lib as L
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    s = scene(oracle, torch, (16, 12))
    _, (gp, gt, gn) = s.step()
    trk = tracker(16, 12, s.K, monkeypatch, flags=3)
    start32 = s.start.astype(np.float32)
    trk.max_iters = 0
    got = trk.Align(gp, gt, gn, start=start32).copy()
    S = tracking.se3_exp(tracking.se3_log(start32.astype(np.float64))).astype(np.float32)
    assert trk.iterations == 0 and np.array_equal(got.view(np.uint32), S.view(np.uint32))
    assert not np.array_equal(got, start32) or np.array_equal(S, start32)
    trk.max_iters = 65536
    trk.Align(gp, gt, gn)
    assert 0 <= trk.iterations <= 65536 and np.isfinite(trk.delta).all()
    kept = trk.delta.copy()
    trk.max_iters = 65537
    with pytest.raises(L.VoxelHashError, match="max_iters"):
        trk.Align(gp, gt, gn)
    assert np.array_equal(trk.delta, kept)
    # the C call itself leaves the caller's matrix alone
    d = start32.reshape(16).copy()
    sys, it = L.IcpSystem(), C.c_int32(-5)
    rc = trk._lib.vh_icp_align(trk._h, C.c_void_p(gp.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(gn.data_ptr()),
                               trk.K.ctypes.data_as(C.POINTER(C.c_float)), DIST, 65537, 3,
                               d.ctypes.data_as(C.POINTER(C.c_float)), C.byref(sys), C.byref(it))
    assert rc == 1 and np.array_equal(d, start32.reshape(16)) and it.value == -5          # VH_ERR_INVALID_ARGUMENT
    trk.close()

    s = scene(oracle, torch, (40, 30))
    _, (gp, gt, gn) = s.step()
    res = []
    for stamps in (False, True):
        with monkeypatch.context() as m:
            if stamps:
                m.setenv("VH_ICP_STAMPS", "1")
            trk = tracker(40, 30, s.K, monkeypatch, flags=3)
        trk.max_iters = 200
        res.append((trk.Align(gp, gt, gn).copy(), trk.last, trk.iterations))
        trk.close()
    assert res[0][2] == 200
    assert_bit_equal([res[0]], [res[1]])


def test_fusion_step_is_track_then_fuse_at_80x60(vh, torch_cuda):
    """vh_fusion_step at 80x60 (a one-launch Align on 19 workgroups, one pixel per lane) against the same stages called one by
    one (FusionLoop.track + FusionLoop.fuse), as test_gpu_icp.test_fusion_step_is_track_then_fuse does at 320x240."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    w, h = 80, 60
    prims = synth.room_primitives()
    gt_poses = synth.camera_loop(500)[200:206]
    K = synth.K_matrix(w, h)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    dev = [(synth.render_room_verts(p, w, h, prims, device="cuda")[..., 2] * 5000.0).round().clamp(0, 65535).to(torch.uint16)
           for p in gt_poses]
    kw = dict(numBuckets=1 << 14, numVoxelBlocks=1 << 12)
    flags = tracking.ICP_ABS_DISTANCE | tracking.ICP_NEED_TARGET
    tables = [vh.SDFHashtable(vh.default_params(**kw), w, h, 1) for _ in range(2)]
    loops = [tracking.FusionLoop(t, K, kinv, flags=flags) for t in tables]
    for lp in loops:
        assert icp_layout(lp.trk) == expected_layout(w, h) == (19, 19, 1)
        lp.start(dev[0], gt_poses[0])
    for k in range(1, len(gt_poses)):
        a = loops[0].step(dev[k]).copy()
        loops[1].track(dev[k])
        loops[1].fuse(dev[k])
        b = loops[1].pose
        assert loops[0].trk.iterations == loops[1].trk.iterations == 20
        assert loops[0].trk.last[3] > 0.5 * w * h
        assert np.abs(a - b).max() < 1e-5, (k, np.abs(a - b).max())
    ca, cb = tables[0].counters(), tables[1].counters()
    assert abs(ca["allocated_total"] - cb["allocated_total"]) <= 0.01 * ca["allocated_total"]
    for lp in loops:
        lp.close()
    for t in tables:
        t.close()
