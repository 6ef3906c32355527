"""vh_sdf_build_system, vh_sdf_residuals, vh_sdf_align and vh_fusion_step_sdf on the GPU against the rule in numpy
(tests/sdf_track_ref.py, pinned by tests/test_sdf_track_ref_cpu.py).  The per-pixel maps are bit-equal on models the tests
choose themselves; the 29 sums are fp32 sums in a fixed order on the GPU and float64 sums in the rule, compared by the
tracker's own tolerance (close_sums of tests/test_gpu_icp.py); Align and the closed loop run on the synthetic room.  Every
crafted case asserts, on the rule's own answer, the conditions without which it could pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import mesh_models as mm
import sample_ref as sr
import sdf_track_ref as ref
from test_gpu_icp import close_sums
from test_gpu_sample import context_with, points_in_blocks
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
W, H = 320, 240
VS = 0.02
CANARY = -7.5
CRAFTED_THRES = 0.25          # the crafted models hold noise in (-1, 1): about half of the samples lie inside
POSE = ref.se3_exp([0.4, -0.3, 0.2, 0.3, -0.2, 0.25])
MODELS = {"every_configuration": mm.every_configuration, "seam": lambda: mm.uniform_model(mm.cube_keys(-2, 1), seed=31),
          "non_finite": mm.non_finite}
# one wave; a ragged single workgroup; several workgroups with a ragged tail; several passes per lane
SIZES = [(8, 8), (33, 7), (100, 37), (320, 240)]


def crafted_input(model, w, h, seed):
    """A w x h float4 input map in the camera frame of POSE: points inside the cells of the model's blocks (a quarter of them
    on a block's last layer on a random set of axes), every 7th pixel without a point (z == 0), every 11th well outside the
    model."""
    rng = np.random.RandomState(seed)
    n = w * h
    world = points_in_blocks(rng, list(model), n, VS).astype(np.float64)
    idx = np.arange(n)
    world[idx % 11 == 5] += 40.0
    inv = np.linalg.inv(POSE)
    cam = np.concatenate([world @ inv[:3, :3].T + inv[:3, 3], np.ones((n, 1))], 1).astype(F)
    cam[idx % 7 == 3] = 0
    assert (cam[idx % 7 != 3, 2] != 0).all()
    return cam.reshape(h, w, 4)


def guards(q, s, g, kept, sampled, have, non_finite, full):
    """The conditions on the rule's own answer; `full`: the image is large enough for the counted ones."""
    share = kept.mean()
    assert 0.15 <= share <= 0.85, share
    with np.errstate(invalid="ignore"):
        far = sampled & np.isfinite(s) & ~(np.abs(s) < F(CRAFTED_THRES))
        bad = sampled & ~(np.isfinite(g).all(1) & np.isfinite(s))
    kinds = {"no point": ~have, "no sample": have & ~sampled, "far": far}
    if non_finite and full:
        kinds["not finite"] = bad
    for name, mask in kinds.items():
        assert mask.sum() >= 1 and not kept[mask].any(), name
    i = np.floor((q / F(VS)).astype(F)).astype(np.int64)
    code = ((i & 7) == 7) @ np.array([1, 2, 4])
    counts = [int((kept & (code == c)).sum()) for c in range(8)]
    if full:
        # mm.non_finite() is 2 x 2 x 2 blocks: ONE cell crosses a block face on all three axes, and one of its corners holds
        # +inf (asserted in crafted_case), so code 7 cannot have a kept point there; the other two models have all eight
        assert min(counts[:7] if non_finite else counts) >= 20, counts
    return share, counts


def crafted_case(name, w, h):
    model = MODELS[name]()
    inp = crafted_input(model, w, h, seed=100 + w)
    field = sr.Field(model)
    q, s, g, kept, sampled = ref.pixels(field, inp, POSE, VS, CRAFTED_THRES)
    have = inp.reshape(-1, 4)[:, 2] != 0
    if name == "non_finite":
        corners = np.array([-1, -1, -1]) + np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])
        assert set(model) == set(mm.cube_keys(-1, 1)) and np.isinf(field.voxels(corners)[0]).any()
    share, counts = guards(q, s, g, kept, sampled, have, name == "non_finite", (w, h) == (W, H))
    return model, inp, (q, s, g, kept), share, counts


def tracker(vh, gt, w, h, **kw):
    from voxelhashing_demo_amd import tracking
    return tracking.SdfTracking(gt, width=w, height=h, **kw)


# ---- 1. per-pixel maps and sums on crafted models --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_maps_and_sums_on_crafted_models(vh, torch_cuda, tmp_path, name):
    torch = torch_cuda
    gt = None
    for w, h in SIZES:
        model, inp, (q, s, g, kept), share, counts = crafted_case(name, w, h)
        if gt is None:
            gt = context_with(vh, model, tmp_path)
        trk = tracker(vh, gt, w, h, dist_thres=CRAFTED_THRES)
        d_in = torch.from_numpy(inp).cuda()
        guard = 64
        bufs = [torch.full((guard + w * h * k + guard,), CANARY, dtype=torch.float32, device="cuda") for k in (3, 1, 3)]
        got = trk.residuals(d_in, POSE, *(b[guard:guard + w * h * k] for b, k in zip(bufs, (3, 1, 3))))
        want_maps = ref.maps(q, s, g, kept)
        for what, b, k, wm in zip(("points", "sdf", "gradient"), bufs, (3, 1, 3), want_maps):
            hb = b.cpu().numpy()
            assert (hb[:guard] == CANARY).all() and (hb[guard + w * h * k:] == CANARY).all(), (what, w, h)
            assert sr.same_bits(hb[guard:guard + w * h * k], wm.reshape(-1)), (what, w, h)
        want = ref.system(q, s, g, kept)
        print(f"{name} {w}x{h}: kept {want[3]} of {w * h} ({share:.2f}), per face code {counts}")
        close_sums(got, want)                                # count exact, sums by the tracker's tolerance, JTJ symmetric
        for again in (trk.build_system(d_in, POSE), trk.build_system(d_in, POSE)):       # without the maps; run to run
            assert again[3] == got[3] and again[2] == got[2]
            assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
        trk.close()
    gt.close()


# ---- 2. Align on the room --------------------------------------------------------------------------------------------------
ROOM = dict(numBuckets=1 << 16, numVoxelBlocks=1 << 14, truncation=0.06)


def room(torch, lo, hi):
    prims = synth.room_primitives()
    poses = [np.asarray(p, np.float64).reshape(4, 4) for p in synth.camera_loop(500)[lo:hi]]
    K = synth.K_matrix(W, H)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    d16 = [(synth.render_room_verts(p, W, H, prims, device="cuda")[..., 2] * 5000.0).round().clamp(0, 65535).to(torch.uint16)
           for p in poses]
    return poses, K, kinv, d16


def translation_error(a, b):
    return float(np.abs(np.asarray(a)[:3, 3] - np.asarray(b)[:3, 3]).max())


def test_align_matches_the_rule_and_halves_the_error(vh, torch_cuda):
    from voxelhashing_demo_amd import hashtable
    torch = torch_cuda
    poses, K, kinv, d16 = room(torch, 200, 205)
    gt = vh.SDFHashtable(vh.default_params(**ROOM), W, H, 1)
    for k in range(4):
        gt.integrate_depth(poses[k].astype(F), d16[k], kinv)
    in_v, in_n = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    hashtable.preprocess(d16[4], kinv, in_v, in_n)
    trk = tracker(vh, gt, W, H, dist_thres=0.08, max_iters=10)
    got = trk.Align(in_v, poses[3]).copy()
    assert trk.iterations == 10 and trk.last[3] > 0.5 * W * H
    model = mm.model_of(gt.hash_table(), gt.sdf_blocks())
    want, last, steps = ref.align(model, in_v.cpu().numpy(), poses[3], VS, 0.08, 10)
    start, e_got, e_want = (translation_error(p, poses[4]) for p in (poses[3], got, want))
    print(f"align: start {1e3 * start:.2f} mm, library {1e3 * e_got:.2f} mm, rule {1e3 * e_want:.2f} mm, "
          f"library - rule {np.abs(got - want).max():.2e}, kept {trk.last[3]} / {last[3]}")
    assert steps == 10
    assert np.abs(got - want).max() < 2e-4             # fp32 sums against double sums (test_align_matches_oracle_and_truth)
    assert e_got <= 0.5 * start and e_want <= 0.5 * start
    trk.close()
    gt.close()


# ---- 3. the closed loop ----------------------------------------------------------------------------------------------------
def test_tracking_loop_without_a_raycast(vh, torch_cuda):
    """Only frame 0 is given its pose; the bounds are those of test_frame_to_model_tracking_loop for the ICP loop."""
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    poses, K, kinv, d16 = room(torch, 200, 212)
    gt = vh.SDFHashtable(vh.default_params(**ROOM), W, H, 1)
    loop = tracking.SdfFusionLoop(gt, kinv, K, dist_thres=0.08, max_iters=10)
    loop.start(d16[0], poses[0])
    errs = []
    for k in range(1, len(poses)):
        pose = loop.step(d16[k])
        assert loop.trk.last[3] > 0.5 * W * H, (k, loop.trk.last[3])
        errs.append(translation_error(pose, poses[k]))
    moved = translation_error(poses[-1], poses[0])
    assert moved > 0.1 and loop.frames == len(poses)
    print(f"sdf tracking drift: {1e3 * max(errs):.2f} mm over {1e3 * moved:.0f} mm ({', '.join(f'{1e3 * e:.1f}' for e in errs)})")
    assert max(errs) < 0.012, errs
    loop.close()
    gt.close()


def test_fusion_step_sdf_is_track_then_fuse(vh, torch_cuda):
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    poses, K, kinv, d16 = room(torch, 200, 205)
    tables = [vh.SDFHashtable(vh.default_params(**ROOM), W, H, 1) for _ in range(2)]
    loops = [tracking.SdfFusionLoop(t, kinv, K, dist_thres=0.08, max_iters=10) for t in tables]
    for lp in loops:
        lp.start(d16[0], poses[0])
    for k in range(1, len(poses)):
        a = loops[0].step(d16[k]).copy()
        loops[1].track(d16[k])
        loops[1].fuse(d16[k])
        b = loops[1].pose
        assert loops[0].trk.iterations == loops[1].trk.iterations == 10
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (k, np.abs(a - b).max())
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(loops[0].trk.last, loops[1].trk.last))
        assert translation_error(a, poses[k]) < 0.012
    assert loops[0].frames == loops[1].frames == len(poses)
    ma, mb = (mm.model_of(t.hash_table(), t.sdf_blocks()) for t in tables)      # (block ids may be handed out in another order)
    assert len(ma) > 100 and sorted(ma) == sorted(mb)               # (a few hundred surface blocks)
    assert all(ma[k][0].tobytes() == mb[k][0].tobytes() and ma[k][1].tobytes() == mb[k][1].tobytes() for k in ma)
    for lp in loops:
        lp.close()
    for t in tables:
        t.close()


# ---- 4. queueing -----------------------------------------------------------------------------------------------------------
def test_sees_a_pending_pipelined_frame(vh, torch_cuda):
    from voxelhashing_demo_amd import hashtable
    torch = torch_cuda
    poses, K, kinv, d16 = room(torch, 200, 204)
    in_v, in_n = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    hashtable.preprocess(d16[3], kinv, in_v, in_n)
    results = []
    for pipeline in (0, 1):
        gt = vh.SDFHashtable(vh.default_params(**ROOM), W, H, 1)
        gt.set_option("pipeline", pipeline)
        for k in range(3):
            gt.integrate_depth(poses[k].astype(F), d16[k], kinv)        # pipelined: the last frame's second half is pending
        trk = tracker(vh, gt, W, H, dist_thres=0.08)
        results.append(trk.build_system(in_v, poses[2]))
        trk.close()
        gt.close()
    a, b = results
    assert a[3] > 0.5 * W * H
    assert a[3] == b[3] and a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 5. refusals and the empty model ---------------------------------------------------------------------------------------
def test_refusals_and_the_empty_model(vh, torch_cuda, tmp_path):
    from voxelhashing_demo_amd import _lib as L
    from voxelhashing_demo_amd import tracking
    torch = torch_cuda
    lib = vh.load()
    model = mm.every_configuration()
    gt = context_with(vh, model, tmp_path)
    w, h = 33, 7
    inp = torch.from_numpy(crafted_input(model, w, h, seed=5)).cuda()
    trk = tracker(vh, gt, w, h, dist_thres=CRAFTED_THRES)
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    good = trk.build_system(inp, POSE)
    assert good[3] > 0
    fp, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p32, p64 = np.ascontiguousarray(POSE, F).reshape(16), np.ascontiguousarray(POSE, np.float64).reshape(16)
    sys_, it = L.IcpSystem(), C.c_int32()
    maps = [torch.full((w * h * k,), CANARY, dtype=torch.float32, device="cuda") for k in (3, 1, 3)]
    d_in, ctx, icp = inp.data_ptr(), gt._h, trk._h
    trk_table = tracker(vh, gt, 640, 480, dist_thres=CRAFTED_THRES)              # vh_fusion_step_sdf: the table's image size
    icp_table = trk_table._h
    depth = torch.zeros((480, 640), dtype=torch.uint16, device="cuda")
    big = [torch.empty((480, 640, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    kinv = np.ascontiguousarray(np.linalg.inv(synth.K_matrix(640, 480).astype(np.float64)), F).reshape(9)
    m = [t.data_ptr() for t in maps]

    def build(c=ctx, i=icp, d=d_in, p=p32, thres=CRAFTED_THRES, out=sys_):
        return lib.vh_sdf_build_system(c, i, d, None if p is None else fp(p), thres, None if out is None else C.byref(out))

    def resid(c=ctx, i=icp, d=d_in, p=p32, thres=CRAFTED_THRES, a=m[0], b=m[1], g=m[2], out=sys_):
        return lib.vh_sdf_residuals(c, i, d, None if p is None else fp(p), thres, a, b, g, None if out is None else C.byref(out))

    def align(c=ctx, i=icp, d=d_in, thres=CRAFTED_THRES, iters=3, p=p64):
        return lib.vh_sdf_align(c, i, d, thres, iters, None if p is None else dp(p), C.byref(sys_), C.byref(it))

    def step(c=ctx, i=icp_table, d=depth.data_ptr(), k=kinv, thres=CRAFTED_THRES, iters=3, v=big[0].data_ptr(), n=big[1].data_ptr(), p=p64):
        return lib.vh_fusion_step_sdf(c, i, d, None if k is None else fp(k), thres, iters, v, n, None if p is None else dp(p),
                                      C.byref(sys_), C.byref(it))

    def poisoned(a, value):
        b = a.copy()
        b[7] = value
        return b

    refused = []
    # a NULL argument
    refused += [build(c=None), build(i=None), build(d=None), build(p=None), build(out=None)]
    refused += [resid(c=None), resid(i=None), resid(d=None), resid(p=None), resid(a=None), resid(b=None), resid(g=None), resid(out=None)]
    refused += [align(c=None), align(i=None), align(d=None), align(p=None)]
    refused += [step(c=None), step(i=None), step(d=None), step(k=None), step(v=None), step(n=None), step(p=None)]
    # a pose or dist_thres that is not finite, dist_thres <= 0
    for bad in (np.nan, np.inf, -np.inf):
        refused += [build(p=poisoned(p32, bad)), resid(p=poisoned(p32, bad)), align(p=poisoned(p64, bad)), step(p=poisoned(p64, bad))]
        refused += [build(thres=bad), resid(thres=bad), align(thres=bad), step(thres=bad)]
    for bad in (0.0, -0.08):
        refused += [build(thres=bad), resid(thres=bad), align(thres=bad), step(thres=bad)]
    # max_iters outside 0..65536
    refused += [align(iters=-1), align(iters=65537), step(iters=-1), step(iters=65537)]
    # vh_fusion_step_sdf with a workspace of another image size
    refused += [step(i=icp)]
    assert refused and all(rc == 1 for rc in refused), refused                   # VH_ERR_INVALID_ARGUMENT
    # a workspace of another device: only where there is one
    if torch.cuda.device_count() > 1:
        h2 = C.c_void_p()
        assert lib.vh_icp_create(w, h, 1, C.byref(h2)) == 0
        assert build(i=h2) == 1 and align(i=h2) == 1
        lib.vh_icp_destroy(h2)
    # ... and of another stream
    other = torch.cuda.Stream()
    lib.vh_icp_set_stream(icp, C.c_void_p(other.cuda_stream))
    assert build() == 1 and align() == 1
    lib.vh_icp_set_stream(icp, C.c_void_p(gt.stream_handle))
    torch.cuda.synchronize()
    for t in maps:
        assert (t.cpu().numpy() == CANARY).all()                                 # nothing was launched
    assert np.array_equal(p64, np.ascontiguousarray(POSE, np.float64).reshape(16))
    # the accepted edges: max_iters 0 gives the pose back, the workspace still works
    assert align(iters=0) == 0 and it.value == 0 and np.array_equal(p64.reshape(4, 4), POSE)
    again = trk.build_system(inp, POSE)
    assert again[3] == good[3] and np.array_equal(again[0], good[0])
    assert state(gt) == s0
    gt.close()
    # the empty model: count 0, a singular system, the pose as given
    empty = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=64), 640, 480, 1)
    trk2 = tracker(vh, empty, w, h, dist_thres=CRAFTED_THRES)
    JTJ, JTr, err, cnt = trk2.build_system(inp, POSE)
    assert cnt == 0 and err == 0 and not JTJ.any() and not JTr.any()
    assert not tracking.icp_solve(JTJ, JTr, np.zeros(6))[0]
    out = trk2.Align(inp, POSE)
    assert trk2.iterations == 0 and trk2.last[3] == 0 and np.array_equal(out, POSE)
    trk2.close()
    trk.close()
    trk_table.close()
    empty.close()
