"""vh_cast_rays on the GPU against the specification (tests/rays_ref.py, pinned by tests/test_rays_ref_cpu.py), bit for bit (two
NaNs count as equal): the crafted views of tests/raycast_cases.py cast as ray lists on every table form, against vh_raycast of
the same context pixel for pixel, with and without the shared plane; incoherent waves; the edges of the walk; sizes, refusals,
optional outputs, argument errors; shards, overflow chains, queued frames, purity, repeats, and the C++ facade.  Every case
asserts, on the reference's own answer, a condition without which it could pass vacuously."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_models as mm
import raycast_cases as rc
import rays_ref
from test_gpu_gc import frames
from test_gpu_mesh import fuse, shard_pair, table_of
from test_rays_ref_cpu import ramp_wall, refusals
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
MARKER = -7.5
IMARKER = -77
CELLS = [pytest.param(c, table, id=f"{c.name}-{table}") for c in rc.CASES for table in c.tables]


def case_rays(vh, case):
    return vh.pinhole_rays(case.pose, case.focal, case.focal, case.cx, case.cy, case.W, case.H, *case.t)


def case_plane(oracle, case):
    return np.asarray(oracle.invert4x4(case.pose), F).reshape(4, 4)[2]


def cast(torch, gt, rays, plane=None):
    """(t, normals, voxels with the status word) of the GPU, as numpy."""
    d = torch.from_numpy(np.ascontiguousarray(rays, F)).cuda()
    t, n, v = gt.cast_rays(d, plane, normals=True, voxels=True)
    gt.synchronize()
    return t.cpu().numpy(), n.cpu().numpy(), v.cpu().numpy()


def assert_same(got, want, what=""):
    """GPU (t, normal, voxel + status) against rays_ref.cast's (t, status, voxel, normal, record)."""
    t, n, v = got
    wt, ws, wv, wn, rec = want
    assert np.array_equal(v[:, 3], ws), f"{what}: status differs at rays {np.nonzero(v[:, 3] != ws)[0][:8]}"
    assert np.array_equal(v[:, :3], wv), f"{what}: hit voxel differs at rays {np.nonzero((v[:, :3] != wv).any(1))[0][:8]}"
    assert rays_ref.same_bits(t, wt), f"{what}: t differs at rays {np.nonzero(~((t == wt) | (np.isnan(t) & np.isnan(wt))))[0][:8]}"
    assert rays_ref.same_bits(n, wn), f"{what}: normals differ"


def context_with(vh, model, tmp_path, **kw):
    gt = vh.SDFHashtable(vh.default_params(voxelSize=rc.VS, **(kw or dict(rc.TABLES["a"], numVoxelBlocks=rc.POOL))), 64, 48, 1)
    return mm.load_model(gt, model, tmp_path)


@pytest.fixture(scope="module")
def contexts(vh, torch_cuda, tmp_path_factory):
    """One context per (model, table, image size), as tests/test_gpu_raycast_crafted.py builds them: (a) comfortable, (b) crowded
    13-bucket, (c) a view table, (d) (a) after deleting a third of the keys."""
    torch = torch_cuda
    memo = {}

    def get(case, table):
        key = (id(case.model), table, case.size)
        if key in memo:
            return memo[key]
        kw = dict(voxelSize=rc.VS, **rc.TABLES[table])
        if table == "c":
            rec = torch.from_numpy(mm.view_records(case.model)).cuda()
            gt = vh.SDFHashtable(vh.default_params(numVoxelBlocks=1, **kw), case.W, case.H, 1)
            gt.import_view(rec, len(case.model))
        else:
            gt = vh.SDFHashtable(vh.default_params(numVoxelBlocks=rc.POOL, **kw), case.W, case.H, 1)
            mm.load_model(gt, case.model, tmp_path_factory.mktemp("snap"))
            if table == "d":
                gone = np.zeros((len(rc.deleted_keys(case.model)), 4), np.int32)
                gone[:, :3] = rc.deleted_keys(case.model)
                gt.delete_blocks(torch.from_numpy(gone).cuda())
                gt.synchronize()
                assert sorted(map(tuple, gt.allocated()["pos"].tolist())) == sorted(rc.reduced(case.model))
        memo[key] = gt
        return gt
    yield get
    for gt in memo.values():
        gt.close()


@pytest.fixture(scope="module")
def refs(vh, oracle):
    """rays_ref on a crafted case (its model, or the reduced one of table d), with the shared plane or along each ray: once."""
    memo, fields = {}, {}

    def get(case, reduced, shared):
        key = (case.name, reduced, shared)
        if key not in memo:
            fkey = (id(case.model), reduced)
            if fkey not in fields:
                fields[fkey] = rays_ref.Field(rc.reduced(case.model) if reduced else case.model)
            memo[key] = rays_ref.cast(fields[fkey], rc.VS, case_rays(vh, case), case_plane(oracle, case) if shared else None)
        return memo[key]
    return get


# ---- 1. the crafted views as ray lists, on every table form ------------------------------------------------------------
@pytest.mark.parametrize("case,table", CELLS)
def test_crafted_case(vh, oracle, torch_cuda, contexts, refs, case, table):
    torch = torch_cuda
    gt = contexts(case, table)
    rays, plane = case_rays(vh, case), case_plane(oracle, case)
    want = refs(case, table == "d", True)
    got = cast(torch, gt, rays, plane)
    assert_same(got, want, "shared plane")
    assert (want[1] == 1).mean() > 0.02
    # vh_raycast / vh_raycast_normals of the same context, pixel for pixel: depth bits (its 0 for a miss <-> NaN), normals
    # through the rotation n_i = (T[0,i] w0 + T[1,i] w1) + T[2,i] w2
    gt.set_raycast_intrinsics(case.focal, case.focal, case.cx, case.cy)
    d = torch.full((case.H, case.W), MARKER, dtype=torch.float32, device="cuda")
    n = torch.full((case.H, case.W, 4), MARKER, dtype=torch.float32, device="cuda")
    gt.raycast_normals(case.pose, d, n, *case.t)
    gt.synchronize()
    depth, normals = d.cpu().numpy().reshape(-1), n.cpu().numpy().reshape(-1, 4)
    t, w, v = got
    hit = v[:, 3] == 1
    assert (depth[~hit] == 0).all() and rc.same_image(t[hit], depth[hit], case.nan)
    T = case.pose
    with np.errstate(all="ignore"):
        cam = np.stack([(T[0, i] * w[:, 0] + T[1, i] * w[:, 1]) + T[2, i] * w[:, 2] for i in range(3)], 1)
    assert rc.same_image(cam, normals[:, :3], case.nan) and (normals[:, 3] == 0).all()
    # the same list along each ray
    want = refs(case, table == "d", False)
    assert_same(cast(torch, gt, rays), want, "along each ray")
    assert (want[1] == 1).mean() > 0.02


def test_exact_ties_and_the_far_cluster_are_what_they_claim(refs):
    """The census of the views above, along each ray: the wall views tie two and three axes and have inactive axes, the far
    cluster sits at voxel coordinate 2^20."""
    walls = [c for c in rc.CASES if "wall" in c.kinds]
    rec = [refs(c, False, False)[4] for c in walls]
    assert sum(int((r["tie_xyz"] > 0).sum()) for r in rec) > 100 and sum(int((r["inactive"] == 2).sum()) for r in rec) >= len(walls)
    assert sum(int(((r["tie_xy"] > 0) | (r["tie_xz"] > 0) | (r["tie_yz"] > 0)).sum()) for r in rec) > 1000
    far = refs(rc.BY_NAME["far"], False, False)
    assert (far[1] == 1).mean() > 0.25 and np.abs(far[2][far[1] == 1]).max() >= rc.FAR_KEY * 8


# ---- 2. incoherent waves -----------------------------------------------------------------------------------------------
def test_incoherent_waves(vh, torch_cuda, contexts):
    """The rays of six views of the noise model, each ray with a range of its own, concatenated and shuffled: every lane of a
    wave has its own origin, direction and range.  The result is the same permutation of the in-order result."""
    views = [rc.BY_NAME[f"noise{v}"] for v in rc.AXES]
    assert all(c.model is views[0].model for c in views)
    rng = np.random.RandomState(61)
    rays = np.concatenate([case_rays(vh, c) for c in views])
    lo, hi = np.concatenate([np.full(c.W * c.H, c.t[0], F) for c in views]), np.concatenate([np.full(c.W * c.H, c.t[1], F) for c in views])
    mid = (lo + hi) / 2
    rays[:, 3] = rng.uniform(lo, mid).astype(F)
    rays[:, 7] = rng.uniform(mid, hi).astype(F)
    gt = contexts(views[0], "a")
    want = rays_ref.cast(views[0].model, rc.VS, rays)
    in_order = cast(torch_cuda, gt, rays)
    assert_same(in_order, want, "in order")
    perm = rng.permutation(len(rays))
    shuffled = cast(torch_cuda, gt, rays[perm])
    for a, b in zip(shuffled, in_order):
        assert np.array_equal(a.view(U), b[perm].view(U))
    hits = want[1] == 1
    print(f"rays={len(rays)} hits={hits.mean():.2f} events: mean {want[4]['events'].mean():.1f} most {want[4]['events'].max()}")
    assert 0.2 < hits.mean() < 0.98 and len(np.unique(rays[perm][:64, 0:3], axis=0)) >= 4


# ---- 3. edges of the walk ----------------------------------------------------------------------------------------------
def test_edges_of_the_walk(vh, torch_cuda, contexts):
    case = rc.BY_NAME["noise+z"]
    model = case.model
    gt = contexts(case, "a")
    field = rays_ref.Field(model)
    keys = np.array(list(model))
    lo, hi = keys.min(0) * 8 * rc.VS, (keys.max(0) * 8 + 8) * rc.VS
    rng = np.random.RandomState(62)
    n = 512

    def random_dirs(k):
        d = rng.normal(size=(k, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (k, 1))).astype(F)

    # origins inside the model, t_min < 0 and t_min = 0
    inside = np.zeros((2 * n, 8), F)
    inside[:, 0:3] = rng.uniform(lo, hi, (2 * n, 3))
    inside[:, 4:7] = random_dirs(2 * n)
    inside[:n, 3], inside[n:, 3], inside[:, 7] = -0.1, 0.0, rng.uniform(0.005, 0.2, 2 * n)       # (many end after a voxel or two)
    want = rays_ref.cast(field, rc.VS, inside)
    assert_same(cast(torch_cuda, gt, inside), want, "origins inside")
    rec = want[4]
    print(f"origins inside: starts in allocated {rec['starts_in_allocated'].mean():.2f}, ends in allocated {rec['ends_in_allocated'].mean():.2f}, "
          f"hits {(want[1] == 1).mean():.2f}")
    assert rec["starts_in_allocated"][:n].mean() > 0.3 and rec["starts_in_allocated"][n:].mean() > 0.5
    assert (rec["ends_in_allocated"] & (want[1] == 0)).sum() > 10 and (want[1] == 1).mean() > 0.3      # rays that end inside a block without a hit
    # wholly in absent space
    away = inside.copy()
    away[:, 0:3] += (hi - lo) * 3 + 1.0
    away[:, 4:7] = np.abs(away[:, 4:7])
    want = rays_ref.cast(field, rc.VS, away)
    assert_same(cast(torch_cuda, gt, away), want, "absent space")
    assert (want[1] == 0).all() and not want[4]["starts_in_allocated"].any()
    # two inactive axes: along +-x, +-y, +-z through the model, from outside and from inside
    axis = np.zeros((6 * 64, 8), F)
    for i, (a, sgn) in enumerate(rc.AXES.values()):
        rows = slice(64 * i, 64 * i + 64)
        o = rng.uniform(lo, hi, (64, 3))
        o[:32, a] = lo[a] - 0.05 if sgn > 0 else hi[a] + 0.05
        axis[rows, 0:3] = o
        axis[rows, 4 + a] = sgn * rng.choice([0.5, 1.0, 3.0], 64)
    axis[:, 3], axis[:, 7] = 0.0, 0.6
    want = rays_ref.cast(field, rc.VS, axis)
    assert_same(cast(torch_cuda, gt, axis), want, "axis-aligned")
    assert (want[4]["inactive"] == 2).all() and (want[1] == 1).mean() > 0.5


def test_axis_aligned_rays_hit_the_ramp_at_the_analytic_t(vh, torch_cuda, tmp_path):
    """The hand-computed fact of tests/test_rays_ref_cpu.py, on the GPU: t = (19.5 - z0) * VS / |D| exactly."""
    gt = context_with(vh, ramp_wall(), tmp_path)
    vs = F(rc.VS)
    rays = np.array([[x * vs, y * vs, z0 * vs, 0.0, 0.0, 0.0, d, 1.0]
                     for x, y, z0, d in ((0, 0, 4, 1.0), (-3, 5, 0, 1.0), (2, -7, -12, 1.0), (0, 0, 4, 2.0), (-3, 5, 0, 0.5), (5, 5, 8, 4.0))], F)
    t, n, v = cast(torch_cuda, gt, rays)
    want = np.array([(19.5 - r[2] / vs) * vs / r[6] for r in rays], F)
    assert np.array_equal(t.view(U), want.view(U)) and (v[:, 3] == 1).all() and (v[:, 2] == 20).all()
    assert np.array_equal(n, np.tile(np.array([0, 0, -1], F), (len(rays), 1)))
    gt.close()


# ---- 4. sizes ----------------------------------------------------------------------------------------------------------
def test_sizes_and_markers(vh, torch_cuda, contexts):
    """n around a wave and a workgroup, and 2049: the grid is rounded up to 8 workgroups of 256 rays, 2049 is the first size
    with a second round of them.  Marker values behind each output buffer stay untouched."""
    torch = torch_cuda
    case = rc.BY_NAME["noise general"]
    gt = contexts(case, "a")
    rays = case_rays(vh, case)[np.random.RandomState(63).permutation(case.W * case.H)]
    want = rays_ref.cast(case.model, rc.VS, rays)
    assert 0.2 < (want[1] == 1).mean() < 0.98
    guard = 64
    for n in (1, 63, 64, 65, 255, 256, 257, 2049, len(rays)):
        d = torch.from_numpy(rays[:n].copy()).cuda()
        t = torch.full((n + guard,), MARKER, dtype=torch.float32, device="cuda")
        nr = torch.full((3 * n + guard,), MARKER, dtype=torch.float32, device="cuda")
        vx = torch.full((4 * n + guard,), IMARKER, dtype=torch.int32, device="cuda")
        gt.cast_rays_into(d, t[:n], nr[:3 * n], vx[:4 * n])
        gt.synchronize()
        t, nr, vx = t.cpu().numpy(), nr.cpu().numpy(), vx.cpu().numpy()
        assert (t[n:] == MARKER).all() and (nr[3 * n:] == MARKER).all() and (vx[4 * n:] == IMARKER).all(), n
        assert_same((t[:n], nr[:3 * n].reshape(n, 3), vx[:4 * n].reshape(n, 4)), tuple(w[:n] for w in want[:4]) + (None,), f"n={n}")
        # the count argument, not the tensor's length, bounds the call
        t2 = torch.full((n + guard,), MARKER, dtype=torch.float32, device="cuda")
        gt.cast_rays_into(torch.from_numpy(rays[:n + guard].copy()).cuda(), t2, n=n)
        gt.synchronize()
        assert (t2.cpu().numpy()[n:] == MARKER).all() and rays_ref.same_bits(t2.cpu().numpy()[:n], want[0][:n])


# ---- 5. refused rays ---------------------------------------------------------------------------------------------------
def test_refused_rays_among_good_ones(vh, torch_cuda, tmp_path):
    """Every kind of refusal interleaved with good rays, several per wave: status -1, t NaN, zeros; the neighbours are unaffected."""
    model = ramp_wall()
    gt = context_with(vh, model, tmp_path)
    good, bad = refusals()
    vs = F(rc.VS)
    rng = np.random.RandomState(64)
    rows, is_bad = [], []
    for name, r in bad:
        for _ in range(1 + len(rows) % 3):
            g = np.array([rng.randint(-8, 8) * vs, rng.randint(-8, 8) * vs, rng.randint(-4, 12) * vs, 0.0, 0.0, 0.0, 1.0, 1.0], F)
            rows.append(g)
            is_bad.append(False)
        rows.append(r)
        is_bad.append(True)
    rays, is_bad = np.stack(rows), np.array(is_bad)
    assert is_bad[:64].sum() >= 16 and (~is_bad[:64]).sum() >= 16
    want = rays_ref.cast(model, rc.VS, rays)
    assert np.array_equal(want[1] == -1, is_bad) and (want[1][~is_bad] == 1).all()
    t, n, v = got = cast(torch_cuda, gt, rays)
    assert_same(got, want, "refusals")
    assert np.isnan(t[is_bad]).all() and (v[is_bad] == [0, 0, 0, -1]).all() and (n[is_bad] == 0).all()
    # with the shared plane too (the plane changes nothing about who is refused)
    assert_same(cast(torch_cuda, gt, rays, (0.0, 0.0, 1.0, 0.0)), rays_ref.cast(model, rc.VS, rays, (0.0, 0.0, 1.0, 0.0)), "refusals, plane")
    gt.close()


# ---- 6. optional outputs, argument errors, n = 0 -----------------------------------------------------------------------
def test_optional_outputs(vh, torch_cuda, contexts):
    case = rc.BY_NAME["noise general"]
    gt = contexts(case, "a")
    d = torch_cuda.from_numpy(case_rays(vh, case)).cuda()
    t, n, v = (x.cpu().numpy() for x in gt.cast_rays(d, normals=True, voxels=True))
    only = gt.cast_rays(d).cpu().numpy()
    tn = [x.cpu().numpy() for x in gt.cast_rays(d, normals=True)]
    tv = [x.cpu().numpy() for x in gt.cast_rays(d, voxels=True)]
    assert rays_ref.same_bits(only, t) and rays_ref.same_bits(tn[0], t) and rays_ref.same_bits(tv[0], t)
    assert rays_ref.same_bits(tn[1], n) and np.array_equal(tv[1], v) and (v[:, 3] == 1).mean() > 0.2


def test_python_buffer_checks(vh, torch_cuda, contexts):
    """cast_rays_into refuses what would become a write out of bounds: a wrong dtype or shape, a buffer shorter than n."""
    torch = torch_cuda
    gt = contexts(rc.BY_NAME["noise general"], "a")
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    rays = z((16, 8))
    gt.cast_rays_into(rays, z(16), z((16, 3)), z((16, 4), torch.int32))
    gt.cast_rays_into(rays, z(8), n=8)
    for bad in (lambda: gt.cast_rays_into(z((16, 8), torch.float64), z(16)), lambda: gt.cast_rays_into(z((16, 6)), z(16)),
                lambda: gt.cast_rays_into(z(128), z(16)), lambda: gt.cast_rays_into(rays, z(15)),
                lambda: gt.cast_rays_into(rays, z(16, torch.float64)), lambda: gt.cast_rays_into(rays, z(16), z((15, 3))),
                lambda: gt.cast_rays_into(rays, z(16), None, z((16, 4))), lambda: gt.cast_rays_into(rays, z(16), None, z((16, 3), torch.int32)),
                lambda: gt.cast_rays_into(rays, z(32), n=17), lambda: gt.cast_rays_into(rays, None)):
        with pytest.raises(ValueError):
            bad()
    gt.synchronize()


def test_argument_errors(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    gt = context_with(vh, ramp_wall(), tmp_path)
    lib, h = vh.load(), gt._h
    vs = F(rc.VS)
    rays = torch.from_numpy(np.tile(np.array([0, 0, 4 * vs, 0, 0, 0, 1, 1], F), (9, 1))).cuda()
    out = torch.full((24,), MARKER, dtype=torch.float32, device="cuda")
    R, O = C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr())
    f4 = lambda *v: (C.c_float * 4)(*v)
    INVALID = 1
    assert lib.vh_cast_rays(h, 8, R, None, O, None, None) == 0
    assert lib.vh_cast_rays(h, 8, R, f4(0, 0, 1, 0), O, None, None) == 0
    assert lib.vh_cast_rays(None, 8, R, None, O, None, None) == INVALID
    assert lib.vh_cast_rays(h, 1 << 31, R, None, O, None, None) == INVALID
    assert lib.vh_cast_rays(h, (1 << 40) + 8, R, None, O, None, None) == INVALID
    assert lib.vh_cast_rays(h, 8, None, None, O, None, None) == INVALID
    assert lib.vh_cast_rays(h, 8, R, None, None, None, None) == INVALID
    assert lib.vh_cast_rays(h, 8, C.c_void_p(rays.data_ptr() + 4), None, O, None, None) == INVALID          # not 16-byte aligned
    for bad in (float("nan"), float("inf"), -float("inf")):
        for i in range(4):
            p = [0.0, 0.0, 1.0, 0.0]
            p[i] = bad
            assert lib.vh_cast_rays(h, 8, R, f4(*p), O, None, None) == INVALID
            assert lib.vh_cast_rays(h, 0, None, f4(*p), None, None, None) == INVALID
    assert lib.vh_cast_rays(h, 0, None, None, None, None, None) == 0                                     # n = 0: nothing launched
    assert lib.vh_cast_rays(h, 0, R, None, O, None, None) == 0
    assert lib.vh_cast_rays_host(None, 8, None, None, None, None, None) == INVALID
    assert lib.vh_cast_rays_host(h, 8, None, None, None, None, None) == INVALID
    assert lib.vh_cast_rays_host(h, 0, None, None, None, None, None) == 0
    gt.synchronize()
    got = out.cpu().numpy()
    # (the last good call into `out` had the plane z = 0: t is the world z of the zero level, 19.5 voxels)
    assert np.array_equal(got[:8].view(U), np.full(8, 19.5 * vs, F).view(U)) and (got[8:] == MARKER).all()
    assert gt.cast_rays(torch.zeros((0, 8), dtype=torch.float32, device="cuda")).shape == (0,)
    # the host form gives the device form's answer
    h_rays = rays.cpu().numpy()
    t, n, v = np.full(9, MARKER, F), np.full(27, MARKER, F), np.full(36, IMARKER, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.vh_cast_rays_host(h, 9, fp(h_rays), None, fp(t), fp(n), v.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert (t == F(15.5 * vs)).all() and (v.reshape(9, 4) == [0, 0, 20, 1]).all() and np.array_equal(n.reshape(9, 3), np.tile(F([0, 0, -1]), (9, 1)))
    gt.close()


# ---- 7. the room: shards, overflow chains, queued frames, purity ---------------------------------------------------------
def room_rays(vh, index=0, t=(0.1, 4.0), size=(64, 48)):
    """A 64 x 48 view of the room from a pose of the loop tests/test_gpu_gc.py fuses from."""
    pose = synth.camera_loop(60)[index]
    W, H = size
    return pose, vh.pinhole_rays(pose, 525.0 * W / 640, 525.0 * W / 640, W / 2, H / 2, W, H, *t)


def test_two_shards(vh, oracle, torch_cuda):
    shards = shard_pair(vh, torch_cuda)
    models = [mm.model_of(sh.table.hash_table(), sh.table.sdf_blocks()) for sh in shards]
    assert not set(models[0]) & set(models[1]) and min(len(m) for m in models) > 100
    pose, rays = room_rays(vh)
    plane = np.asarray(oracle.invert4x4(pose), F).reshape(4, 4)[2]
    hits = []
    for sh, model in zip(shards, models):
        field = rays_ref.Field(model)
        vs = sh.table.params.voxelSize
        want = rays_ref.cast(field, vs, rays)
        assert_same(cast(torch_cuda, sh.table, rays), want, "shard")
        assert_same(cast(torch_cuda, sh.table, rays, plane), rays_ref.cast(field, vs, rays, plane), "shard, plane")
        hits.append(want[1] == 1)
    print(f"hits per shard: {hits[0].mean():.2f} {hits[1].mean():.2f}, in both {(hits[0] & hits[1]).mean():.2f}")
    assert min(h.mean() for h in hits) > 0.05 and (hits[0] != hits[1]).any()
    for sh in shards:
        sh.table.close()


def test_overflow_list_chains(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096, attachedLinkedListSize=8))
    table = gt.hash_table()
    assert (table["offset"] != 0).sum() > 20                         # chains did form
    model = mm.model_of(table, gt.sdf_blocks())
    _, rays = room_rays(vh)
    want = rays_ref.cast(model, gt.params.voxelSize, rays)
    assert_same(cast(torch_cuda, gt, rays), want, "overflow list")
    print(f"hits {(want[1] == 1).mean():.2f}")
    assert (want[1] == 1).mean() > 0.2
    gt.close()


def test_sees_queued_frames_and_changes_nothing(vh, torch_cuda):
    torch = torch_cuda
    plain = fuse(torch, table_of(vh, 1))
    model = mm.model_of(plain.hash_table(), plain.sdf_blocks())
    _, rays = room_rays(vh, 25)                                       # the pose of the last frame
    gt = table_of(vh, 1)
    fr = frames(6)
    keep = [torch.from_numpy(v).cuda() for _, v in fr]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([q for q, _ in fr[:5]], keep[:5])
    gt.integrate(fr[5][0], keep[5])                                  # pipelined: its second half is still pending, no flush
    before = cast(torch, gt, rays)
    gt.flush()
    after = cast(torch, gt, rays)
    want = rays_ref.cast(model, gt.params.voxelSize, rays)
    assert_same(before, want, "with a frame pending")
    assert_same(after, want, "after the flush")
    five = fuse(torch, table_of(vh, 1), 5)                           # without the last frame the answer differs
    assert not rays_ref.same_bits(cast(torch, five, rays)[0], want[0])
    assert (want[1] == 1).mean() > 0.2
    # purity: everything the context holds, before and after
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    cast(torch, gt, rays)
    cast(torch, gt, rays, (0.0, 0.0, 1.0, 0.0))
    assert state(gt) == s0
    for t in (gt, plain, five):
        t.close()


# ---- 8. repeats --------------------------------------------------------------------------------------------------------
def test_the_same_bits_every_time(vh, torch_cuda, contexts):
    case = rc.BY_NAME["noise+z deep"]
    gt = contexts(case, "b")
    rays = case_rays(vh, case)
    first = cast(torch_cuda, gt, rays)
    assert (first[2][:, 3] == 1).mean() > 0.25
    for rep in range(10):
        for a, b in zip(cast(torch_cuda, gt, rays), first):
            assert np.array_equal(a.view(U), b.view(U)), rep


# ---- 9. C++ ------------------------------------------------------------------------------------------------------------
def test_cpp_program_casts_the_rays(vh, oracle, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "rays_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "rays_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    verts = synth.sphere_inside_scene()
    verts.tofile(tmp_path / "verts.bin")
    # the model in Python: common.h defaults, REFERENCE semantics, two frames at the identity pose
    gt = vh.SDFHashtable(vh.default_params(), 640, 480, 0)
    I4 = np.eye(4, dtype=np.float32)
    d = torch_cuda.from_numpy(verts).cuda()
    gt.integrate(I4, d)
    gt.integrate(I4, d)
    # rays towards some 600 vertices of its mesh, from the origin and from a point beside it
    surf = gt.extract_mesh().reshape(-1, 3)
    surf = surf[::max(1, len(surf) // 300)][:300]
    rays = np.zeros((2 * len(surf), 8), F)
    rays[len(surf):, 0:3] = (0.05, -0.03, 0.02)
    rays[:, 4:7] = np.concatenate([surf, surf]) - rays[:, 0:3]
    rays[:, 3], rays[:, 7] = 0.0, 1.5                                # (D reaches the vertex at t = 1)
    plane = np.array([0.0, 0.0, 1.0, 0.0], F)                        # the camera depth of the identity pose
    np.concatenate([rays.reshape(-1), plane]).astype(F).tofile(tmp_path / "rays.bin")
    out = subprocess.run([str(exe), str(tmp_path / "verts.bin"), str(tmp_path / "rays.bin"), str(tmp_path / "out.bin")],
                         check=True, capture_output=True, text=True).stdout
    got = dict(kv.split("=") for kv in out.split())
    assert int(got["rays"]) == len(rays) >= 400
    raw = np.fromfile(tmp_path / "out.bin", U)
    n, at = len(rays), 0
    for k, p in enumerate((None, plane)):
        t, nr, vx = cast(torch_cuda, gt, rays, p)
        for want in (t, nr.reshape(-1)):
            assert rays_ref.same_bits(raw[at:at + want.size].view(F), want)
            at += want.size
        assert np.array_equal(raw[at:at + vx.size].view(np.int32), vx.reshape(-1))
        at += vx.size
        assert int(got[f"hits{k}"]) == int((vx[:, 3] == 1).sum())
        print(f"pass {k}: {got[f'hits{k}']} of {n} rays hit")
    assert at == len(raw) and int(got["hits0"]) > 50
    gt.close()
