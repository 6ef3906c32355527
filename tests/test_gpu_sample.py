"""vh_sample_sdf and vh_sample_lattice on the GPU against the specification (tests/sample_ref.py, pinned by
tests/test_sample_cpu.py): sdf, weight and gradient bit for bit (two NaNs count as equal), in both modes, on models the
tests choose themselves (tests/mesh_models.py) and on tables the frame path filled.  Every case asserts, on the reference's
own answer, a condition without which it could pass vacuously."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_indexed_ref
import mesh_models as mm
import sample_ref as sr
from test_gpu_gc import frames
from test_gpu_mesh import fuse, shard_pair, table_of
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
SMALL = dict(numBuckets=509, bucketSize=8, numVoxelBlocks=64)
MODES = (sr.NEAREST, sr.TRILINEAR)
CANARY = -7.5


def context_with(vh, model, tmp_path, **kw):
    gt = vh.SDFHashtable(vh.default_params(**(kw or SMALL)), 640, 480, 1)
    return mm.load_model(gt, model, tmp_path)


def sampled(torch, gt, points, mode):
    out = gt.sample_sdf(torch.from_numpy(np.ascontiguousarray(points, F)).cuda(), mode, weight=True, gradient=True)
    return tuple(t.cpu().numpy() for t in out)


def same_as_reference(torch, gt, model, points, mode):
    """The three outputs against the specification on `model`; returns the specification's."""
    got = sampled(torch, gt, points, mode)
    want = sr.sample(model, points, gt.params.voxelSize, mode)
    for name, g, w in zip(("sdf", "weight", "gradient"), got, want):
        assert sr.same_bits(g, w), f"{name} differs from the specification in {np.count_nonzero(~(np.isnan(g) & np.isnan(w)) & (g.view(U) != w.view(U)))} words (mode {mode})"
    return want


def cell_points(rng, cells, vs):
    """World points inside the cells [K, 3] (global voxel of corner 0), t uniform in [0, 1)."""
    return ((np.asarray(cells, np.float64) + rng.uniform(0, 1, (len(cells), 3))) * float(vs)).astype(F)


def points_in_blocks(rng, keys, n, vs, seam=0.25):
    """n points in the cells of the given blocks; a share `seam` has its cell on the block's last layer on a random axis set."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    local = rng.randint(0, 8, (n, 3))
    last = (rng.uniform(size=(n, 3)) < 0.5) & (rng.uniform(size=(n, 1)) < seam)
    local[last] = 7
    return cell_points(rng, keys[rng.randint(0, len(keys), n)] * 8 + local, vs)


def share(want):
    return float((~np.isnan(want[0])).mean())


# ---- 1. bulk -------------------------------------------------------------------------------------------------------
def test_bulk(vh, torch_cuda, tmp_path):
    model = mm.every_configuration()
    gt = context_with(vh, model, tmp_path)
    p = (np.random.RandomState(7).uniform(-1, 25, (4096, 3)) * 0.02).astype(F)
    for mode in MODES:
        want = same_as_reference(torch_cuda, gt, model, p, mode)
        print(f"mode {mode}: with a sample {share(want):.3f}, gradients {(~np.isnan(want[2]).any(1)).mean():.3f}")
        assert 0.15 <= share(want) <= 0.85                      # expected ~0.59 (trilinear), ~0.77 (nearest)
    gt.close()


# ---- 2. seams ------------------------------------------------------------------------------------------------------
def test_seams(vh, torch_cuda, tmp_path):
    model = mm.uniform_model(mm.cube_keys(-2, 1), seed=31)       # voxels -16 .. 7
    gt = context_with(vh, model, tmp_path)
    rng = np.random.RandomState(32)
    cells = [rng.randint(-18, 9, (1024, 3))]
    for code in range(8):                                        # which axes have i & 7 == 7
        c = rng.randint(-17, 8, (128, 3))
        for a in range(3):
            c[:, a] = np.where(code >> a & 1, (c[:, a] & ~7) | 7, np.where(c[:, a] & 7 == 7, c[:, a] - 1, c[:, a]))
        cells.append(c)
    cells = np.concatenate(cells)
    p = cell_points(rng, cells, 0.02)
    want = same_as_reference(torch_cuda, gt, model, p, sr.TRILINEAR)
    same_as_reference(torch_cuda, gt, model, p, sr.NEAREST)
    i = np.floor((p / F(0.02)).astype(F)).astype(np.int64)
    has = ~np.isnan(want[0])
    code = ((i & 7) == 7) @ np.array([1, 2, 4])
    field = sr.Field(model)
    valid = np.stack([field.voxels(i + [c & 1, (c >> 1) & 1, c >> 2])[0] for c in range(8)], 1)
    valid = valid == valid
    inside = lambda k: ((k >= -2) & (k <= 0)).all(-1)
    blocks_here = np.stack([inside((i + [c & 1, (c >> 1) & 1, c >> 2]) >> 3) for c in range(8)], 1)
    for c in range(8):
        assert (has & (code == c)).sum() >= 10 and (~has & (code == c)).sum() >= 1, c
    negative = (i < 0).all(1)
    plus_absent = inside(i >> 3) & ~blocks_here.all(1)            # corner 0's block is there, a +neighbour is not
    one_dead = blocks_here.all(1) & (valid.sum(1) == 7)
    print(f"points={len(p)} with a sample={has.sum()} negative cells={negative.sum()} +neighbour absent={plus_absent.sum()} "
          f"one dead corner={one_dead.sum()}")
    assert (negative & has).sum() > 100 and plus_absent.sum() > 20 and one_dead.sum() > 20
    assert not has[plus_absent].any() and not has[one_dead].any()
    gt.close()


# ---- 3. values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, lo, hi", [("wide_magnitudes", -1, 25), ("zeros", -9, 9), ("subnormals", -9, 9),
                                          ("non_finite", -9, 9), ("weights", -9, 9)])
def test_values(vh, torch_cuda, tmp_path, name, lo, hi):
    model = getattr(mm, name)()
    gt = context_with(vh, model, tmp_path)
    p = (np.random.RandomState(33).uniform(lo, hi, (512, 3)) * 0.02).astype(F)
    for mode in MODES:
        want = same_as_reference(torch_cuda, gt, model, p, mode)
        assert share(want) >= (0.02 if name == "weights" and mode == sr.TRILINEAR else 0.15), share(want)
        if name == "non_finite":
            fin = ~np.isnan(want[0])
            print(f"mode {mode}: infinite sdf {np.isinf(want[0]).sum()}, gradient NaN beside a sample {np.isnan(want[2][fin]).any(1).sum()}")
    gt.close()


def test_zero_gradient(vh, torch_cuda, tmp_path):
    model = mm.zero_gradient()
    gt = context_with(vh, model, tmp_path)
    g = np.random.RandomState(34).randint(1, 15, (512, 3))       # interior voxels: both neighbours on every axis
    want = same_as_reference(torch_cuda, gt, model, (g.astype(F) * F(0.02)).astype(F), sr.NEAREST)
    assert (want[2] == 0).all() and (np.abs(want[0]) == 1).all()
    gt.close()


# ---- 4. sizes and wave patterns --------------------------------------------------------------------------------------
def test_sizes(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    model = mm.every_configuration()
    gt = context_with(vh, model, tmp_path)
    rng = np.random.RandomState(35)
    big = (rng.uniform(-1, 25, (100003, 3)) * 0.02).astype(F)     # (uniform points are in no order: shuffled as they come)
    field = sr.Field(model)
    for mode in MODES:
        want = sr.sample(field, big, 0.02, mode)
        for n in (1, 63, 64, 65, 257, 100003):
            got = sampled(torch, gt, big[:n], mode)
            for g, w in zip(got, want):
                assert sr.same_bits(g, w[:n]), (mode, n)
        assert 0.15 <= share(want) <= 0.85
    # n = 0: VH_OK, nothing written
    out = torch.full((16,), CANARY, dtype=torch.float32, device="cuda")
    gt.sample_sdf_into(torch.zeros((4, 3), dtype=torch.float32, device="cuda"), out, out, out, sr.TRILINEAR, n=0)
    assert (out.cpu().numpy() == CANARY).all()
    assert gt.sample_sdf(torch.zeros((0, 3), dtype=torch.float32, device="cuda")).shape == (0,)
    # n = 65 inside larger buffers
    guard, n = 256, 65
    for mode in MODES:
        bufs = [torch.full((guard + n * k + guard,), CANARY, dtype=torch.float32, device="cuda") for k in (1, 1, 3)]
        gt.sample_sdf_into(torch.from_numpy(big[:n]).cuda(), bufs[0][guard:guard + n], bufs[1][guard:guard + n],
                           bufs[2][guard:guard + 3 * n], mode)
        want = sr.sample(field, big[:n], 0.02, mode)
        for b, w, k in zip(bufs, want, (1, 1, 3)):
            h = b.cpu().numpy()
            assert (h[:guard] == CANARY).all() and (h[guard + n * k:] == CANARY).all()
            assert sr.same_bits(h[guard:guard + n * k], w.reshape(-1))
    gt.close()


def test_wave_patterns(vh, torch_cuda, tmp_path):
    model = mm.every_configuration()
    gt = context_with(vh, model, tmp_path)
    rng = np.random.RandomState(36)
    one = cell_points(rng, np.array([8, 8, 8]) + rng.randint(0, 7, (64, 3)), 0.02)             # one block, no seam
    one_seam = cell_points(rng, np.array([8, 8, 8]) + rng.randint(5, 8, (64, 3)), 0.02)        # ... its + faces
    two = cell_points(rng, np.where(np.arange(64)[:, None] % 2 == 0, [8, 8, 8], [0, 16, 8]) + rng.randint(0, 8, (64, 3)), 0.02)
    for p in (one, one_seam, two):
        for mode in MODES:
            want = same_as_reference(torch_cuda, gt, model, p, mode)
            assert share(want) >= 0.3
    gt.close()


def test_a_wave_of_64_blocks(vh, torch_cuda, tmp_path):
    model = mm.many_blocks()
    gt = vh.SDFHashtable(vh.default_params(numBuckets=mm.MANY_BUCKETS, bucketSize=mm.MANY_BUCKET_SIZE,
                                           numVoxelBlocks=len(model) + 11), 640, 480, 1)
    mm.load_model(gt, model, tmp_path)
    rng = np.random.RandomState(37)
    keys = np.array(list(model), np.int64)
    keys = keys[rng.permutation(len(keys))[:256]]                 # four waves, every lane another block
    assert len(np.unique(keys[:64], axis=0)) == 64
    p = cell_points(rng, keys * 8 + rng.randint(0, 8, (256, 3)), 0.02)
    field = sr.Field(model)
    for mode in MODES:
        want = same_as_reference(torch_cuda, gt, field, p, mode)
        assert share(want) >= 0.15
    gt.close()


# ---- 5. optional outputs ---------------------------------------------------------------------------------------------
def test_optional_outputs(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    model = mm.every_configuration()
    gt = context_with(vh, model, tmp_path)
    p = torch.from_numpy((np.random.RandomState(38).uniform(-1, 25, (1000, 3)) * 0.02).astype(F)).cuda()
    for mode in MODES:
        sdf, w, g = (t.cpu().numpy() for t in gt.sample_sdf(p, mode, weight=True, gradient=True))
        only = gt.sample_sdf(p, mode).cpu().numpy()
        sw = [t.cpu().numpy() for t in gt.sample_sdf(p, mode, weight=True)]
        sg = [t.cpu().numpy() for t in gt.sample_sdf(p, mode, gradient=True)]
        assert sr.same_bits(only, sdf) and sr.same_bits(sw[0], sdf) and sr.same_bits(sg[0], sdf)
        assert sr.same_bits(sw[1], w) and sr.same_bits(sg[1], g)
        assert not np.isnan(sdf).all()
    gt.close()


# ---- 6. tables -------------------------------------------------------------------------------------------------------
def test_view_table(vh, torch_cuda):
    torch = torch_cuda
    model = mm.every_configuration()
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), 640, 480, 1)
    view.import_view(rec, len(model))
    assert sorted(map(tuple, view.allocated()["pos"].tolist())) == sorted(model)
    p = (np.random.RandomState(39).uniform(-1, 25, (2048, 3)) * 0.02).astype(F)
    for mode in MODES:
        assert share(same_as_reference(torch, view, model, p, mode)) >= 0.15
    lo, dims = (-2, 5, 3), (20, 7, 9)
    sdf, w = (t.cpu().numpy() for t in view.sample_lattice(lo, dims, weight=True))
    want = sr.lattice(model, lo, dims)
    assert sr.same_bits(sdf, want[0]) and sr.same_bits(w, want[1]) and not np.isnan(sdf).all()
    view.close()


def test_two_shards(vh, torch_cuda):
    torch = torch_cuda
    shards = shard_pair(vh, torch)
    models = [mm.model_of(sh.table.hash_table(), sh.table.sdf_blocks()) for sh in shards]
    assert not set(models[0]) & set(models[1]) and min(len(m) for m in models) > 100
    union = sorted(set(models[0]) | set(models[1]))
    rng = np.random.RandomState(40)
    p = points_in_blocks(rng, union, 8192, 0.02, seam=0.5)
    i = np.floor((p / F(0.02)).astype(F)).astype(np.int64)
    owner = np.full((len(p), 8), -1)
    for c in range(8):
        k = (i + [c & 1, (c >> 1) & 1, c >> 2]) >> 3
        owner[:, c] = [0 if tuple(r) in models[0] else 1 if tuple(r) in models[1] else -1 for r in k.tolist()]
    straddle = (owner >= 0).all(1) & (owner.min(1) != owner.max(1))
    print(f"cells that straddle the two shards: {straddle.sum()} of {len(p)}")
    assert straddle.sum() >= 1
    total = 0
    for sh, model in zip(shards, models):
        want = same_as_reference(torch, sh.table, model, p, sr.TRILINEAR)
        same_as_reference(torch, sh.table, model, p, sr.NEAREST)
        assert np.isnan(want[0][straddle]).all()
        total += (~np.isnan(want[0])).sum()
    assert total > 0.15 * len(p)
    for sh in shards:
        sh.table.close()


def test_overflow_list_chains(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096,
                                   attachedLinkedListSize=8))
    table = gt.hash_table()
    assert (table["offset"] != 0).sum() > 20                         # chains did form
    model = mm.model_of(table, gt.sdf_blocks())
    p = points_in_blocks(np.random.RandomState(41), list(model), 8192, gt.params.voxelSize)
    field = sr.Field(model)
    for mode in MODES:
        want = same_as_reference(torch_cuda, gt, field, p, mode)
        print(f"mode {mode}: with a sample {share(want):.3f}")
        assert 0.15 <= share(want) <= 0.85
    gt.close()


# ---- 7. queueing and purity ------------------------------------------------------------------------------------------
def test_sees_queued_frames_and_changes_nothing(vh, torch_cuda):
    torch = torch_cuda
    plain = fuse(torch, table_of(vh, 1))
    model = mm.model_of(plain.hash_table(), plain.sdf_blocks())
    p = points_in_blocks(np.random.RandomState(42), list(model), 8192, plain.params.voxelSize)
    gt = table_of(vh, 1)
    fr = frames(6)
    keep = [torch.from_numpy(v).cuda() for _, v in fr]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([q for q, _ in fr[:5]], keep[:5])
    gt.integrate(fr[5][0], keep[5])                                  # pipelined: its second half is still pending, no flush
    before = {mode: sampled(torch, gt, p, mode) for mode in MODES}
    gt.flush()
    field = sr.Field(model)
    for mode in MODES:
        after = sampled(torch, gt, p, mode)
        want = sr.sample(field, p, gt.params.voxelSize, mode)
        for a, b, w in zip(before[mode], after, want):
            assert sr.same_bits(a, b) and sr.same_bits(a, w)
        assert 0.15 <= share(want) <= 0.85
    # purity: everything the context holds, before and after
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    for mode in MODES:
        sampled(torch, gt, p, mode)
    gt.sample_lattice((-40, -40, 0), (80, 80, 40), weight=True)
    gt.synchronize()
    assert state(gt) == s0
    gt.close()
    plain.close()


# ---- 8. lattice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 5))
def test_lattice_boxes(vh, torch_cuda, tmp_path, seed):
    torch = torch_cuda
    model = mm.holes(seed)                                           # around key (-2, 3, -1): voxels x -24..-1, y 16..39, z -16..7
    gt = context_with(vh, model, tmp_path)
    field = sr.Field(model)
    centre = np.array((-2, 3, -1)) * 8
    boxes = [((-10, 27, -3), (1, 1, 1)), ((-17, 23, -9), (3, 2, 1)), ((-3, 5, -9), (13, 9, 20)),
             (tuple(centre + (-3, 5, -9)), (13, 9, 20)), ((-24, 16, -16), (24, 24, 24)), ((-32, 8, -24), (40, 40, 40))]
    mixed = 0
    for lo, dims in boxes:
        n, guard = int(np.prod(dims)), 512
        bufs = [torch.full((n + 2 * guard,), CANARY, dtype=torch.float32, device="cuda") for _ in range(2)]
        gt.sample_lattice_into(lo, dims, bufs[0][guard:guard + n], bufs[1][guard:guard + n])
        want = sr.lattice(field, lo, dims)
        for b, w in zip(bufs, want):
            h = b.cpu().numpy()
            assert (h[:guard] == CANARY).all() and (h[guard + n:] == CANARY).all(), (lo, dims)
            assert sr.same_bits(h[guard:guard + n], w.reshape(-1)), (lo, dims)
        only = gt.sample_lattice(lo, dims).cpu().numpy()
        assert only.shape == tuple(dims[::-1]) and sr.same_bits(only, want[0])
        nan = np.isnan(want[0])
        mixed += bool(nan.any() and not nan.all())
        # the same voxels through the point call: (lo + ijk) * voxelSize rounds back to the voxel while |g| <= 64
        k, j, i = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
        g = np.stack([i, j, k], -1).reshape(-1, 3) + np.array(lo)
        assert np.abs(g).max() <= 64
        near = gt.sample_sdf(torch.from_numpy((g.astype(F) * F(0.02)).astype(F)).cuda(), sr.NEAREST, weight=True)
        assert sr.same_bits(near[0].cpu().numpy(), want[0].reshape(-1)) and sr.same_bits(near[1].cpu().numpy(), want[1].reshape(-1))
    assert mixed >= 3
    # a zero dimension: nothing happens
    out = torch.full((64,), CANARY, dtype=torch.float32, device="cuda")
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        gt.sample_lattice_into((-24, 16, -16), dims, out, out)
    assert (out.cpu().numpy() == CANARY).all()
    assert gt.sample_lattice((0, 0, 0), (3, 0, 2)).shape == (2, 0, 3)
    gt.close()


# ---- 9. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    gt = context_with(vh, mm.lone_block(), tmp_path)
    lib, h = vh.load(), gt._h
    p = torch.zeros((8, 3), dtype=torch.float32, device="cuda")
    out = torch.full((24,), CANARY, dtype=torch.float32, device="cuda")
    P, O = C.c_void_p(p.data_ptr()), C.c_void_p(out.data_ptr())
    INVALID = 1
    assert lib.vh_sample_sdf(h, 1, 8, P, O, None, None) == 0
    assert lib.vh_sample_sdf(None, 1, 8, P, O, None, None) == INVALID
    assert lib.vh_sample_sdf(h, 1, 1 << 31, P, O, None, None) == INVALID
    assert lib.vh_sample_sdf(h, 1, (1 << 40) + 8, P, O, None, None) == INVALID
    for mode in (2, -1, 7):
        assert lib.vh_sample_sdf(h, mode, 8, P, O, None, None) == INVALID
    assert lib.vh_sample_sdf(h, 1, 8, None, O, None, None) == INVALID
    assert lib.vh_sample_sdf(h, 1, 8, P, None, None, None) == INVALID
    assert lib.vh_sample_sdf(h, 0, 0, None, None, None, None) == 0
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    out.fill_(CANARY)
    assert lib.vh_sample_lattice(h, i3(0, 0, 0), i3(2, 2, 2), O, None) == 0
    assert lib.vh_sample_lattice(h, i3(0, 0, 0), i3(-1, 2, 2), O, None) == INVALID
    assert lib.vh_sample_lattice(h, i3(0, 0, 0), i3(2, 2, -5), O, None) == INVALID
    assert lib.vh_sample_lattice(h, i3(2**31 - 2, 0, 0), i3(2, 1, 1), O, None) == INVALID
    assert lib.vh_sample_lattice(h, i3(0, 2**31 - 1, 0), i3(1, 1, 1), O, None) == INVALID
    assert lib.vh_sample_lattice(h, i3(2**31 - 3, 0, -2**31), i3(2, 1, 1), O, None) == 0      # lo + dims = int32's last
    assert lib.vh_sample_lattice(h, i3(0, 0, 0), i3(2, 2, 2), None, None) == INVALID
    assert lib.vh_sample_lattice(h, None, i3(2, 2, 2), O, None) == INVALID
    assert lib.vh_sample_lattice(h, i3(0, 0, 0), i3(0, 2, 2), None, None) == 0
    gt.synchronize()
    h_out = out.cpu().numpy()
    assert np.isnan(h_out[:8]).all() and (h_out[8:] == CANARY).all()      # the two good lattice calls wrote 8 and 2 absent voxels
    gt.close()


# ---- 10. mesh tie-in -------------------------------------------------------------------------------------------------
def test_mesh_vertices_on_axis_edges_lie_on_the_zero_level(vh, torch_cuda, tmp_path):
    """Trilinear sdf at the vertices of extract_mesh_indexed that lie on axis edges of cells (edge bit set d in {1, 2, 4}):
    bit-equal to the specification, and the specification's values there satisfy |sdf| <= 2^-16 * (|sA| + |sB|), sA and sB the
    two ends of the edge.  The vertex is the zero of the field along its edge, A + t with t = sA / (sA - sB); its voxel
    coordinates are below 64, three roundings of relative 2^-24 (the sum A + t, the product with voxelSize, the quotient by
    it) move u by at most 3 * 2^-18 voxel, and the slope of the field along the edge is |sB - sA| = |sA| + |sB| (the ends
    differ in sign).  On the specification alone (no GPU) the worst ratio |sdf| / bound over this model is 0.275.  A vertex
    whose own cell (corner 0 at floor(u)) has an invalid corner has no trilinear sample, although a neighbouring cell emitted
    it: 110 of the 1284 here; the bound is about the others."""
    model = mm.as_model(*mm.ball_model(mm.cube_keys(0, 3), (11.3, 12.1, 12.6), 8.4, seed=51))
    gt = context_with(vh, model, tmp_path)
    verts, _ = gt.extract_mesh_indexed()
    rverts, _, _, info = mesh_indexed_ref.extract_indexed(gt.hash_table(), gt.sdf_blocks(), gt.params.voxelSize)
    assert np.array_equal(verts.view(U), rverts.view(U))
    edge = info["edge"]
    axis = np.isin(edge[:, 3], (1, 2, 4))
    p, a, d = verts[axis], edge[axis, :3], edge[axis, 3]
    want = same_as_reference(torch_cuda, gt, model, p, sr.TRILINEAR)
    field = sr.Field(model)
    sA, sB = field.voxels(a)[0], field.voxels(a + np.stack([d & 1, (d >> 1) & 1, d >> 2], 1))[0]
    have = ~np.isnan(want[0])
    ratio = np.abs(want[0][have]) / ((np.abs(sA) + np.abs(sB))[have] * 2.0 ** -16)
    print(f"vertices={len(verts)} on axis edges={axis.sum()} with a sample={have.sum()} worst |sdf| / bound={ratio.max():.3f}")
    assert axis.sum() > 1000 and have.mean() > 0.8 and np.abs(a).max() < 64
    assert ratio.max() <= 1.0
    gt.close()


# ---- 11. C++ ---------------------------------------------------------------------------------------------------------
def test_cpp_program_samples_the_model(vh, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "sample_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sample_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    verts = synth.sphere_inside_scene()
    verts.tofile(tmp_path / "verts.bin")
    # the model in Python: common.h defaults, REFERENCE semantics, two frames at the identity pose
    gt = vh.SDFHashtable(vh.default_params(), 640, 480, 0)
    I4 = np.eye(4, dtype=np.float32)
    d = torch_cuda.from_numpy(verts).cuda()
    gt.integrate(I4, d)
    gt.integrate(I4, d)
    # the points: some 400 vertices of its mesh, and the same moved by a third of a voxel
    surf = gt.extract_mesh().reshape(-1, 3)
    surf = surf[::max(1, len(surf) // 400)][:400]
    pts = np.concatenate([surf, surf + F(0.007)]).astype(F)
    pts.tofile(tmp_path / "points.bin")
    out = subprocess.run([str(exe), str(tmp_path / "verts.bin"), str(tmp_path / "points.bin"), str(tmp_path / "out.bin")],
                         check=True, capture_output=True, text=True).stdout
    got = dict(kv.split("=") for kv in out.split())
    assert int(got["points"]) == len(pts) >= 400
    res = np.fromfile(tmp_path / "out.bin", F)
    n, at = len(pts), 0
    for mode in MODES:
        sdf, w, g = sampled(torch_cuda, gt, pts, mode)
        for want in (sdf, w, g.reshape(-1)):
            assert sr.same_bits(res[at:at + len(want)], want)
            at += len(want)
        assert int(got[f"samples{mode}"]) == int((~np.isnan(sdf)).sum())
        print(f"mode {mode}: {got[f'samples{mode}']} of {n} points with a sample")
    assert at == len(res) and int(got["samples0"]) > 50
    gt.close()
