"""vh_extract_mesh on voxel values the tests choose themselves (tests/mesh_models.py), loaded through a snapshot or imported
as view records: every cell configuration, values at the edges of the rule (zeros, subnormals, non-finite sdf, odd weights),
holes and missing neighbours, keys at the seams and at the ends of the key domain, capacities that clip inside a cell, and
the host-buffer call.  The comparison is the one of tests/test_gpu_mesh.py (same_as_reference: the specification applied
to the arrays the GPU downloaded, equal bit for bit and in order), with both kernel shapes (mesh_variant 0 and 1).  Every
case asserts a condition, on the downloaded arrays, without which it could pass vacuously; tests/test_mesh_models_cpu.py
asserts the same conditions on the specification alone."""
import ctypes as C

import numpy as np
import pytest

import mesh_models as mm
import mesh_ref
from test_gpu_mesh import same_as_reference
from voxelhashing_demo_amd import _lib as L

pytestmark = pytest.mark.gpu
U = np.uint32
SMALL = dict(numBuckets=509, bucketSize=8, numVoxelBlocks=64)
VARIANTS = (0, 1)


def context_with(vh, model, tmp_path, variant, **kw):
    gt = vh.SDFHashtable(vh.default_params(**(kw or SMALL)), 640, 480, 1)
    mm.load_model(gt, model, tmp_path)
    gt.set_option("mesh_variant", variant)
    return gt


def downloaded(gt):
    """The model the context holds, as the facts of mesh_models see it."""
    return mm.model_of(gt.hash_table(), gt.sdf_blocks())


def cells_of(info):
    return set(map(tuple, info["cell"].tolist()))


def same_as_reference_nan(gt):
    """same_as_reference for the one case that is meant to produce NaN coordinates: NaN in the same places, every other
    word bit-equal (the payload and sign of a NaN the hardware makes up are nobody's rule)."""
    tris, nrm = gt.extract_mesh(normals=True)
    want, wnrm, info = mesh_ref.extract(gt.hash_table(), gt.sdf_blocks(), gt.params.voxelSize, None, normals=True)
    print(f"mesh: blocks={info['blocks']} cells={info['cells']} triangles={len(want)} got={len(tris)}")
    assert len(tris) == len(want) == gt.mesh_count()
    plain = gt.extract_mesh()
    for got, ref in ((tris, want), (nrm, wnrm), (plain, want)):
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got.view(U)[~nan], ref.view(U)[~nan])
    return want, wnrm, info


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_configuration(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.every_configuration(), tmp_path, variant)
    want, _, info = same_as_reference(gt)
    census, words = mm.mask_census(downloaded(gt))
    print(f"masks seen={np.count_nonzero(census)} rarest mixed={census[1:255].min()} table words used={len(words)} of 84")
    assert np.count_nonzero(census) == 256 and census[1:255].min() >= 10
    assert words == {(t, m) for t in range(6) for m in range(1, 15)}
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_configuration_in_a_view_table(vh, torch_cuda, tmp_path, variant):
    torch = torch_cuda
    model = mm.every_configuration()
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), 640, 480, 1)
    view.set_option("mesh_variant", variant)
    view.import_view(rec, len(model))
    assert sorted(map(tuple, view.allocated()["pos"].tolist())) == sorted(model)
    _, _, info = same_as_reference(view, voxels=mm.records_as_voxels(rec.cpu().numpy()))
    assert info["blocks"] == 27 and info["cells"] > 9000
    view.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_wide_magnitudes(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.wide_magnitudes(), tmp_path, variant)
    want, _, _ = same_as_reference(gt)
    t = mm.Dense(downloaded(gt)).vertices()["t"]
    print(f"vertices={len(t)} t<1e-6: {(t < 1e-6).mean():.3f} t>1-1e-6: {(t > 1 - 1e-6).mean():.3f}")
    assert len(t) == 3 * len(want) and (t < 1e-6).mean() >= 0.01 and (t > 1 - 1e-6).mean() >= 0.01
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_zeros(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.zeros(), tmp_path, variant)
    tris, _, _ = same_as_reference(gt)
    same = lambda a, b: (tris[:, a].view(U) == tris[:, b].view(U)).all(1)
    two, three = same(0, 1) | same(1, 2) | same(0, 2), same(0, 1) & same(1, 2)
    v = mm.Dense(downloaded(gt)).vertices()
    ends = [int((((v["sA"].view(U) == bits) & (v["sB"] > 0)) | ((v["sB"].view(U) == bits) & (v["sA"] > 0))).sum())
            for bits in (0, 0x80000000)]
    print(f"triangles={len(tris)} two coincident={(two & ~three).sum()} three={three.sum()} edges with +0 / -0 as the inside end={ends}")
    assert (two & ~three).sum() > 0 and three.sum() > 0 and min(ends) > 100
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_subnormals(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.subnormals(), tmp_path, variant)
    want, _, _ = same_as_reference(gt)
    v = mm.Dense(downloaded(gt)).vertices()
    share = (mm.is_subnormal(v["sA"]) | mm.is_subnormal(v["sB"])).mean()
    print(f"vertices={len(v['t'])} on an edge with a subnormal end={share:.3f}")
    assert len(v["t"]) == 3 * len(want) and share >= 0.10
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_non_finite(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.non_finite(), tmp_path, variant)
    want, _, info = same_as_reference_nan(gt)
    d = mm.Dense(downloaded(gt))
    nan_valid = np.isnan(d.sdf) & (d.weight > 0)
    cell = info["cell"] - d.origin + 1
    for i in range(8):
        assert not nan_valid[cell[:, 2] + (i >> 2), cell[:, 1] + ((i >> 1) & 1), cell[:, 0] + (i & 1)].any()
    print(f"NaN sdf with weight 1: {nan_valid.sum()} voxels, inf: {np.isinf(d.sdf).sum()}, triangles with a NaN coordinate="
          f"{np.isnan(want).any((1, 2)).sum()} of {len(want)}")
    assert nan_valid.sum() > 20 and np.isnan(want).any() and not np.isnan(want).all()
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_weights(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.weights(), tmp_path, variant)
    _, _, info = same_as_reference(gt)
    d = mm.Dense(downloaded(gt))
    cells, _ = d.emitting_cells()
    assert set(map(tuple, cells.tolist())) == cells_of(info) and len(cells) > 500
    cell = info["cell"] - d.origin + 1
    seen = set()
    for i in range(8):
        seen |= set(d.weight[cell[:, 2] + (i >> 2), cell[:, 1] + ((i >> 1) & 1), cell[:, 0] + (i & 1)].view(U).tolist())
    print(f"cells={len(cells)} weights at the corners of emitting cells={np.array(sorted(seen), U).view(np.float32).tolist()}")
    assert seen == set(mm.WEIGHTS[[2, 3, 5]].view(U).tolist())
    assert {w for w in d.weight.view(U).ravel().tolist()} >= set(mm.WEIGHTS.view(U).tolist())     # all six kinds were stored
    gt.close()


def test_holes_and_borders(vh, torch_cuda, tmp_path):
    absent, present = set(), set()
    for seed in mm.HOLE_SEEDS:
        have = mm.holes_present(seed)
        present |= have
        absent |= set(mm.NEIGHBOURS) - have
        gt = context_with(vh, mm.holes(seed), tmp_path, seed & 1)
        want, _, _ = same_as_reference(gt)
        d = mm.Dense(downloaded(gt))
        v = d.vertices()
        share = (d.one_sided(v["a"]) | d.one_sided(v["b"])).mean()
        print(f"seed {seed}: variant={seed & 1} blocks={len(have)} one-sided share of the vertices={share:.3f}")
        assert len(v["t"]) == 3 * len(want) and 0.10 <= share <= 0.90
        if seed < 2:                                       # and the other kernel shape on the same table
            gt.set_option("mesh_variant", 1 - (seed & 1))
            same_as_reference(gt)
        gt.close()
    assert present >= set(mm.NEIGHBOURS) and absent == set(mm.NEIGHBOURS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_zero_gradient(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.zero_gradient(), tmp_path, variant)
    _, nrm, _ = same_as_reference(gt)
    got = gt.extract_mesh(normals=True)[1]
    zero = (got.reshape(-1, 3).view(U) << 1 == 0).all(1).mean()
    print(f"share of zero normals={zero:.3f}")
    assert zero >= 0.5 and not np.isnan(got).any()
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_lone_block(vh, torch_cuda, tmp_path, variant):
    model = mm.lone_block()
    (key,) = model
    gt = context_with(vh, model, tmp_path, variant)
    _, _, info = same_as_reference(gt)
    local = info["cell"] - np.array(key) * 8
    print(f"emitting cells={info['cells']} of 343")
    assert local.min() >= 0 and local.max() <= 6 and info["cells"] >= 300
    cells, _ = mm.Dense(downloaded(gt)).emitting_cells()
    assert set(map(tuple, cells.tolist())) == cells_of(info)
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_keys(vh, torch_cuda, tmp_path, variant):
    model = mm.keys_model()
    gt = context_with(vh, model, tmp_path, variant)
    _, _, info = same_as_reference(gt)
    blocks = set(map(tuple, info["block"].tolist()))
    for name, keys in mm.KEY_CLUSTERS.items():
        assert set(keys) <= blocks, name
        lo = np.array(keys).min(0)
        mine = info["cell"][(info["block"] == lo).all(1)] - lo * 8
        assert all((mine[:, axis] == 7).any() for axis in range(3)), name
    for region in mm.KEY_REGIONS:
        _, _, part = same_as_reference(gt, region)
        lo, hi = np.array(region[0]), np.array(region[1])
        assert 0 < part["blocks"] < len(model)
        assert part["blocks"] == sum(bool(((np.array(k) >= lo) & (np.array(k) < hi)).all()) for k in model)
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_capacities(vh, torch_cuda, tmp_path, variant):
    torch = torch_cuda
    gt = context_with(vh, mm.every_configuration(), tmp_path, variant)
    whole, wn, info = same_as_reference(gt)
    count = len(whole)
    first_cell = int((info["cell"] == info["cell"][0]).all(1).sum())
    first_block = int((info["block"] == info["block"][0]).all(1).sum())
    caps = [1, 2, first_cell - 1, first_cell, first_cell + 1, first_block - 1, first_block, first_block + 1, count - 1, count, count + 1]
    print(f"count={count} first cell={first_cell} first block={first_block} capacities={caps}")
    assert len(set(caps)) == len(caps)
    guard = 1024
    for cap in caps:
        for with_normals in (False, True):
            pos = torch.full((cap * 9 + guard,), -7.5, dtype=torch.float32, device="cuda")
            nrm = torch.full((cap * 9 + guard,), -7.5, dtype=torch.float32, device="cuda") if with_normals else None
            assert gt.extract_mesh_into(cap, pos, nrm) == count               # the whole count, whatever was written
            n = min(cap, count)
            for buf, ref in ((pos, whole), (nrm, wn)):
                if buf is None:
                    continue
                b = buf.cpu().numpy()
                assert np.array_equal(b[:n * 9].view(U), ref[:n].reshape(-1).view(U)), (cap, with_normals)
                assert (b[n * 9:] == -7.5).all(), (cap, with_normals)
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_host_copy(vh, torch_cuda, tmp_path, variant):
    gt = context_with(vh, mm.every_configuration(), tmp_path, variant)
    whole, wn = gt.extract_mesh(normals=True)
    count = len(whole)
    lib = L.load()
    fp = C.POINTER(C.c_float)
    for cap in (count // 2, count + 50):
        for with_normals in (False, True):
            pos = np.full(cap * 9 + 64, -7.5, np.float32)
            nrm = np.full(cap * 9 + 64, -7.5, np.float32) if with_normals else None
            n_out = C.c_uint64()
            L.check(lib.vh_extract_mesh_host(gt._h, None, cap, pos.ctypes.data_as(fp), nrm.ctypes.data_as(fp) if with_normals else None,
                                             C.byref(n_out)), "vh_extract_mesh_host")
            n = min(cap, count)
            assert n_out.value == count
            assert pos[:n * 9].tobytes() == whole[:n].tobytes() and (pos[n * 9:] == -7.5).all()
            if with_normals:
                assert nrm[:n * 9].tobytes() == wn[:n].tobytes() and (nrm[n * 9:] == -7.5).all()
    n_out = C.c_uint64()
    L.check(lib.vh_extract_mesh_host(gt._h, None, 0, None, None, C.byref(n_out)), "vh_extract_mesh_host")
    assert n_out.value == count
    gt.close()
