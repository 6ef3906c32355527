"""vh_extract_mesh at the sizes that reach the paths a small room never does: workgroups of mesh_block_kernel that run
several passes (more than 8 192 listed blocks), more than one tile of slice counts (more than 2^20 buckets), more than 256
tiles of block counts (the carry of block_scan_totals_kernel from one round to the next), and a view context whose record
count grows and shrinks between extractions.  Models: tests/mesh_models.py; comparison: same_as_reference of
tests/test_gpu_mesh.py (bit for bit, in order).  tests/test_mesh_models_cpu.py checks the models' conditions without a GPU."""
import numpy as np
import pytest

import mesh_models as mm
import mesh_ref
from test_gpu_mesh import same_as_reference

pytestmark = pytest.mark.gpu
U = np.uint32
GRID, TILE, SLICE = 8192, 1024, 1024          # mesh_block_kernel's grid limit, kScanTile, kListSliceBuckets


def emitting_positions(table, info):
    """Positions in the block list (allocated entries in table order) of the blocks that emitted a triangle."""
    listed = table[table["ptr"] != -1]
    index = {tuple(p): i for i, p in enumerate(listed["pos"].tolist())}
    return np.array(sorted(index[b] for b in set(map(tuple, info["block"].tolist())))), len(listed)


def test_workgroups_run_several_passes(vh, torch_cuda, tmp_path):
    model = mm.many_blocks()
    gt = vh.SDFHashtable(vh.default_params(numBuckets=mm.MANY_BUCKETS, bucketSize=mm.MANY_BUCKET_SIZE,
                                           numVoxelBlocks=len(model) + 11), 640, 480, 1)
    mm.load_model(gt, model, tmp_path)
    for variant in (0, 1):
        gt.set_option("mesh_variant", variant)
        _, _, info = same_as_reference(gt)            # with normals, and the pass without
    at, listed = emitting_positions(gt.hash_table(), info)
    emits = np.zeros(listed, bool)
    emits[at] = True
    passes = -(-listed // GRID)
    print(f"blocks listed={listed} grid={GRID} passes per workgroup={passes - 1} and {passes} (the first {listed - (passes - 1) * GRID} "
          f"workgroups) emitting blocks={len(at)} runs of emitting / silent blocks={np.count_nonzero(emits[1:] != emits[:-1]) + 1}")
    assert listed == mm.MANY_BLOCKS > 3 * GRID and passes == 4
    for lo in range(0, listed, GRID):                 # every pass has blocks that emit and blocks that do not
        assert emits[lo:lo + GRID].any() and not emits[lo:lo + GRID].all()
    # one workgroup's consecutive passes: silent after emitting and emitting after silent both occur
    col = emits[:(passes - 1) * GRID].reshape(passes - 1, GRID)
    assert (col[:-1] & ~col[1:]).any() and (~col[:-1] & col[1:]).any()
    gt.close()


def test_more_than_one_tile_of_slices(vh, torch_cuda, tmp_path):
    model = mm.many_slices()
    gt = vh.SDFHashtable(vh.default_params(numBuckets=mm.SLICE_BUCKETS, bucketSize=2, numVoxelBlocks=4096), 640, 480, 1)
    mm.load_model(gt, model, tmp_path)
    for variant in (0, 1):
        gt.set_option("mesh_variant", variant)
        _, _, info = same_as_reference(gt)
    table = gt.hash_table()
    bucket = np.nonzero(table["ptr"] != -1)[0] // 2
    where = dict(zip(map(tuple, table["pos"][table["ptr"] != -1].tolist()), bucket.tolist()))
    emitting = np.array(sorted({where[b] for b in set(map(tuple, info["block"].tolist()))}))
    slices = mm.SLICE_BUCKETS // SLICE
    tiles = np.bincount(emitting // SLICE // TILE, minlength=2)
    print(f"buckets={mm.SLICE_BUCKETS} slices={slices} slice tiles={-(-slices // TILE)} blocks={len(bucket)} "
          f"emitting blocks per slice tile={tiles.tolist()} entries in the last slice={(bucket // SLICE == slices - 1).sum()} "
          f"in the last bucket={(bucket == mm.SLICE_BUCKETS - 1).sum()}")
    assert slices == 2 * TILE and tiles.min() > 500
    assert (bucket == mm.SLICE_BUCKETS - 1).sum() == 2 and emitting.max() == mm.SLICE_BUCKETS - 1 and (bucket == 0).any()
    gt.close()


def test_more_than_256_tiles_of_block_counts(vh, torch_cuda):
    """A view context over records made on the device: isolated blocks, so the specification may be applied to chunks of the
    downloaded table in entry order and the results concatenated."""
    torch = torch_cuda
    keys, emit = mm.many_tiles_plan()
    n = len(keys)
    rec = torch.zeros((n, mm.RECORD_BYTES), dtype=torch.uint8, device="cuda")
    header = torch.zeros((n, 4), dtype=torch.int32)
    header[:, :3] = torch.from_numpy(keys)
    rec[:, :16] = header.cuda().view(torch.uint8).reshape(n, 16)
    gen = torch.Generator(device="cuda").manual_seed(31)
    vox = torch.empty((int(emit.sum()), 512, 2), dtype=torch.float32, device="cuda")
    x = (torch.arange(512, device="cuda") & 7).float()
    vox[:, :, 0] = x[None, :] - 3.4 + (torch.rand((len(vox), 512), generator=gen, device="cuda") - 0.5) * 0.4
    vox[:, :, 1] = 1.0
    rec[torch.from_numpy(np.nonzero(emit)[0]).cuda(), 16:] = vox.view(torch.uint8).reshape(len(vox), 4096)
    view = vh.SDFHashtable(vh.default_params(numBuckets=mm.TILE_BUCKETS, bucketSize=mm.TILE_BUCKET_SIZE, numVoxelBlocks=1),
                           640, 480, 1)
    view.import_view(rec, n)
    assert view.counters()["bin_overflow"] == 0
    got = {}
    for variant in (0, 1):
        view.set_option("mesh_variant", variant)
        got[variant] = view.extract_mesh(normals=True)
    plain = view.extract_mesh()
    count = view.mesh_count()
    table = view.hash_table()
    voxels = mm.records_as_voxels(rec.cpu().numpy())
    used = np.nonzero(table["ptr"] != -1)[0]
    assert len(used) == n
    pos = table["pos"][used].astype(np.int64)
    assert (pos % 3 == 0).all() and len(np.unique(pos, axis=0)) == n       # isolated: the keys lie on the lattice of multiples of 3
    want, wnrm, at = [], [], []
    for lo in range(0, n, 16 * TILE):                                       # chunks of the table in entry order
        sel = used[lo:lo + 16 * TILE]
        chunk = table[sel[0]:sel[-1] + 1]
        t, q, info = mesh_ref.extract(chunk, voxels, view.params.voxelSize, None, normals=True)
        want.append(t)
        wnrm.append(q)
        first = {tuple(p): lo + i for i, p in enumerate(table["pos"][sel].tolist())}
        at += [first[b] for b in set(map(tuple, info["block"].tolist()))]
    want, wnrm, at = np.concatenate(want), np.concatenate(wnrm), np.array(sorted(at))
    tiles = np.unique(at // TILE)
    print(f"blocks listed={n} block tiles={-(-n // TILE)} rounds of the second level={-(-(-(-n // TILE)) // 256)} emitting blocks={len(at)} "
          f"tiles with an emitting block={len(tiles)} triangles={len(want)}")
    assert n > 256 * TILE and set(mm.TILES_WITH_SURFACE) <= set(tiles.tolist()) and tiles.max() == (n - 1) // TILE >= 257
    assert len(want) == count > 100000
    for v, (tris, nrm) in got.items():
        assert np.array_equal(tris.view(U), want.view(U)), v
        assert np.array_equal(nrm.view(U), wnrm.view(U)), v
    assert np.array_equal(plain.view(U), want.view(U))
    view.close()


def test_view_context_grows_and_shrinks(vh, torch_cuda):
    torch = torch_cuda
    view = vh.SDFHashtable(vh.default_params(numBuckets=mm.VIEW_STEP_BUCKETS, bucketSize=mm.VIEW_STEP_BUCKET_SIZE,
                                             numVoxelBlocks=1), 640, 480, 1)
    cells = []
    for step, model in enumerate(mm.view_steps()):
        rec = torch.from_numpy(mm.view_records(model)).cuda()
        view.import_view(rec, len(model))
        assert view.counters()["bin_overflow"] == 0
        view.set_option("mesh_variant", step & 1)
        _, _, info = same_as_reference(view, voxels=mm.records_as_voxels(rec.cpu().numpy()))
        assert info["blocks"] == len(model) and info["cells"] > 100
        assert sorted(map(tuple, view.allocated()["pos"].tolist())) == sorted(model)
        cells.append(info["cells"])
    print(f"records per import={[len(m) for m in mm.view_steps()]} emitting cells={cells}")
    view.close()
