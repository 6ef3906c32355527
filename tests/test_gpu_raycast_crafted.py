"""The DDA raycast on the GPU against tests/raycast_ref.py on the crafted views of tests/raycast_cases.py: exact ties, inactive
axes, many candidates per ray, values at the edges of the rule, crowded and prime-sized tables, a view table, a table after
deletions, ranges that start and end inside blocks, and the cooperative form's fall-backs -- in every form of the kernel
(raycast_beam 2, 1, 0, 3).  tests/test_raycast_ref_cpu.py asserts, on the reference alone, that each view has the property
it is there for (and that the reference gives the oracle's bits).

Found by these views (holes0+x, raycast_beam 1 and 0, pixel u=12 v=29): at t_min the ray sits exactly on a y and on a z voxel
plane; its first voxel floor(G + E t_min) lies past the z plane but before the y plane.  The y crossing enters an allocated
block, the z crossing has the same time and follows it in the merge order, and the per-lane walk, which rebuilt the entry voxel
from the block's near face, put the ray one voxel BEHIND its own first voxel on z (a hit between two voxels the ray never
visits).  The entry voxel now starts from the ray's first voxel where that lies inside the block's slab, as the cooperative
form's did."""
import numpy as np
import pytest

import mesh_models as mm
import raycast_cases as rc

pytestmark = pytest.mark.gpu
MARKER = -7.5

# What makes `long beam` and `two clusters` fall back inside the cooperative launch (more than 256 cells with a set bit in a
# patch's set; a listed block more than 511 blocks from the patch's first) is asserted, from the placed table's bitmap and the
# reference's record, by tests/test_raycast_ref_cpu.py::test_census_forms -- which also says which cases keep narrow boxes.

CELLS = [pytest.param(c, table, beam, id=f"{c.name}-{table}-beam{beam}") for c in rc.CASES for table in c.tables for beam in c.forms]
MARCH = [pytest.param(c, table, id=f"{c.name}-{table}") for c in rc.CASES for table in c.tables
         if c.focal == rc.FOCAL and (table == "b" or c.kinds & {"noise", "zeros", "weights"})]


@pytest.fixture(scope="module")
def refs(oracle):
    memo = {}

    def get(case, table):
        key = (case.name, table == "d")
        if key not in memo:
            memo[key] = rc.reference(case, oracle, rc.reduced(case.model) if table == "d" else None)
        return memo[key]
    return get


@pytest.fixture(scope="module")
def contexts(vh, torch_cuda, tmp_path_factory):
    """One context per (model, table, image size), filled once: (a), (b) through a snapshot, (c) through vh_import_view, (d) a
    snapshot and then vh_delete_blocks of a third of the keys."""
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
            assert sorted(map(tuple, gt.allocated()["pos"].tolist())) == sorted(case.model)
        else:
            gt = vh.SDFHashtable(vh.default_params(numVoxelBlocks=rc.POOL, **kw), case.W, case.H, 1)
            mm.load_model(gt, case.model, tmp_path_factory.mktemp("snap"))
            if table == "d":
                gone = np.zeros((len(rc.deleted_keys(case.model)), 4), np.int32)
                gone[:, :3] = rc.deleted_keys(case.model)
                gt.delete_blocks(torch.from_numpy(gone).cuda())
                gt.synchronize()
                assert sorted(map(tuple, gt.allocated()["pos"].tolist())) == sorted(rc.reduced(case.model))
            if table == "b":         # the crowded table really is: entries in later slots of their buckets
                t = gt.hash_table()
                assert (t["ptr"].reshape(-1, rc.TABLES["b"]["bucketSize"])[:, 1] != -1).any()
        memo[key] = gt
        return gt
    yield get
    for gt in memo.values():
        gt.close()


def render(torch, gt, case, beam, normals=True):
    gt.set_raycast_intrinsics(case.focal, case.focal, case.cx, case.cy)
    gt.set_option("raycast_beam", beam)
    d = torch.full((case.H, case.W), MARKER, dtype=torch.float32, device="cuda")
    n = torch.full((case.H, case.W, 4), MARKER, dtype=torch.float32, device="cuda")
    if normals:
        gt.raycast_normals(case.pose, d, n, *case.t)
    else:
        gt.raycast(case.pose, d, *case.t)
    gt.synchronize()
    return d.cpu().numpy(), n.cpu().numpy()


def explain(case, record, got, want):
    """The first ray that differs, with what the reference knows about it."""
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if not len(bad):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    v, u = bad[0][:2]
    facts = {k: (a[v, u].tolist() if hasattr(a[v, u], "tolist") else a[v, u]) for k, a in record.items()}
    return f"{case.name}: {len(bad)} words differ; first at pixel (u={u}, v={v}): got {got[v, u]}, want {want[v, u]}; the ray: {facts}"


@pytest.mark.parametrize("case,table,beam", CELLS)
def test_crafted_view(vh, torch_cuda, contexts, refs, case, table, beam):
    depth, normals, record = refs(case, table)
    gt = contexts(case, table)
    d, n = render(torch_cuda, gt, case, beam)
    assert rc.same_image(d, depth, case.nan), explain(case, record, d, depth)
    assert rc.same_image(n, normals, case.nan), explain(case, record, n, normals)
    d, _ = render(torch_cuda, gt, case, beam, normals=False)                   # the kernel without the normal output
    assert rc.same_image(d, depth, case.nan), explain(case, record, d, depth)


@pytest.mark.parametrize("case,table", MARCH)
def test_fixed_step_march(oracle, vh, torch_cuda, contexts, case, table):
    """The fixed-step march shares lookup_block and the hit test with the DDA: against its own oracle, vho_raycast."""
    model = rc.reduced(case.model) if table == "d" else case.model
    ot = oracle.OracleTable(oracle.default_params(voxelSize=rc.VS, **rc.TABLES["a"]), case.W, case.H, 1)
    ot.set_raycast_intrinsics(case.focal, case.focal, case.cx, case.cy)
    assert ot.import_view(mm.view_records(model)) == 0
    ot.set_raycast_mode(oracle.RAYCAST_FIXED_STEP)
    want = ot.raycast(case.pose, *case.t)
    gt = contexts(case, table)
    gt.set_raycast_mode(vh.RAYCAST_FIXED_STEP)
    try:
        got, _ = render(torch_cuda, gt, case, 3, normals=False)
    finally:
        gt.set_raycast_mode(vh.RAYCAST_DDA)
    assert (want != 0).mean() >= 0.25
    assert rc.same_image(got, want, case.nan)
    ot.close()


def test_the_same_bits_every_time(vh, torch_cuda, contexts, refs):
    """Who walks which listed block is a race by design; the image is not: the noise view 20 times in the default form."""
    case = rc.BY_NAME["noise+z"]
    depth, normals, record = refs(case, "a")
    gt = contexts(case, "a")
    for rep in range(20):
        d, n = render(torch_cuda, gt, case, 3)
        assert rc.same_image(d, depth, False) and rc.same_image(n, normals, False), rep
