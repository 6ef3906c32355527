"""vh_extract_mesh_blocks: the triangles of a list of blocks, block by block, against vh_extract_mesh of the one-block regions
and of the whole model, bit for bit -- on a sphere, a tilted plane and a two-block model with the sheet on the seam, with both
kernel shapes (mesh_variant 0 and 1), for absent and repeated keys, an empty list, a clipped capacity, a shard and a view
table."""
import ctypes as C

import numpy as np
import pytest

import mesh_models as mm

pytestmark = pytest.mark.gpu
U = np.uint32
F = np.float32
KW = dict(numBuckets=256, bucketSize=8, numVoxelBlocks=128)
VARIANTS = (0, 1)


def field_model(keys, fn, seed, dead=0.01):
    """sdf = fn(global voxel coordinates [N, 3]) + a little noise, sampled in the given blocks."""
    rng = np.random.RandomState(seed)
    i = np.arange(512)
    local = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    model = {}
    for k in keys:
        p = (np.array(k) * 8 + local).astype(np.float64)
        sdf = (fn(p) + rng.uniform(-0.05, 0.05, 512)).astype(F)
        model[k] = (sdf, np.where(rng.uniform(size=512) < dead, 0, 1).astype(F))
    return model


def sphere():
    return mm.as_model(*mm.ball_model(mm.cube_keys(-2, 2), (0.3, -0.4, 1.1), 11.3, seed=31))


def tilted_plane():
    n = np.array([0.31, 0.52, 0.795])
    return field_model(mm.cube_keys(-1, 2), lambda p: p @ n - 6.2, seed=32)


def seam_sheet():
    """Two blocks, the sheet between voxel x = 7 of the first and voxel x = 0 of the second: every triangle belongs to cells
    of block (0, 0, 0) whose +x corners are block (1, 0, 0)'s."""
    return field_model([(0, 0, 0), (1, 0, 0)], lambda p: p[:, 0] - 7.5, seed=33, dead=0.0)


MODELS = {"sphere": sphere, "tilted plane": tilted_plane, "seam": seam_sheet}


def chunk_of(model):
    keys, vox = mm.model_arrays(model)
    return {"keys": keys.astype(np.int32), "voxels": vox, "colors": None}


def table_with(vh, model, variant, bucket_range=None, **kw):
    gt = vh.SDFHashtable(vh.default_params(**dict(KW, **kw)), 64, 48, 1, bucket_range=bucket_range)
    gt.set_option("mesh_variant", variant)
    st = gt.stream_in(chunk_of(model))
    assert st["unplaced"] == 0 and st["placed"] + st["foreign"] == len(model)
    return gt


def region_of(k):
    return (tuple(int(c) for c in k), tuple(int(c) + 1 for c in k))


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


def check_blocks(gt, keys):
    """Every key's range against the one-block region's extraction; returns (positions, normals, first)."""
    pos, nrm, first = gt.extract_mesh_blocks(np.asarray(keys, np.int32), normals=True)
    plain, none, first2 = gt.extract_mesh_blocks(np.asarray(keys, np.int32))
    assert none is None and same(plain, pos) and np.array_equal(first, first2)
    assert first.dtype == np.uint64 and len(first) == len(keys) + 1 and first[0] == 0 and first[-1] == len(pos)
    counts = []
    for j, k in enumerate(keys):
        want, wn = gt.extract_mesh(region_of(k), normals=True)
        a, b = int(first[j]), int(first[j + 1])
        assert same(pos[a:b], want) and same(nrm[a:b], wn), k
        counts.append(len(want))
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))      # d_first = the prefix sums
    return pos, nrm, first


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_block_and_the_whole_model(vh, torch_cuda, name, variant):
    model = MODELS[name]()
    gt = table_with(vh, model, variant)
    keys = gt.allocated()["pos"].tolist()                  # the ordered block list: ascending entry index
    assert sorted(map(tuple, keys)) == sorted(model)
    pos, nrm, first = check_blocks(gt, keys)
    whole, wn = gt.extract_mesh(normals=True)
    assert len(whole) > 100 and same(pos, whole) and same(nrm, wn)
    emitting = int((np.diff(first.astype(np.int64)) > 0).sum())
    print(f"{name}: blocks={len(keys)} emitting={emitting} triangles={len(whole)}")
    assert 0 < emitting and (name == "seam" or emitting < len(keys))      # empty ranges between full ones
    if name == "seam":
        per_key = dict(zip(map(tuple, keys), np.diff(first.astype(np.int64)).tolist()))
        assert per_key == {(0, 0, 0): len(whole), (1, 0, 0): 0}          # the cells at x = 7 are the first block's
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_absent_and_repeated_keys_and_the_fourth_word(vh, torch_cuda, variant):
    torch = torch_cuda
    gt = table_with(vh, tilted_plane(), variant)
    held = gt.allocated()["pos"].tolist()
    k = [tuple(x) for x in held if gt.mesh_count(region_of(x)) > 0][:2]
    absent = [(50, 50, 50), (-1, -1, -9)]
    keys = [absent[0], k[0], k[1], k[0], absent[1], k[0], absent[0]]
    pos, _, first = check_blocks(gt, keys)
    n = np.diff(first.astype(np.int64))
    assert n[0] == n[4] == n[6] == 0 and n[1] == n[3] == n[5] > 0 and n[2] > 0
    assert same(pos[first[1]:first[2]], pos[first[3]:first[4]])
    # the 4th word of a key is ignored: a flags word of vh_changes, or anything
    k4 = np.zeros((len(keys), 4), np.int32)
    k4[:, :3], k4[:, 3] = keys, [3, -1, 2, 1 << 30, 7, 0, -5]
    again, _, first4 = gt.extract_mesh_blocks(torch.from_numpy(k4).cuda())
    assert same(again, pos) and np.array_equal(first4, first)
    # only absent keys
    none, _, f0 = gt.extract_mesh_blocks(np.array(absent, np.int32))
    assert len(none) == 0 and f0.tolist() == [0, 0, 0]
    gt.close()


def test_empty_list_and_argument_errors(vh, torch_cuda):
    torch = torch_cuda
    gt = table_with(vh, seam_sheet(), 0)
    lib, n = gt._lib, C.c_uint64(77)
    assert lib.vh_extract_mesh_blocks(gt._h, 0, None, 0, None, None, None, C.byref(n)) == 0 and n.value == 0
    pos, nrm, first = gt.extract_mesh_blocks(np.zeros((0, 3), np.int32), normals=True)
    assert pos.shape == (0, 3, 3) and nrm.shape == (0, 3, 3) and first.tolist() == [0]
    keys = torch.zeros((129, 4), dtype=torch.int32, device="cuda")
    assert lib.vh_extract_mesh_blocks(gt._h, 128, keys.data_ptr(), 0, None, None, None, C.byref(n)) == 0
    assert lib.vh_extract_mesh_blocks(gt._h, 129, keys.data_ptr(), 0, None, None, None, C.byref(n)) == 1      # more than the pool holds
    assert lib.vh_extract_mesh_blocks(gt._h, 1, None, 0, None, None, None, C.byref(n)) == 1
    assert lib.vh_extract_mesh_blocks(gt._h, 1, keys.data_ptr(), 5, None, None, None, C.byref(n)) == 1
    assert lib.vh_extract_mesh_blocks(gt._h, 1, keys.data_ptr(), 0, None, None, None, None) == 1
    assert lib.vh_extract_mesh_blocks(None, 1, keys.data_ptr(), 0, None, None, None, C.byref(n)) == 1
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_clipping_writes_nothing_past_the_capacity(vh, torch_cuda, variant):
    torch = torch_cuda
    gt = table_with(vh, sphere(), variant)
    keys = np.zeros((len(gt.allocated()), 4), np.int32)
    keys[:, :3] = gt.allocated()["pos"]
    dk = torch.from_numpy(keys).cuda()
    whole, wn = gt.extract_mesh(normals=True)
    total = len(whole)
    full_first = gt.extract_mesh_blocks(dk)[2]
    inside = int(full_first[np.nonzero(np.diff(full_first.astype(np.int64)) > 2)[0][3]]) + 2      # clips inside a block's range
    for cap in (1, inside, total - 1):
        guard = 0x7FC0DEAD
        pos = torch.full((total + 8, 9), guard, dtype=torch.int32, device="cuda")
        nrm = torch.full((total + 8, 9), guard, dtype=torch.int32, device="cuda")
        first = torch.zeros((len(keys) + 1,), dtype=torch.int64, device="cuda")
        assert gt.extract_mesh_blocks_into(dk, cap, pos, nrm, first) == total
        p, q = pos.cpu().numpy(), nrm.cpu().numpy()
        assert (p[cap:] == guard).all() and (q[cap:] == guard).all()
        assert np.array_equal(p[:cap].view(U), whole.reshape(-1, 9)[:cap].view(U))
        assert np.array_equal(q[:cap].view(U), wn.reshape(-1, 9)[:cap].view(U))
        assert np.array_equal(first.cpu().numpy().view(np.uint64), full_first)      # always the unclipped offsets
    gt.close()


def test_host_form(vh, torch_cuda):
    gt = table_with(vh, tilted_plane(), 0)
    keys = np.zeros((len(gt.allocated()) + 1, 4), np.int32)
    keys[:-1, :3], keys[-1, :3] = gt.allocated()["pos"], (99, 0, 0)
    pos, nrm, first = gt.extract_mesh_blocks(keys, normals=True)
    n = C.c_uint64()
    hp, hn, hf = np.zeros_like(pos), np.zeros_like(nrm), np.zeros(len(keys) + 1, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert gt._lib.vh_extract_mesh_blocks_host(gt._h, len(keys), vp(keys), len(pos), vp(hp), vp(hn), vp(hf), C.byref(n)) == 0
    assert n.value == len(pos) and same(hp, pos) and same(hn, nrm) and np.array_equal(hf, first)
    gt.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_shard_and_a_view_table(vh, torch_cuda, variant):
    torch = torch_cuda
    model = sphere()
    shard = table_with(vh, model, variant, bucket_range=(0, 128))
    keys = shard.allocated()["pos"].tolist()
    assert 0 < len(keys) < len(model)                                    # the other keys hash to the other shard
    pos, _, _ = check_blocks(shard, keys + [k for k in sorted(model) if list(k) not in keys][:3])
    assert same(pos, shard.extract_mesh()) and len(pos) > 0
    shard.close()
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=256, bucketSize=8, numVoxelBlocks=1), 64, 48, 1)
    view.set_option("mesh_variant", variant)
    view.import_view(rec, len(model))
    keys = view.allocated()["pos"].tolist()
    assert len(keys) == len(model)
    pos, nrm, _ = check_blocks(view, keys)
    whole, wn = view.extract_mesh(normals=True)
    assert same(pos, whole) and same(nrm, wn) and len(whole) > 100
    view.close()
