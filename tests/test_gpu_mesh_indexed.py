"""vh_extract_mesh_indexed on the GPU against the specification (tests/mesh_indexed_ref.py) applied to the GPU's OWN
downloaded table and voxels: both counts, the vertices, their normals and the indices equal as uint32 words and in order,
and vertices[indices] equal to what vh_extract_mesh of the same context writes.  NaN coordinates (from +-inf sdf) are
compared as "NaN in the same places" in the one case that makes them.  Every case asserts V > 0 and T > 0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_indexed_ref as ir
import mesh_models as mm
import mesh_ref
from conftest import blocks_by_pos
from test_gpu_gc import frames
from test_gpu_mesh import ROOT, fuse, shard_pair, table_of
from test_gpu_mesh_crafted import SMALL
from test_mesh_indexed_cpu import BALL_REGION, ball
from voxelhashing_demo_amd import _lib as L
from voxelhashing_demo_amd import dist as vdist
from voxelhashing_demo_amd import mesh_io, synth

pytestmark = pytest.mark.gpu
U = np.uint32


def words_equal(got, want, nan_ok):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    if not nan_ok:
        return np.array_equal(got.view(U), want.view(U))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(U)[~nan], want.view(U)[~nan])


def same_as_specification(gt, region=None, voxels=None, nan_ok=False):
    """Extract first (the call has to see queued frames by itself), then download and compare."""
    v, f, n = gt.extract_mesh_indexed(region, normals=True)
    table = gt.hash_table()
    voxels = gt.sdf_blocks() if voxels is None else voxels
    wv, wf, wn, info = ir.extract_indexed(table, voxels, gt.params.voxelSize, region, normals=True)
    print(f"indexed mesh: vertices={len(wv)} got={len(v)} triangles={len(wf)} got={len(f)}")
    assert gt.mesh_counts(region) == (len(wv), len(wf)) == (len(v), len(f))
    assert len(v) > 0 and len(f) > 0
    assert f.dtype == np.int32 and np.array_equal(f.astype(np.int64), wf)
    assert words_equal(v, wv, nan_ok) and words_equal(n, wn, nan_ok)
    pv, pf = gt.extract_mesh_indexed(region)                            # the pass without normals writes the same
    assert words_equal(pv, wv, nan_ok) and np.array_equal(pf, f)
    tris, nrm = gt.extract_mesh(region, normals=True)                   # and de-indexed it is the triangle list
    assert words_equal(v[f], tris, nan_ok) and words_equal(n[f], nrm, nan_ok)
    return v, f, n, info


def context_with(vh, model, tmp_path, **kw):
    gt = vh.SDFHashtable(vh.default_params(**(kw or SMALL)), 640, 480, 1)
    return mm.load_model(gt, model, tmp_path)


# ---- the fused room ----
def test_room_pinhole(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1))
    v, f, n, _ = same_as_specification(gt)
    assert len(f) > 100000 and len(v) < 0.6 * len(f)
    assert (np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-5).mean() > 0.5
    assert ir.repeated_directed_edges(f) == 0
    gt.close()


def test_room_reference_semantics(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 0))
    same_as_specification(gt)
    gt.close()


def test_band_allocation(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, band=0.1))
    same_as_specification(gt)
    gt.close()


def test_overflow_list_chains(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096,
                                   attachedLinkedListSize=8))
    same_as_specification(gt)
    assert (gt.hash_table()["offset"] != 0).sum() > 20
    gt.close()


def test_sees_queued_pipelined_frames(vh, torch_cuda):
    torch = torch_cuda
    gt = table_of(vh, 1)
    fr = frames(6)
    keep = [torch.from_numpy(v).cuda() for _, v in fr]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([p for p, _ in fr[:5]], keep[:5])
    gt.integrate(fr[5][0], keep[5])                         # pipelined: its second half is still pending, no flush
    v, f, _, _ = same_as_specification(gt)
    plain = fuse(torch, table_of(vh, 1))
    pv, pf = plain.extract_mesh_indexed()
    assert np.array_equal(v[f].view(U), pv[pf].view(U))
    gt.close()
    plain.close()


def test_frame_path_is_untouched(vh, torch_cuda):
    torch = torch_cuda
    a, b = table_of(vh, 1), table_of(vh, 1)
    fr = frames(7)
    for pose, verts in fr[:6]:
        d = torch.from_numpy(verts).cuda()
        a.integrate(pose, d)
        b.integrate(pose, d)
    nv, nt = b.mesh_counts()
    v, f = b.extract_mesh_indexed()
    assert (len(v), len(f)) == (nv, nt) and nv > 0 and nt > 0
    d = torch.from_numpy(fr[6][1]).cuda()
    a.integrate(fr[6][0], d)
    b.integrate(fr[6][0], d)
    ta, tb = a.hash_table(), b.hash_table()
    assert np.array_equal(ta["pos"], tb["pos"]) and np.array_equal(ta["ptr"] != -1, tb["ptr"] != -1)
    assert np.array_equal(ta["offset"], tb["offset"])
    va = blocks_by_pos(ta[ta["ptr"] != -1], a.sdf_blocks())
    vb = blocks_by_pos(tb[tb["ptr"] != -1], b.sdf_blocks())
    assert va.keys() == vb.keys() and len(va) > 1000
    for k in va:
        assert np.array_equal(va[k].view(U), vb[k].view(U)), k
    assert a.counters() == b.counters()
    a.close()
    b.close()


# ---- crafted models ----
@pytest.mark.parametrize("name", ["every_configuration", "wide_magnitudes", "zeros", "subnormals", "weights", "zero_gradient",
                                  "lone_block"])
def test_crafted(vh, torch_cuda, tmp_path, name):
    gt = context_with(vh, getattr(mm, name)(), tmp_path)
    v, f, _, _ = same_as_specification(gt)
    assert ir.repeated_directed_edges(f) == 0
    if name == "zeros":                                    # more vertices by edge than by position: no positional weld
        assert len(v) > len(np.unique(v.view(U), axis=0))
    gt.close()


def test_non_finite(vh, torch_cuda, tmp_path):
    gt = context_with(vh, mm.non_finite(), tmp_path)
    v, _, _, _ = same_as_specification(gt, nan_ok=True)
    assert np.isnan(v).any() and not np.isnan(v).all()
    gt.close()


def test_holes_and_borders(vh, torch_cuda, tmp_path):
    for seed in mm.HOLE_SEEDS:
        gt = context_with(vh, mm.holes(seed), tmp_path)
        same_as_specification(gt)
        gt.close()


def test_keys(vh, torch_cuda, tmp_path):
    gt = context_with(vh, mm.keys_model(), tmp_path)
    v, _, _, _ = same_as_specification(gt)
    assert len(v) > len(np.unique(v.view(U), axis=0))      # rounded coordinates coincide, the vertices stay apart
    for region in mm.KEY_REGIONS:
        same_as_specification(gt, region)
    gt.close()


def test_closed_ball(vh, torch_cuda, tmp_path):
    gt = context_with(vh, ball(), tmp_path, numBuckets=509, bucketSize=8, numVoxelBlocks=256)
    v, f, _, _ = same_as_specification(gt)
    two, euler = ir.closed_manifold(f, len(v))
    assert two and euler == 2 and ir.repeated_directed_edges(f) == 0
    gt.close()


def test_ball_region_uses_vertices_of_other_blocks(vh, torch_cuda, tmp_path):
    gt = context_with(vh, ball(), tmp_path, numBuckets=509, bucketSize=8, numVoxelBlocks=256)
    v, f, _, info = same_as_specification(gt, BALL_REGION)
    lo, hi = np.array(BALL_REGION[0]), np.array(BALL_REGION[1])
    block = info["edge"][:, :3] >> 3
    outside = int((~((block >= lo) & (block < hi)).all(1)).sum())
    # the block of each triangle's cell, from the GPU's own table
    cell_block = mesh_ref.extract(gt.hash_table(), gt.sdf_blocks(), gt.params.voxelSize, BALL_REGION)[2]["block"]
    pairs = np.unique(np.concatenate([f.reshape(-1, 1).astype(np.int64), np.repeat(cell_block, 3, axis=0)], 1), axis=0)
    shared = int((np.bincount(pairs[:, 0], minlength=len(v)) >= 2).sum())
    print(f"vertices={len(v)} anchored outside the region={outside} used from two or more blocks={shared}")
    assert outside == 198 and shared > 600
    gt.close()


# ---- sizes, shards, views ----
def test_workgroups_run_several_passes(vh, torch_cuda, tmp_path):
    model = mm.many_blocks()
    gt = vh.SDFHashtable(vh.default_params(numBuckets=mm.MANY_BUCKETS, bucketSize=mm.MANY_BUCKET_SIZE,
                                           numVoxelBlocks=len(model) + 11), 640, 480, 1)
    mm.load_model(gt, model, tmp_path)
    same_as_specification(gt)
    assert len(model) > 3 * 8192
    gt.close()


def test_more_than_one_tile_of_slices(vh, torch_cuda, tmp_path):
    gt = vh.SDFHashtable(vh.default_params(numBuckets=mm.SLICE_BUCKETS, bucketSize=2, numVoxelBlocks=4096), 640, 480, 1)
    mm.load_model(gt, mm.many_slices(), tmp_path)
    same_as_specification(gt)
    gt.close()


def test_shard_owning_half_the_buckets(vh, torch_cuda):
    shards = shard_pair(vh, torch_cuda)
    for sh in shards:
        lo, hi = sh.table.bucket_range
        assert hi - lo == (1 << 12) // 2
        same_as_specification(sh.table)                    # seam cells emit nothing, and so do their vertices
    assert shards[1].table.bucket_range[0] > 0
    for sh in shards:
        sh.table.close()


def test_view_table(vh, torch_cuda):
    torch = torch_cuda
    model = mm.every_configuration()
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), 640, 480, 1)
    view.import_view(rec, len(model))
    same_as_specification(view, voxels=mm.records_as_voxels(rec.cpu().numpy()))
    view.close()


# ---- capacities and the host entry point ----
def test_capacities(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    gt = context_with(vh, mm.every_configuration(), tmp_path)
    wv, wf, wn, _ = same_as_specification(gt)
    V, T = len(wv), len(wf)
    assert gt.extract_mesh_indexed_into(0, 0, None, None) == (V, T)
    guard = 1024
    pairs = [(1, 1), (V - 1, T - 1), (V, T), (V + 1, T + 1), (V - 1, T + 1), (V + 1, T - 1), (100, T), (V, 0), (0, T)]
    for cv, ct in pairs:
        for with_normals in (False, True):
            pos = torch.full((cv * 3 + guard,), -7.5, dtype=torch.float32, device="cuda")
            nrm = torch.full((cv * 3 + guard,), -7.5, dtype=torch.float32, device="cuda") if with_normals else None
            idx = torch.full((ct * 3 + guard,), -7, dtype=torch.int32, device="cuda")
            assert gt.extract_mesh_indexed_into(cv, ct, pos if cv else None, idx if ct else None, nrm if cv else None) == (V, T)
            nv, nt = min(cv, V), min(ct, T)
            for buf, ref in ((pos, wv), (nrm, wn)):
                if buf is None:
                    continue
                b = buf.cpu().numpy()
                assert np.array_equal(b[:nv * 3].view(U), ref[:nv].reshape(-1).view(U)), (cv, ct, with_normals)
                assert (b[nv * 3:] == -7.5).all(), (cv, ct, with_normals)
            i = idx.cpu().numpy()
            assert np.array_equal(i[:nt * 3], wf[:nt].reshape(-1)) and (i[nt * 3:] == -7).all(), (cv, ct, with_normals)
    gt.close()


def test_host_copy(vh, torch_cuda, tmp_path):
    gt = context_with(vh, mm.every_configuration(), tmp_path)
    wv, wf, wn = gt.extract_mesh_indexed(normals=True)
    V, T = len(wv), len(wf)
    assert V > 0 and T > 0
    lib = L.load()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for cv, ct in ((V // 2, T + 50), (V + 50, T // 2)):
        for with_normals in (False, True):
            pos = np.full(cv * 3 + 64, -7.5, np.float32)
            nrm = np.full(cv * 3 + 64, -7.5, np.float32)
            idx = np.full(ct * 3 + 64, 0xFFFFFFF9, np.uint32)
            nv, nt = C.c_uint64(), C.c_uint64()
            L.check(lib.vh_extract_mesh_indexed_host(gt._h, None, cv, ct, pos.ctypes.data_as(fp),
                                                     nrm.ctypes.data_as(fp) if with_normals else None, idx.ctypes.data_as(up),
                                                     C.byref(nv), C.byref(nt)), "vh_extract_mesh_indexed_host")
            assert (nv.value, nt.value) == (V, T)
            a, b = min(cv, V), min(ct, T)
            assert pos[:a * 3].tobytes() == wv[:a].tobytes() and (pos[a * 3:] == -7.5).all()
            assert idx[:b * 3].tobytes() == wf[:b].tobytes() and (idx[b * 3:] == 0xFFFFFFF9).all()
            if with_normals:
                assert nrm[:a * 3].tobytes() == wn[:a].tobytes() and (nrm[a * 3:] == -7.5).all()
    nv, nt = C.c_uint64(), C.c_uint64()
    L.check(lib.vh_extract_mesh_indexed_host(gt._h, None, 0, 0, None, None, None, C.byref(nv), C.byref(nt)), "count only")
    assert (nv.value, nt.value) == (V, T)
    gt.close()


# ---- the other host layers ----
def test_cpp_program_writes_the_indexed_mesh(vh, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "mesh_indexed_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "mesh_indexed_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    verts = synth.sphere_inside_scene()
    verts.tofile(tmp_path / "verts.bin")
    ply = tmp_path / "out.ply"
    out = subprocess.run([str(exe), str(tmp_path / "verts.bin"), str(ply)], check=True, capture_output=True, text=True).stdout
    got = dict(kv.split("=") for kv in out.split())
    gt = vh.SDFHashtable(vh.default_params(), 640, 480, 0)
    I4 = np.eye(4, dtype=np.float32)
    d = torch_cuda.from_numpy(verts).cuda()
    gt.integrate(I4, d)
    gt.integrate(I4, d)
    wv, wf, wn = gt.extract_mesh_indexed(normals=True)
    assert (int(got["vertices"]), int(got["triangles"])) == (len(wv), len(wf)) and len(wf) > 100
    v, f, n = mesh_io.load_ply(ply)
    assert np.array_equal(v.view(U), wv.view(U)) and np.array_equal(f, wf) and np.array_equal(n.view(U), wn.view(U))
    gt.close()


def test_pipeline_demo_writes_the_indexed_mesh(vh, torch_cuda, tmp_path):
    ply = tmp_path / "demo.ply"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pipeline_demo.py"), "4", "--mesh-indexed", str(ply)],
                         check=True, capture_output=True, text=True, cwd=ROOT).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("mesh indexed:")][-1]
    count = int(line.split("triangles=")[1].split()[0])
    nv = int(line.split("vertices=")[1].split()[0])
    v, f, n = mesh_io.load_ply(ply)
    assert len(f) == count > 1000 and len(v) == nv and f.max() == nv - 1 and n is not None and n.shape == v.shape
    assert ir.repeated_directed_edges(f) == 0
