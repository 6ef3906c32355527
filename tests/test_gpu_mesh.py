"""vh_extract_mesh on the GPU against the specification (tests/mesh_ref.py) applied to the GPU's OWN downloaded table and
voxels (which the parity tests pin to the oracle bit for bit): same count, same positions bit for bit and in order, same
normals bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref
from conftest import blocks_by_pos
from test_gpu_gc import VARIANTS, H, W, frames
from voxelhashing_demo_amd import dist as vdist
from voxelhashing_demo_amd import mesh_io, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = dict(numBuckets=4096, bucketSize=5, numVoxelBlocks=8192)
U = np.uint32


def table_of(vh, sem=1, variant=None, band=0.0, overflow=False, **kw):
    gt = vh.SDFHashtable(vh.default_params(**(kw or ROOM)), W, H, sem)
    if variant is not None:
        fused, walk = VARIANTS[variant]
        gt.set_option("fused_frame", fused)
        gt.set_option("flatten_variant", walk)
    if overflow:
        gt.set_option("overflow_list", 1)
    if band:
        gt.set_alloc_band(band)
    return gt


def fuse(torch, gt, n=6):
    for pose, verts in frames(n):
        gt.integrate(pose, torch.from_numpy(verts).cuda())
    return gt


def same_as_reference(gt, region=None, voxels=None, got=None):
    """Extract first (the call has to see queued frames by itself), then download and compare."""
    tris, nrm = gt.extract_mesh(region, normals=True) if got is None else got
    table = gt.hash_table()
    voxels = gt.sdf_blocks() if voxels is None else voxels
    want, wnrm, info = mesh_ref.extract(table, voxels, gt.params.voxelSize, region, normals=True)
    print(f"mesh: blocks={info['blocks']} cells={info['cells']} triangles={len(want)} got={len(tris)}")
    assert len(tris) == len(want) == gt.mesh_count(region)
    assert np.array_equal(tris.view(U), want.view(U))                     # bit for bit and in order
    assert np.array_equal(nrm.view(U), wnrm.view(U))
    plain = gt.extract_mesh(region)
    assert np.array_equal(plain.view(U), want.view(U))                    # the pass without normals writes the same positions
    return want, wnrm, info


def test_room_pinhole(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1))
    want, wnrm, info = same_as_reference(gt)
    assert info["cells"] >= 50000 and info["blocks"] > 1000
    assert (np.abs(np.linalg.norm(wnrm.reshape(-1, 3), axis=1) - 1) < 1e-5).mean() > 0.5      # the normals are not all zero
    gt.close()


def test_room_reference_semantics(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 0))
    _, _, info = same_as_reference(gt)
    assert info["cells"] >= 1000
    gt.close()


def test_band_allocation(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, band=0.1))
    _, _, info = same_as_reference(gt)
    assert info["cells"] >= 50000
    gt.close()


def test_overflow_list_chains(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096,
                                   attachedLinkedListSize=8))
    _, _, info = same_as_reference(gt)
    assert (gt.hash_table()["offset"] != 0).sum() > 20 and info["cells"] > 1000      # chains did form
    gt.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_frame_forms(vh, torch_cuda, variant):
    gt = fuse(torch_cuda, table_of(vh, 1, variant))
    _, _, info = same_as_reference(gt)
    assert info["cells"] >= 50000
    gt.close()


def test_sees_queued_pipelined_frames(vh, torch_cuda):
    torch = torch_cuda
    gt = table_of(vh, 1)
    fr = frames(6)
    keep = [torch.from_numpy(v).cuda() for _, v in fr]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([p for p, _ in fr[:5]], keep[:5])
    gt.integrate(fr[5][0], keep[5])                         # pipelined: its second half is still pending, no flush
    _, _, info = same_as_reference(gt)
    assert info["cells"] >= 50000
    plain = fuse(torch, table_of(vh, 1))
    assert np.array_equal(gt.extract_mesh().view(U), plain.extract_mesh().view(U))
    gt.close()
    plain.close()


def test_after_delete_and_collect(vh, torch_cuda):
    torch = torch_cuda
    gt = fuse(torch, table_of(vh, 1))
    keys = sorted(tuple(k) for k in gt.allocated()["pos"].tolist())
    victims = keys[::3]
    k4 = np.zeros((len(victims), 4), np.int32)
    k4[:, :3] = victims
    gt.delete_blocks(torch.from_numpy(k4).cuda())
    _, _, info = same_as_reference(gt)
    assert info["cells"] > 5000
    gone = set(victims)
    assert not gone & set(map(tuple, info["block"].tolist()))           # no triangle in a deleted block's cells
    gt.garbage_collect(0.01)                                            # (the compact list is empty after a deletion)
    same_as_reference(gt)
    pose, verts = frames(1)[0]
    gt.integrate(pose, torch.from_numpy(verts).cuda())
    gt.garbage_collect(0.01)
    print("freed by the collection:", gt.counters()["last_freed"])
    _, _, info = same_as_reference(gt)
    assert info["cells"] > 1000
    gt.close()


def test_regions_partition_the_model(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1))
    whole = gt.extract_mesh()
    pos = gt.allocated()["pos"]
    lo, hi = pos.min(0), pos.max(0) + 1
    mid = (lo + hi) // 2
    parts, counts = [], []
    for ix in range(2):
        for iy in range(2):
            for iz in range(2):
                sel = (ix, iy, iz)
                rlo = [lo[a] if sel[a] == 0 else mid[a] for a in range(3)]
                rhi = [mid[a] if sel[a] == 0 else hi[a] for a in range(3)]
                part = gt.extract_mesh((rlo, rhi))
                assert len(part) == gt.mesh_count((rlo, rhi))
                counts.append(len(part))
                parts.append(part)
    both = np.concatenate(parts)
    rows = lambda t: sorted(map(bytes, np.ascontiguousarray(t.reshape(-1, 9)).view(U)))
    assert len(both) == len(whole) and rows(both) == rows(whole)
    assert sum(c > 0 for c in counts) >= 4
    same_as_reference(gt, (lo.tolist(), mid.tolist()))
    assert gt.mesh_count(((1000, 1000, 1000), (1010, 1010, 1010))) == 0      # an empty region
    assert gt.mesh_count((hi.tolist(), lo.tolist())) == 0                    # and an inverted one
    gt.close()


def test_capacity_is_respected(vh, torch_cuda):
    torch = torch_cuda
    gt = fuse(torch, table_of(vh, 1))
    count = gt.mesh_count()
    whole, wn = gt.extract_mesh(normals=True)
    assert count == len(whole) > 100000
    assert gt.extract_mesh_into(0, None, None) == count                  # capacity 0 with NULL buffers
    cap, guard = count // 3, 1024                                        # guard band: 4 KB of floats
    for with_normals in (False, True):
        pos = torch.full((cap * 9 + guard,), -7.5, dtype=torch.float32, device="cuda")
        nrm = torch.full((cap * 9 + guard,), -7.5, dtype=torch.float32, device="cuda") if with_normals else None
        assert gt.extract_mesh_into(cap, pos, nrm) == count              # the whole count, although only cap were written
        p = pos.cpu().numpy()
        assert np.array_equal(p[:cap * 9].view(U), whole[:cap].reshape(-1).view(U))      # the first third, in order
        assert (p[cap * 9:] == -7.5).all()
        if with_normals:
            q = nrm.cpu().numpy()
            assert np.array_equal(q[:cap * 9].view(U), wn[:cap].reshape(-1).view(U)) and (q[cap * 9:] == -7.5).all()
    # a capacity beyond the count leaves the rest of the buffer alone
    pos = torch.full(((count + 100) * 9,), -7.5, dtype=torch.float32, device="cuda")
    assert gt.extract_mesh_into(count + 100, pos, None) == count
    assert (pos.cpu().numpy()[count * 9:] == -7.5).all()
    gt.close()


def test_empty_table(vh, torch_cuda):
    gt = table_of(vh, 1)
    assert gt.mesh_count() == 0
    assert gt.extract_mesh().shape == (0, 3, 3)
    v, f = gt.extract_mesh(weld=True)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    gt.close()


def test_reproducible_and_after_snapshot(vh, torch_cuda, tmp_path):
    gt = fuse(torch_cuda, table_of(vh, 1))
    a, an = gt.extract_mesh(normals=True)
    b, bn = gt.extract_mesh(normals=True)
    assert a.tobytes() == b.tobytes() and an.tobytes() == bn.tobytes()
    gt.save_snapshot(tmp_path / "model.snap")
    again = table_of(vh, 1)
    again.load_snapshot(tmp_path / "model.snap")
    want, _, _ = same_as_reference(again)
    assert np.array_equal(np.sort(want.reshape(-1, 9).view(U), axis=0), np.sort(a.reshape(-1, 9).view(U), axis=0))
    # both kernel shapes (9^3 apron in LDS / corners straight from global memory) give the same bytes
    gt.set_option("mesh_variant", 1)
    c, cn = gt.extract_mesh(normals=True)
    assert a.tobytes() == c.tobytes() and an.tobytes() == cn.tobytes()
    gt.close()
    again.close()


def test_welded_mesh_is_a_surface(vh, torch_cuda):
    """The host-side welding of the product's output: every directed edge at most once (2-manifold with boundary where
    the observed volume ends)."""
    gt = fuse(torch_cuda, table_of(vh, 1))
    tris = gt.extract_mesh()
    verts, faces, vn = gt.extract_mesh(normals=True, weld=True)
    assert np.array_equal(verts[faces].view(U), tris.view(U)) and vn.shape == verts.shape
    assert len(verts) < 0.6 * 3 * len(tris)
    good = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]
    directed = np.concatenate([good[:, [0, 1]], good[:, [1, 2]], good[:, [2, 0]]])
    _, counts = np.unique(directed, axis=0, return_counts=True)
    assert counts.max() == 1
    gt.close()


def shard_pair(vh, torch, world=2):
    kw = dict(numBuckets=1 << 12, numVoxelBlocks=3000)
    plan = vdist.ShardPlan(kw["numBuckets"], world)
    shards = [vdist.HipShard(vh.default_params(**kw), W, H, 1, plan, r, W * H) for r in range(world)]
    prims = synth.room_primitives()
    for step in range(3):
        cams = []
        for r in range(world):
            pose = synth.camera_loop(60, phase=vdist.camera_phase(r, world))[(5 * step) % 60]
            cams.append((pose, synth.render_room_verts(pose, W, H, prims).numpy()))
        vdist.loopback_step(shards, [[c[0]] for c in cams], [[torch.from_numpy(c[1]).cuda()] for c in cams])
    return shards


def test_shard_owning_half_the_buckets(vh, torch_cuda):
    shards = shard_pair(vh, torch_cuda)
    total = 0
    for sh in shards:
        lo, hi = sh.table.bucket_range
        assert hi - lo == (1 << 12) // 2
        _, _, info = same_as_reference(sh.table)                       # the shard's table alone: seam cells are missing
        assert info["cells"] > 1000
        total += info["cells"]
    assert total > 5000
    for sh in shards:
        sh.table.close()


def test_view_table(vh, torch_cuda):
    """A view context (vh_import_view): the voxels live in the imported records."""
    torch = torch_cuda
    shards = shard_pair(vh, torch, 1)
    pose = synth.camera_loop(60)[5]
    records, counts = shards[0].export_views([pose], 2048)
    torch.cuda.synchronize()
    n = int(counts.cpu().numpy()[0])
    assert 100 < n <= 2048
    view = vdist.HipViewTable(vh.default_params(numBuckets=1 << 12, numVoxelBlocks=3000), W, H, 1, 1, 2048)
    view.recv[:n] = records[:n]
    torch.cuda.synchronize()
    view.table.import_view(view.recv, n)
    voxels = view.recv.cpu().numpy().reshape(-1).view(np.dtype([("sdf", "<f4"), ("weight", "<f4")]))
    _, _, info = same_as_reference(view.table, voxels=voxels)
    assert info["blocks"] == n and info["cells"] > 1000
    view.table.close()
    shards[0].table.close()


def test_frame_path_is_untouched(vh, torch_cuda):
    torch = torch_cuda
    a, b = table_of(vh, 1), table_of(vh, 1)
    for t in (a, b):
        t.set_option("pipeline", 1)
    for pose, verts in frames(6):
        d = torch.from_numpy(verts).cuda()
        a.integrate(pose, d)
        b.integrate(pose, d)
        assert b.mesh_count() >= 0
    a.flush()
    b.flush()
    # (which heap block an entry received is a race between the frame's workgroups, so ptr values are compared through
    # the voxels they name, as every parity test of the suite does)
    ta, tb = a.hash_table(), b.hash_table()
    assert np.array_equal(ta["pos"], tb["pos"]) and np.array_equal(ta["ptr"] != -1, tb["ptr"] != -1)
    assert np.array_equal(ta["offset"], tb["offset"])
    va = blocks_by_pos(ta[ta["ptr"] != -1], a.sdf_blocks())
    vb = blocks_by_pos(tb[tb["ptr"] != -1], b.sdf_blocks())
    assert va.keys() == vb.keys() and len(va) > 1000
    for k in va:
        assert np.array_equal(va[k].view(U), vb[k].view(U)), k
    assert a.counters() == b.counters()
    assert a.mesh_count() == b.mesh_count()
    a.close()
    b.close()


def test_cpp_program_writes_the_mesh(vh, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "mesh_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "mesh_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    verts = synth.sphere_inside_scene()
    verts.tofile(tmp_path / "verts.bin")
    ply = tmp_path / "out.ply"
    out = subprocess.run([str(exe), str(tmp_path / "verts.bin"), str(ply)], check=True, capture_output=True, text=True).stdout
    got = dict(kv.split("=") for kv in out.split())
    # the same model in Python: common.h defaults, REFERENCE semantics, two frames at the identity pose
    gt = vh.SDFHashtable(vh.default_params(), 640, 480, 0)
    I4 = np.eye(4, dtype=np.float32)
    d = torch_cuda.from_numpy(verts).cuda()
    gt.integrate(I4, d)
    gt.integrate(I4, d)
    count = gt.mesh_count()
    assert int(got["triangles"]) == count > 100
    v, f, n = mesh_io.load_ply(ply)
    assert len(f) == count and len(v) == 3 * count and n is not None
    tris, nrm = gt.extract_mesh(normals=True)
    assert np.array_equal(v[f].view(U), tris.view(U)) and np.array_equal(n[f].view(U), nrm.view(U))
    gt.close()


def test_pipeline_demo_writes_the_mesh(vh, torch_cuda, tmp_path):
    ply = tmp_path / "demo.ply"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pipeline_demo.py"), "4", "--mesh", str(ply)],
                         check=True, capture_output=True, text=True, cwd=ROOT).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("mesh:")][-1]
    count = int(line.split("triangles=")[1].split()[0])
    v, f, n = mesh_io.load_ply(ply)
    assert len(f) == count > 1000 and f.max() == len(v) - 1 and n is not None and n.shape == v.shape
