"""tests/cpp/components_demo.cpp builds against the headers, runs SDF_Hashtable::components and ::removeComponents on a model
it fuses itself, and writes records, labels and stats equal to the Python calls' on the same model, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_program_labels_and_removes(vh, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "components_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "components_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    verts = synth.sphere_inside_scene()
    verts.tofile(tmp_path / "verts.bin")
    d = torch_cuda.from_numpy(verts).cuda()
    I4 = np.eye(4, dtype=np.float32)
    for target, conn, min_size in ((cr.INSIDE, 14, 8), (cr.OUTSIDE, 6, 3)):
        # the model in Python: common.h defaults, REFERENCE semantics, two frames at the identity pose
        gt = vh.SDFHashtable(vh.default_params(), 640, 480, 0)
        gt.integrate(I4, d)
        gt.integrate(I4, d)
        surf = gt.extract_mesh().reshape(-1, 3)
        assert len(surf) > 100
        dims = [27, 22, 19]
        centre = np.round(surf[len(surf) // 2] / gt.params.voxelSize).astype(np.int64)
        lo = [int(c) - e // 2 for c, e in zip(centre, dims)]
        out = subprocess.run([str(exe), str(tmp_path / "verts.bin"), str(target), str(conn), *map(str, lo), *map(str, dims),
                              str(min_size), str(tmp_path / "out.bin")], check=True, capture_output=True, text=True).stdout
        got = {k: int(v) for k, v in (kv.split("=") for kv in out.split())}
        rec, lab, stats = gt.components(None, target, conn, (lo, dims))
        removed = gt.remove_components(min_size, None, target, conn)
        after, _, _ = gt.components(None, target, conn)
        assert {k: got[k] for k in ("blocks", "nodes", "components", "largest")} == {k: stats[k] for k in ("blocks", "nodes", "components", "largest")}
        assert {k: got[k] for k in removed} == removed and got["after"] == len(after)
        n, voxels = len(rec), int(np.prod(dims))
        raw = np.fromfile(tmp_path / "out.bin", np.uint8)
        assert len(raw) == 16 * n + 4 * voxels + 16 * len(after)
        assert np.array_equal(raw[:16 * n].view(cr.RECORD), rec)
        assert np.array_equal(raw[16 * n:16 * n + 4 * voxels].view(np.uint32), lab.cpu().numpy().view(np.uint32).reshape(-1))
        assert np.array_equal(raw[16 * n + 4 * voxels:].view(cr.RECORD), after)
        labels = lab.cpu().numpy()
        assert stats["nodes"] > 300 and n >= 1 and (labels >= 0).sum() > 50 and (labels == -1).sum() > 50
        print(f"target={target} connectivity={conn}: {out.strip()}")
        gt.close()
