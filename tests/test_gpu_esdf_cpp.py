"""tests/cpp/esdf_demo.cpp builds against the headers, runs SDF_Hashtable::esdfLattice on a model it fuses itself, and writes
values equal to the Python call's on the same model, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import esdf_ref as er
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_program_computes_the_esdf(vh, torch_cuda, tmp_path):
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "esdf_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "esdf_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    verts = synth.sphere_inside_scene()
    verts.tofile(tmp_path / "verts.bin")
    # the model in Python: common.h defaults, REFERENCE semantics, two frames at the identity pose
    gt = vh.SDFHashtable(vh.default_params(), 640, 480, 0)
    I4 = np.eye(4, dtype=np.float32)
    d = torch_cuda.from_numpy(verts).cuda()
    gt.integrate(I4, d)
    gt.integrate(I4, d)
    # a box around a vertex of the model's mesh: the surface passes through it
    surf = gt.extract_mesh().reshape(-1, 3)
    assert len(surf) > 100
    dims, radius = [27, 22, 19], 6
    centre = np.round(surf[len(surf) // 2] / gt.params.voxelSize).astype(np.int64)
    lo = [int(c) - d // 2 for c, d in zip(centre, dims)]
    for unknown in (er.KEEP, er.FREE):
        out = subprocess.run([str(exe), str(tmp_path / "verts.bin"), *map(str, lo), *map(str, dims), str(radius), str(unknown),
                              str(tmp_path / "out.bin")], check=True, capture_output=True, text=True).stdout
        got = dict(kv.split("=") for kv in out.split())
        n = int(np.prod(dims))
        assert int(got["voxels"]) == n
        raw = np.fromfile(tmp_path / "out.bin", np.int32)
        assert len(raw) == 2 * n
        dist, d2 = (t.cpu().numpy() for t in gt.esdf_lattice(lo, dims, radius, unknown, distance=True, dist2=True))
        assert np.array_equal(raw[:n], d2.reshape(-1))
        assert er.same_bits(raw[n:].view(np.float32), dist.reshape(-1))
        near = (d2 != er.NONE) & (np.abs(d2.astype(np.int64)) < er.FAR)
        assert int(got["near"]) == int(near.sum()) > 50 and int(got["none"]) == int((d2 == er.NONE).sum())
        print(f"unknown={unknown}: {out.strip()}")
    gt.close()
