"""SDF_Hashtable::changedBlocks / extractMeshBlocks of the C++ facade (tests/cpp/mesh_blocks_demo.cpp, built here as
tests/test_gpu_stream_cpp.py builds its demo) against the same two calls from Python on a table built the same way: the
listed keys with their flags, in order, and a checksum of every block's triangles and normals."""
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def checksum(pos, nrm):
    words = np.concatenate([pos.reshape(-1), nrm.reshape(-1)]).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((words * (2 * np.arange(len(words), dtype=np.uint64) + 1)).sum(dtype=np.uint64))


def test_cpp_program_lists_and_meshes_what_python_does(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "mesh_blocks_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "mesh_blocks_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    frames = DC.frames(oracle)
    np.stack([f[1] for f in frames]).tofile(tmp_path / "frames.bin")
    np.stack([np.asarray(f[0], F) for f in frames]).tofile(tmp_path / "poses.bin")
    DC.k_inv().astype(F).tofile(tmp_path / "kinv.bin")
    out = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("frames.bin", "poses.bin", "kinv.bin")],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    gt = vh.SDFHashtable(vh.default_params(**DC.KW), DC.W, DC.H, 1)
    state = gt.changes_state()
    line = 0
    for r in (0, 1):
        gt.integrate_depth(frames[r][0], torch.from_numpy(frames[r][1]).cuda(), DC.k_inv())
        changed, removed = gt.changes(state, halo="normals")
        changed = changed.cpu().numpy().copy()
        pos, nrm, first = gt.extract_mesh_blocks(changed, normals=True)
        first = first.astype(np.int64)
        assert out[line] == f"round {r} changed={len(changed)} removed={len(removed)} triangles={len(pos)}", out[line]
        print(out[line], "allocated:", len(gt.allocated()))
        for j, k in enumerate(changed.tolist()):
            a, b = first[j], first[j + 1]
            assert out[line + 1 + j] == f"key {k[0]} {k[1]} {k[2]} {k[3]} {b - a} {checksum(pos[a:b], nrm[a:b])}", (r, j)
        line += 1 + len(changed)
        assert len(changed) > 20 and len(pos) > 100
        if r == 1:
            assert len(changed) <= len(gt.allocated())               # (blocks the second frame and its halo did not reach are not listed)
    assert line == len(out)
    gt.close()
