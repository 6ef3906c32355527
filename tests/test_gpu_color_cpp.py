"""SDF_Hashtable::integrateColor / sampleColor of the C++ facade (tests/cpp/color_demo.cpp, built here as
tests/test_gpu_merge_cpp.py builds its demo) against the same calls from Python on a table built the same way: the sampled
colours in both modes, and a checksum of every block's colour words per key."""
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
BAND, WEIGHT_MAX = 0.12, 2


def image(i):
    return np.random.default_rng(100 + i).integers(0, 1 << 32, (DC.H, DC.W), dtype=np.uint64).astype(U)


def test_cpp_program_colours_as_python_does(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "color_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "color_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    frames = DC.frames(oracle)
    # the same in Python first (the projection is the one vh_create installs, as in the program): it says where colour is
    gt = vh.SDFHashtable(vh.default_params(**DC.KW), DC.W, DC.H, 1)
    for i, (pose, d16, _) in enumerate(frames):
        gt.integrate_depth_color(pose, torch.from_numpy(d16).cuda(), DC.k_inv(), torch.from_numpy(image(i)).cuda(), BAND, WEIGHT_MAX)
    gt.synchronize()
    tab, col = gt.allocated(), gt.color_volume()
    odd = 2 * np.arange(512, dtype=np.uint64) + 1
    want_sums = {tuple(e["pos"].tolist()): int((col[int(e["ptr"]):int(e["ptr"]) + 512].astype(np.uint64) * odd).sum(dtype=np.uint64))
                 for e in tab}
    rng = np.random.default_rng(3)
    where = np.nonzero(col)[0][::37]                                      # coloured voxels, wherever their block sits
    block_of = {int(e["ptr"]): e["pos"].astype(np.int64) for e in tab}
    lin = where & 511
    g = np.stack([block_of[int(w) - int(w & 511)] for w in where]) * 8 + np.stack([lin & 7, (lin >> 3) & 7, lin >> 6], 1)
    pts = np.concatenate([(g + rng.random(g.shape) * 0.4).astype(F) * F(DC.KW["voxelSize"]), np.array([[90.0, 90.0, 90.0]], F)])
    want = [gt.sample_color(torch.from_numpy(pts).cuda(), mode).cpu().numpy() for mode in (0, 1)]
    assert (want[0] != 0).sum() > 100 and (want[1] != 0).sum() > 20 and want[0][-1] == 0
    gt.close()

    np.stack([f[1] for f in frames]).tofile(tmp_path / "frames.bin")
    np.stack([image(i) for i in range(3)]).tofile(tmp_path / "colors.bin")
    np.stack([np.asarray(f[0], F) for f in frames]).tofile(tmp_path / "poses.bin")
    DC.k_inv().astype(F).tofile(tmp_path / "kinv.bin")
    pts.tofile(tmp_path / "points.bin")
    out = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("frames.bin", "colors.bin", "poses.bin", "kinv.bin", "points.bin")] +
                         [repr(BAND), str(WEIGHT_MAX)], check=True, capture_output=True, text=True).stdout.splitlines()
    head = {k: int(v) for k, v in (kv.split("=") for kv in out[0].split())}
    assert head == dict(points=len(pts), colours0=int((want[0] != 0).sum()), colours1=int((want[1] != 0).sum())), out[0]
    for mode in (0, 1):
        got = np.array([int(w, 16) for w in out[1 + mode].split()], np.uint64).astype(U)
        assert np.array_equal(got, want[mode]), mode
    sums = {tuple(int(c) for c in line.split()[1:4]): int(line.split()[4]) for line in out[3:]}
    assert sums == want_sums and len(want_sums) == len(out) - 3 and sum(1 for v in sums.values() if v) > 10
