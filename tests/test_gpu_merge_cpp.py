"""SDF_Hashtable::merge of the C++ facade (tests/cpp/merge_demo.cpp, built here as tests/test_gpu_sdf_track_cpp.py builds its
demo) against the same calls from Python on tables built the same way: the stats, and a checksum of every block per key."""
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC
import merge_cases as MC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def checksums(gt):
    """{key: the sum over the block's 1024 32-bit words of word[i] * (2 i + 1), modulo 2^64}."""
    tab, vox = gt.hash_table(), gt.sdf_blocks()
    odd = (2 * np.arange(1024, dtype=np.uint64) + 1)
    out = {}
    for e in tab[tab["ptr"] != -1]:
        words = vox[int(e["ptr"]):int(e["ptr"]) + 512].view(np.uint32).astype(np.uint64)
        out[tuple(e["pos"].tolist())] = int((words * odd).sum(dtype=np.uint64))
    return out


def test_cpp_program_merges_as_python_does(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "merge_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "merge_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    frames = DC.frames(oracle)
    np.stack([f[1] for f in frames]).tofile(tmp_path / "frames.bin")
    np.stack([np.asarray(f[0], F) for f in frames]).tofile(tmp_path / "poses.bin")
    DC.k_inv().astype(F).tofile(tmp_path / "kinv.bin")
    MC.OBLIQUE.tofile(tmp_path / "transform.bin")
    out = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("frames.bin", "poses.bin", "kinv.bin", "transform.bin")] + ["1"],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    got_stats = {k: int(v) for k, v in (kv.split("=") for kv in out[0].split())}
    got = {tuple(int(c) for c in line.split()[1:4]): int(line.split()[4]) for line in out[1:]}
    # the same in Python (the projection is the one vh_create installs, as in the program)
    src = vh.SDFHashtable(vh.default_params(**MC.SRC_KW), MC.W, MC.H, 1)
    dst = vh.SDFHashtable(vh.default_params(**MC.DST_KW), MC.W, MC.H, 1)
    for gt, which in ((src, MC.SRC_FRAMES), (dst, MC.DST_FRAMES)):
        for i in which:
            gt.integrate_depth(frames[i][0], torch.from_numpy(frames[i][1]).cuda(), DC.k_inv())
    stats = dst.merge(src, MC.OBLIQUE, 1)
    want = checksums(dst)
    print(f"C++: {out[0]}; Python: {stats}; {len(want)} blocks")
    assert got_stats == stats and stats["allocated"] > 0 and stats["unplaced"] == 0
    assert got == want and len(want) == len(out) - 1
    src.close()
    dst.close()
