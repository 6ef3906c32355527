"""mergeColor, reintegrateDepthColor, deintegrateDepthColor, saveColor and loadColor of the C++ facade
(tests/cpp/merge_color_demo.cpp, built here as tests/test_gpu_merge_cpp.py builds its demo) against the same calls from Python on
tables built the same way: the stats, and per block key a checksum of the voxels and of the colour words at two points of the
sequence."""
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC
import merge_cases as MC
import merge_color_cases as CC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def checksums(tab, words, n):
    """{key: the sum over the block's n 32-bit words of word[i] * (2 i + 1), modulo 2^64}; `words` holds n / 512 per voxel."""
    odd = (2 * np.arange(n, dtype=np.uint64) + 1)
    per = n // 512
    out = {}
    for e in tab[tab["ptr"] != -1]:
        block = words[int(e["ptr"]) * per:(int(e["ptr"]) + 512) * per].astype(np.uint64)
        out[tuple(e["pos"].tolist())] = int((block * odd).sum(dtype=np.uint64))
    return out


def test_cpp_program_carries_colour_as_python_does(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "merge_color_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "merge_color_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    frames = DC.frames(oracle)
    images = [CC.image(i) for i in range(3)]
    np.stack([f[1] for f in frames]).tofile(tmp_path / "frames.bin")
    np.stack(images).tofile(tmp_path / "colors.bin")
    np.stack([np.asarray(f[0], F) for f in frames]).tofile(tmp_path / "poses.bin")
    DC.k_inv().astype(F).tofile(tmp_path / "kinv.bin")
    CC.CLOSE.tofile(tmp_path / "transform.bin")
    band, weight_max = float(F(CC.BAND)), 3
    args = [str(tmp_path / n) for n in ("frames.bin", "colors.bin", "poses.bin", "kinv.bin", "transform.bin")]
    out = subprocess.run([str(exe)] + args + ["1", repr(band), str(weight_max), str(tmp_path / "cpp.vhc")],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    got_stats = {k: int(v) for k, v in (kv.split("=") for kv in out[0].split())}
    got = {tuple(int(c) for c in line.split()[1:4]): tuple(int(c) for c in line.split()[4:7]) for line in out[1:]}
    # the same in Python (the projection is the one vh_create installs, as in the program)
    src = vh.SDFHashtable(vh.default_params(**MC.SRC_KW), MC.W, MC.H, 1)
    dst = vh.SDFHashtable(vh.default_params(**MC.DST_KW), MC.W, MC.H, 1)
    d16 = [torch.from_numpy(f[1]).cuda() for f in frames]
    rgba = [torch.from_numpy(c).cuda() for c in images]
    for gt, which in ((src, (0, 1)), (dst, (2,))):
        for i in which:
            gt.integrate_depth_color(frames[i][0], d16[i], DC.k_inv(), rgba[i], band, 255)
    src.reintegrate_depth_color(frames[1][0], frames[0][0], d16[1], DC.k_inv(), rgba[1], band, 255)
    stats = dst.merge(src, CC.CLOSE, 1, colors=True, color_weight_max=weight_max)
    path = str(tmp_path / "python.vhc")
    dst.save_color(path)
    merged = dst.color_volume()
    dst.deintegrate_depth_color(frames[2][0], d16[2], DC.k_inv(), rgba[2], band)
    dst.synchronize()
    tab = dst.hash_table()
    voxels = checksums(tab, dst.sdf_blocks().view(np.uint32), 1024)
    removed = checksums(tab, dst.color_volume(), 512)
    dst.load_color(path)
    assert np.array_equal(dst.color_volume(), merged) and merged.any()
    loaded = checksums(tab, dst.color_volume(), 512)
    want = {k: (voxels[k], removed[k], loaded[k]) for k in voxels}
    print(f"C++: {out[0]}; Python: {stats}; {len(want)} blocks")
    assert got_stats == stats and stats["allocated"] > 0 and stats["unplaced"] == 0
    assert got == want and len(want) == len(out) - 1
    assert any(v[1] != v[2] for v in want.values())                               # the de-integration moved colour
    # the two files hold the same records, whatever slot and heap block a key got
    def records(p):
        raw = np.fromfile(p, np.uint8)[32:].reshape(-1, 12 + 2048)
        return {tuple(r[:12].view(np.int32).tolist()): r[12:].tobytes() for r in raw}
    assert records(path) == records(str(tmp_path / "cpp.vhc"))
    src.close()
    dst.close()
