"""SDF_Hashtable::streamOut / streamIn of the C++ facade (tests/cpp/stream_demo.cpp, built here as tests/test_gpu_merge_cpp.py
builds its demo) against the rule (tests/stream_ref.py) on a table built the same way from Python: which blocks leave, a
checksum of every record, and the model after the round trip."""
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC
import stream_cases as SC
import stream_ref as S

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


def test_cpp_program_streams_as_the_rule_says(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "stream_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "stream_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    frames = DC.frames(oracle)
    np.stack([f[1] for f in frames]).tofile(tmp_path / "frames.bin")
    np.stack([np.asarray(f[0], F) for f in frames]).tofile(tmp_path / "poses.bin")
    DC.k_inv().astype(F).tofile(tmp_path / "kinv.bin")
    # the same table in Python (the projection is the one vh_create installs, as in the program)
    gt = vh.SDFHashtable(vh.default_params(**DC.KW), DC.W, DC.H, 1)
    for i in (0, 1):
        gt.integrate_depth(frames[i][0], torch.from_numpy(frames[i][1]).cuda(), DC.k_inv())
    gt.synchronize()
    tab = gt.hash_table()
    region = SC.middle_sphere(SC.live_keys(tab), invert=True)
    out = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("frames.bin", "poses.bin", "kinv.bin")] +
                         [repr(c) for c in region["centre"]] + [repr(region["radius"])],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    head = {k: int(v) for k, v in (kv.split("=") for kv in out[0].split())}
    moved = [(tuple(int(c) for c in line.split()[1:4]), int(line.split()[4])) for line in out[1:] if line.startswith("out ")]
    stats = {k: int(v) for k, v in (kv.split("=") for kv in out[1 + len(moved)].split())}
    final = {tuple(int(c) for c in line.split()[1:4]): int(line.split()[4]) for line in out[2 + len(moved):]}
    want = checksums(gt)
    order = S.selection_of_table(tab, region, DC.KW["voxelSize"])
    keys = [tuple(p) for p in tab["pos"][order].tolist()]
    print(f"C++: {out[0]}; {out[1 + len(moved)]}; the rule moves {len(keys)} of {len(want)} blocks")
    assert len(keys) >= 8 and len(want) - len(keys) >= 8
    assert [k for k, _ in moved] == keys and head == {"moved": len(keys), "left": len(want) - len(keys)}
    assert all(want[k] == c for k, c in moved)
    assert stats == {"placed": len(keys), "present": 0, "unplaced": 0, "foreign": 0, "rounds": stats["rounds"], "status_placed": len(keys)}
    assert stats["rounds"] >= 1 and final == want
    gt.close()
