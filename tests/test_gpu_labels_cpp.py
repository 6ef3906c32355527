"""SDF_Hashtable::integrateLabels / sampleLabels / labelCounts / removeLabel of the C++ facade (tests/cpp/labels_demo.cpp, built
here as tests/test_gpu_color_cpp.py builds its demo) against the same calls from Python on a table built the same way: the
sampled words, the counts before and after the removal, the removal's stats, and a checksum of every block's label words per
key."""
import os
import subprocess

import numpy as np
import pytest

import deintegrate_cases as DC
import labels_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
BAND, VOTE_MAX, MIN_VOTES, BINS, DOOMED = 0.12, 3, 2, 3, 2


def test_cpp_program_labels_as_python_does(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    lib = os.path.join(ROOT, "voxelhashing_demo_amd", "lib")
    exe = tmp_path / "labels_demo"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "labels_demo.cpp"), "-o", str(exe),
                    "-L", lib, "-lsdf_hashtable", "-lvoxelhash_hip", f"-Wl,-rpath,{lib}"], check=True)
    frames = DC.frames(oracle)
    images = [LC.image(0, noise=0.1) for _ in range(3)]                   # one segmentation seen from three poses: votes add up
    # the same in Python first (the projection is the one vh_create installs, as in the program): it says where labels are
    gt = vh.SDFHashtable(vh.default_params(**DC.KW), DC.W, DC.H, 1)
    for pose, d16, _ in frames:
        gt.integrate_depth(pose, torch.from_numpy(d16).cuda(), DC.k_inv())
    for (pose, d16, _), image in zip(frames, images):
        gt.integrate_labels(pose, torch.from_numpy(d16).cuda(), DC.k_inv(), torch.from_numpy(image).cuda(), BAND, VOTE_MAX)
    gt.synchronize()
    tab, vol = gt.allocated(), gt.label_volume()
    odd = 2 * np.arange(512, dtype=np.uint64) + 1
    want_sums = {tuple(e["pos"].tolist()): int((vol[int(e["ptr"]):int(e["ptr"]) + 512].astype(np.uint64) * odd).sum(dtype=np.uint64))
                 for e in tab}
    rng = np.random.default_rng(3)
    where = np.nonzero(vol)[0][::37]                                      # labelled voxels, wherever their block sits
    block_of = {int(e["ptr"]): e["pos"].astype(np.int64) for e in tab}
    lin = where & 511
    g = np.stack([block_of[int(w) - int(w & 511)] for w in where]) * 8 + np.stack([lin & 7, (lin >> 3) & 7, lin >> 6], 1)
    pts = np.concatenate([(g + rng.random(g.shape) * 0.4).astype(F) * F(DC.KW["voxelSize"]), np.array([[90.0, 90.0, 90.0]], F)])
    want = gt.sample_labels(torch.from_numpy(pts).cuda(), MIN_VOTES).cpu().numpy()
    assert 50 < (want != 0).sum() < len(pts) - 1 and want[-1] == 0        # MIN_VOTES cuts some of the labelled points away
    before = gt.label_counts(BINS, min_votes=MIN_VOTES).cpu().numpy()
    stats = gt.remove_label(DOOMED, MIN_VOTES)
    after = gt.label_counts(BINS, min_votes=MIN_VOTES).cpu().numpy()
    assert before[DOOMED] > 100 and after[DOOMED] == 0 and stats["removed_voxels"] >= before[DOOMED]
    gt.close()

    np.stack([f[1] for f in frames]).tofile(tmp_path / "frames.bin")
    np.stack(images).tofile(tmp_path / "labels.bin")
    np.stack([np.asarray(f[0], F) for f in frames]).tofile(tmp_path / "poses.bin")
    DC.k_inv().astype(F).tofile(tmp_path / "kinv.bin")
    pts.tofile(tmp_path / "points.bin")
    out = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("frames.bin", "labels.bin", "poses.bin", "kinv.bin", "points.bin")] +
                         [repr(BAND), str(VOTE_MAX), str(MIN_VOTES), str(BINS), str(DOOMED)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    head = {k: int(v) for k, v in (kv.split("=") for kv in out[0].split())}
    assert head == dict(points=len(pts), labelled=int((want != 0).sum())), out[0]
    got = np.array([int(w, 16) for w in out[1].split()], np.uint64).astype(U)
    assert np.array_equal(got, want)
    assert out[2].split() == ["counts"] + [str(int(c)) for c in before], out[2]
    keys = [line for line in out[3:] if line.startswith("key")]
    sums = {tuple(int(c) for c in line.split()[1:4]): int(line.split()[4]) for line in keys}
    assert sums == want_sums and len(want_sums) == len(keys) and sum(1 for v in sums.values() if v) > 10
    tail = out[3 + len(keys):]
    removed = {k: int(v) for k, v in (kv.split("=") for kv in tail[0].split()[1:])}
    assert removed == dict(blocks=stats["blocks"], voxels=stats["removed_voxels"], freed=stats["freed_blocks"]), tail[0]
    assert tail[1].split() == ["counts"] + [str(int(c)) for c in after], tail[1]
