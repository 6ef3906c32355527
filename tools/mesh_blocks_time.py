#!/usr/bin/env python3
"""What a live consumer pays to keep its mesh current, against extracting the whole model again: a workload's pose loop in one
process, and at every --every-th pose three quantities, alternating over --rounds rounds (as tools/ab_kernels.py alternates),
with HIP events around the calls:
  (a) the update on the device alone: vh_changes with halo MESH into device lists, then vh_extract_mesh_blocks of what it lists
      (each round starts from a copy of the state as it was before the pose's update, so every round does the same work);
  (b) vh_extract_mesh of the whole model into the same buffers -- the baseline, the kernels as they were before this call existed;
  (c) vh_changes on a state that has just seen the model (nothing to list: the block list, one digest pass over every allocated
      block, the state pass, the scans) next to a device-to-device copy of as many bytes as the allocated blocks hold, the read
      floor of the digest pass.  The digest kernel alone is a row of `rocprofv3 --kernel-trace --stats` over this tool
      (tools/kstats.py <dir> changes_digest).
Prints the medians and minima over all samples and the listed / allocated block counts.

  python tools/mesh_blocks_time.py [--workload C2|C3] [--frames N] [--every 10] [--rounds 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses of the loop (0: the workload's)")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch

    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import synth
    wl = WORKLOADS[a.workload]
    Wd, Ht = wl["width"], wl["height"]
    n = a.frames or wl["frames"]
    poses = synth.camera_loop(wl.get("loop", wl["frames"]))[:n]
    prims = synth.room_primitives()
    t = V.SDFHashtable(V.default_params(numBuckets=wl["buckets"], numVoxelBlocks=wl["blocks"], voxelSize=wl["voxel"]), Wd, Ht,
                       V.SEM_PINHOLE)
    pool = int(t.params.numVoxelBlocks)
    state, before = t.changes_state(), t.changes_state()
    changed = torch.empty((pool, 4), dtype=torch.int32, device="cuda")
    removed = torch.empty((pool, 4), dtype=torch.int32, device="cuda")
    first = torch.empty((pool + 1,), dtype=torch.int64, device="cuda")
    pos = torch.empty((1 << 16, 3, 3), dtype=torch.float32, device="cuda")
    copy_src = copy_dst = None
    rows = {k: [] for k in ("update", "changes", "blocks", "whole", "peek", "copy")}
    counts = []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for i, p in enumerate(poses):
        t.integrate(p, synth.render_room_verts(p, Wd, Ht, prims, device="cuda"))
        if i % a.every != a.every - 1:
            continue
        t.synchronize()
        blocks = int((t.hash_table()["ptr"] != -1).sum())
        total = t.mesh_count()
        if total > pos.shape[0]:
            pos = torch.empty((total + total // 4, 3, 3), dtype=torch.float32, device="cuda")
        if copy_src is None or copy_src.numel() < blocks * 4096:
            copy_src = torch.zeros((blocks * 4096 * 2,), dtype=torch.uint8, device="cuda")
            copy_dst = torch.empty_like(copy_src)
        before.copy_(state)
        torch.cuda.synchronize()
        listed = triangles = 0
        for r in range(a.rounds + 1):                # (round 0 warms up and is not kept)
            state.copy_(before)
            torch.cuda.synchronize()
            ms_c, (listed, gone) = timed(lambda: t.changes_into(state, pool, changed, pool, removed, halo="mesh"))
            ms_b, triangles = timed(lambda: t.extract_mesh_blocks_into(changed, pos.shape[0], pos, None, first, n=listed))
            ms_w, whole = timed(lambda: t.extract_mesh_into(pos.shape[0], pos))
            ms_p, (none, _) = timed(lambda: t.changes_into(state, 0, None, 0, None, halo="mesh"))
            ms_m, _ = timed(lambda: copy_dst[:blocks * 4096].copy_(copy_src[:blocks * 4096]))
            assert none == 0 and whole == total and triangles <= pos.shape[0]
            if r:
                for k, v in (("update", ms_c + ms_b), ("changes", ms_c), ("blocks", ms_b), ("whole", ms_w), ("peek", ms_p), ("copy", ms_m)):
                    rows[k].append(v)
        counts.append((listed, blocks, triangles, total))
    c = np.array(counts, np.float64)
    print(f"{a.workload}: {n} poses, a sample every {a.every} ({len(counts)} samples x {a.rounds} rounds); at the end {int(c[-1, 1])} "
          f"blocks, {int(c[-1, 3])} triangles")
    print(f"  listed / allocated blocks: median {int(np.median(c[:, 0]))} / {int(np.median(c[:, 1]))}, last {int(c[-1, 0])} / {int(c[-1, 1])}; "
          f"triangles re-made / in the model: median {int(np.median(c[:, 2]))} / {int(np.median(c[:, 3]))}")
    names = {"update": "(a) vh_changes + vh_extract_mesh_blocks", "changes": "      vh_changes (halo MESH, device lists)",
             "blocks": "      vh_extract_mesh_blocks of what it lists", "whole": "(b) vh_extract_mesh, whole model",
             "peek": "(c) vh_changes, nothing to list", "copy": "      device-to-device copy of the blocks' bytes"}
    for k, label in names.items():
        v = np.array(rows[k])
        print(f"  {label:48s} median {np.median(v):8.3f} ms  min {v.min():8.3f} ms")


if __name__ == "__main__":
    main()
