#!/usr/bin/env python3
"""Time of vh_deintegrate_depth after a workload's pose loop, next to its yardstick in the same process: the step-level TSDF
update of the same frame over the same list, vh_set_pose + vh_flatten + vh_integrate_depth_map.  The two alternate -- frame
out, frame in again -- so the model is in the same state at the start of every cycle, and each call sits between HIP events of
its own.  After --warmup cycles, --cycles cycles are recorded and read once at the end: median and mean per call.

  python tools/deintegrate_time.py [--workload C2] [--frames N] [--cycles K] [--warmup W]

The removal moves the bytes of the update (4 KiB in per visible block, 4 KiB out per block it changed), so about the same time
is the expectation; the flatten is part of both sides.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--cycles", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch

    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("deintegrate_time.py needs a GPU: there is nothing to time without one")
    wl = WORKLOADS[a.workload]
    Wd, Ht = wl["width"], wl["height"]
    n = a.frames or wl["frames"]
    poses = synth.camera_loop(wl.get("loop", wl["frames"]))[:n]
    prims = synth.room_primitives()
    t = V.SDFHashtable(V.default_params(numBuckets=wl["buckets"], numVoxelBlocks=wl["blocks"], voxelSize=wl["voxel"]), Wd, Ht,
                       V.SEM_PINHOLE)
    kinv = np.linalg.inv(synth.K_matrix(Wd, Ht).astype(np.float64)).astype(np.float32)

    def sensor(p):
        z = synth.render_room_verts(p, Wd, Ht, prims, device="cuda")[..., 2]
        return torch.round(z * 5000.0).clamp(0, 65535).to(torch.int32).to(torch.uint16).contiguous()

    for p in poses:
        t.integrate_depth(p, sensor(p), kinv)
    t.synchronize()
    pose = poses[len(poses) // 2]
    d16 = sensor(pose)
    verts = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    nrm = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    V.preprocess(d16, kinv, verts, nrm)
    torch.cuda.synchronize()
    t.set_pose(pose)
    visible = t.flatten()
    print(f"{a.workload}: {n} poses, {len(t.allocated())} blocks, {visible} visible from pose {len(poses) // 2}, {Wd}x{Ht}")

    def cycle(events):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events else None
        if e: e[0].record()
        t.deintegrate_depth(pose, d16, kinv)
        if e: e[1].record()
        t.set_pose(pose)
        t.flatten(sync=False)
        t.integrate_depth_map(verts)
        if e: e[2].record()
        return e

    for _ in range(a.warmup):
        cycle(False)
    t.synchronize()
    recorded = [cycle(True) for _ in range(a.cycles)]
    t.synchronize()
    out_us = np.array([1e3 * e[0].elapsed_time(e[1]) for e in recorded])
    in_us = np.array([1e3 * e[1].elapsed_time(e[2]) for e in recorded])
    for name, us in (("vh_deintegrate_depth", out_us), ("set_pose + flatten + integrate_depth_map", in_us)):
        print(f"  {name:44s} median {np.median(us):8.1f} us  mean {us.mean():8.1f} us  min {us.min():8.1f} us  "
              f"p90 {np.percentile(us, 90):8.1f} us  over {len(us)} calls")
    print(f"  ratio of medians (out / in): {np.median(out_us) / np.median(in_us):.3f}")


if __name__ == "__main__":
    main()
