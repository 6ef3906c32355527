#!/usr/bin/env python3
"""Time of the colour launch and of the colour sampler after a workload's pose loop, each next to its yardstick in the same
process, the two alternating cycle by cycle.

  colour launch   integrate_ms of vh_integrate_color_map (color_integrate_kernel alone, from the per-dispatch HIP events of
                  vh_set_profiling), against integrate_ms of the step-level TSDF update of the same frame over the same compact
                  list: vh_set_pose + vh_flatten + vh_integrate_depth_map (integrate_kernel alone).  The colour launch moves at
                  most 8 KiB per block (4 KiB TSDF in, 2 KiB colour in, at most 2 KiB out), the update 8 KiB.
  removal launch  integrate_ms of vh_deintegrate_color (color_deintegrate_kernel alone) directly behind the colour launch, with
                  the same image and over the same list: the sample just added is taken out again, so the model the cycles
                  see stays the same.  It reads the uint16 sensor image where the colour launch reads the vertex map.
  colour sampler  vh_sample_color against vh_sample_sdf (sdf only), both trilinear, over the same points -- the voxel positions
                  of the visible blocks, each moved into its cell -- between HIP events on the context's stream.

After --warmup cycles, --cycles cycles are recorded: median and minimum per call, and the ratios of the medians.

  python tools/color_time.py [--workload C2] [--frames N] [--cycles K] [--warmup W] [--band METRES]
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
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--band", type=float, default=0.0, help="colour band in metres (0: three voxels)")
    a = ap.parse_args()
    import torch

    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("color_time.py needs a GPU: there is nothing to time without one")
    wl = WORKLOADS[a.workload]
    Wd, Ht = wl["width"], wl["height"]
    n = a.frames or wl["frames"]
    band = a.band or 3.0 * wl["voxel"]
    poses = synth.camera_loop(wl.get("loop", wl["frames"]))[:n]
    prims = synth.room_primitives()
    t = V.SDFHashtable(V.default_params(numBuckets=wl["buckets"], numVoxelBlocks=wl["blocks"], voxelSize=wl["voxel"]), Wd, Ht,
                       V.SEM_PINHOLE)
    kinv = np.linalg.inv(synth.K_matrix(Wd, Ht).astype(np.float64)).astype(np.float32)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def sensor(p):
        z = synth.render_room_verts(p, Wd, Ht, prims, device="cuda")[..., 2]
        return torch.round(z * 5000.0).clamp(0, 65535).to(torch.int32).to(torch.uint16).contiguous()

    def picture():
        return torch.randint(0, 1 << 24, (Ht, Wd), dtype=torch.int32, device="cuda", generator=gen)

    for p in poses:
        t.integrate_depth_color(p, sensor(p), kinv, picture(), band)
    t.synchronize()
    pose = poses[len(poses) // 2]
    d16, rgba = sensor(pose), picture()
    verts = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    nrm = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    V.preprocess(d16, kinv, verts, nrm)
    torch.cuda.synchronize()
    t.set_pose(pose)
    visible = t.flatten()
    keys = torch.from_numpy(np.ascontiguousarray(t.compact()["pos"]).astype(np.int64)).cuda()
    i = torch.arange(512, device="cuda")
    local = torch.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    g = (keys[:, None, :] * 8 + local[None, :, :]).reshape(-1, 3).to(torch.float32)
    points = ((g + torch.rand(g.shape, device="cuda", generator=gen)) * wl["voxel"]).contiguous()
    sdf = torch.empty(len(points), dtype=torch.float32, device="cuda")
    col = torch.empty(len(points), dtype=torch.int32, device="cuda")
    print(f"{a.workload}: {n} poses, {len(t.allocated())} blocks, {visible} visible from pose {len(poses) // 2}, {Wd}x{Ht}, "
          f"band {band:g} m, {len(points)} sample points")
    t.set_profiling(True)

    rows = []
    for cycle in range(a.warmup + a.cycles):
        t.kernel_times()                                      # (reset)
        t.integrate_color_map(pose, verts, rgba, band)
        colour = t.kernel_times()
        t.deintegrate_color(pose, d16, kinv, rgba, band)
        removal = t.kernel_times()
        t.set_pose(pose)
        t.flatten(sync=False)
        t.integrate_depth_map(verts)
        update = t.kernel_times()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        t.sample_color_into(points, col)
        e[1].record()
        e[2].record()
        t.sample_sdf_into(points, sdf)
        e[3].record()
        torch.cuda.synchronize()
        if cycle >= a.warmup:
            rows.append((1e3 * colour["integrate_ms"], 1e3 * update["integrate_ms"], 1e3 * colour["flatten_ms"],
                         1e3 * e[0].elapsed_time(e[1]), 1e3 * e[2].elapsed_time(e[3]), 1e3 * removal["integrate_ms"]))
    r = np.array(rows)
    coloured = int((torch.from_numpy(t.color_volume().view(np.int32)) != 0).sum())
    print(f"  {coloured} coloured voxels; {int((col != 0).sum())} of the points have a colour, {int(torch.isfinite(sdf).sum())} an sdf")
    for name, c in (("colour launch", 0), ("removal launch", 5), ("update launch (yardstick)", 1), ("flatten of the colour call", 2),
                    ("vh_sample_color", 3), ("vh_sample_sdf (yardstick)", 4)):
        print(f"  {name:30s} median {np.median(r[:, c]):9.1f} us  min {r[:, c].min():9.1f} us  over {len(r)} cycles")
    print(f"  ratio of medians (colour launch / update launch): {np.median(r[:, 0]) / np.median(r[:, 1]):.3f}")
    print(f"  ratio of medians (removal launch / colour launch): {np.median(r[:, 5]) / np.median(r[:, 0]):.3f}")
    print(f"  ratio of medians (vh_sample_color / vh_sample_sdf): {np.median(r[:, 3]) / np.median(r[:, 4]):.3f}")


if __name__ == "__main__":
    main()
