#!/usr/bin/env python3
"""Time of vh_sample_sdf and vh_sample_lattice after a workload's pose loop, in-process and warm, with HIP events around the
call, median of --rounds.  Inputs:
  (a) the vertices of extract_mesh_indexed(), in their order (block order);
  (b) the same, shuffled with a fixed seed;
  (c) the hit points of one raycast view of the workload's size, in image order;
  (d) sample_lattice over the bounding box of the allocated keys.
Per input and mode: microseconds, points/s, and algorithmic bytes / time, the bytes being the inputs (12 B per point), the
outputs (sdf, weight and gradient: 20 B per point; lattice: 8 B per voxel) and 4 KB per distinct block touched.

  python tools/sample_time.py [--workload C2] [--frames N] [--rounds R]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def blocks_touched(points, voxel_size, keys, mode):
    """Distinct allocated blocks the points' voxels lie in (nearest: the voxel; trilinear: the eight corners)."""
    u = points.astype(np.float32) / np.float32(voxel_size)
    ok = (np.abs(u) < 2.0 ** 30).all(1)
    u = u[ok]
    if mode == 0:
        base = np.trunc(u + np.copysign(np.float32(0.5), u)).astype(np.int64)
        corners = [(0, 0, 0)]
    else:
        base = np.floor(u).astype(np.int64)
        corners = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
    pack = lambda k: ((k[:, 0] + (1 << 20)) << 42) | ((k[:, 1] + (1 << 20)) << 21) | (k[:, 2] + (1 << 20))
    have = np.unique(pack(np.asarray(keys, np.int64)))
    seen = np.unique(np.concatenate([np.unique(pack((base + np.array(c)) >> 3)) for c in corners]))
    return int(np.isin(seen, have).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--rounds", type=int, default=10)
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
    for p in poses:
        t.integrate(p, synth.render_room_verts(p, Wd, Ht, prims, device="cuda"))
    t.synchronize()
    keys = t.allocated()["pos"].astype(np.int64)
    vs = t.params.voxelSize
    print(f"{a.workload}: {n} poses, {len(keys)} blocks, voxel {vs} m")

    def timed(fn):
        fn()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        return float(np.median(us)), float(min(us))

    verts, _ = t.extract_mesh_indexed()
    shuffled = verts[np.random.RandomState(0).permutation(len(verts))]
    pose = poses[len(poses) // 2]
    depth = torch.empty((Ht, Wd), dtype=torch.float32, device="cuda")
    vmap = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    nmap = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    t.raycast_maps(pose, depth, vmap, nmap)
    cam = vmap.cpu().numpy().reshape(-1, 4)
    hit = depth.cpu().numpy().reshape(-1) > 0
    T = np.asarray(pose, np.float32).reshape(4, 4)
    world = (cam[hit, :3] @ T[:3, :3].T + T[:3, 3]).astype(np.float32)              # camera frame -> world, image order
    inputs = (("(a) mesh vertices, in order", verts), ("(b) mesh vertices, shuffled", shuffled),
              (f"(c) hits of a {Wd}x{Ht} raycast, image order", world))
    for label, pts in inputs:
        d = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
        sdf = torch.empty((len(pts),), dtype=torch.float32, device="cuda")
        w = torch.empty((len(pts),), dtype=torch.float32, device="cuda")
        g = torch.empty((len(pts), 3), dtype=torch.float32, device="cuda")
        for mode, name in ((V.SAMPLE_NEAREST, "nearest"), (V.SAMPLE_TRILINEAR, "trilinear")):
            touched = blocks_touched(pts, vs, keys, mode)
            nbytes = 32 * len(pts) + 4096 * touched
            med, best = timed(lambda: t.sample_sdf_into(d, sdf, w, g, mode))
            share = float((~torch.isnan(sdf)).float().mean())
            print(f"  {label:44s} {name:9s} n={len(pts):8d} blocks={touched:6d} with a sample={share:.3f}  median {med:9.1f} us  "
                  f"min {best:9.1f} us  {len(pts) / med:8.1f} Mpoints/s  {nbytes / med / 1e3:8.1f} GB/s")
    lo = keys.min(0) * 8
    dims = (keys.max(0) + 1) * 8 - lo
    count = int(np.prod(dims))
    sdf = torch.empty((count,), dtype=torch.float32, device="cuda")
    w = torch.empty((count,), dtype=torch.float32, device="cuda")
    med, best = timed(lambda: t.sample_lattice_into(lo, dims, sdf, w))
    nbytes = 8 * count + 4096 * len(keys)
    print(f"  (d) lattice over the allocated keys' box      lo={tuple(int(v) for v in lo)} dims={tuple(int(v) for v in dims)} "
          f"voxels={count} valid={float((~torch.isnan(sdf)).float().mean()):.3f}  median {med:9.1f} us  min {best:9.1f} us  "
          f"{count / med:8.1f} Mvoxels/s  {nbytes / med / 1e3:8.1f} GB/s")


if __name__ == "__main__":
    main()
