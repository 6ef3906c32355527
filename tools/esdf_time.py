#!/usr/bin/env python3
"""Time of vh_esdf_lattice after a workload's pose loop, in-process and warm, with HIP events around the call: the lattice of
the model's bounding box at radius 16, 64 and 255, next to vh_sample_lattice over the same box (the read floor: the
classification does the same look-ups).  The two calls alternate, round by round; medians and minima of --rounds.  The four
launches of the ESDF are separated with the diagnostics option "esdf_launches" (the call stops behind its first k launches):
launch k = the k-launch call minus the (k - 1)-launch call, medians of alternating rounds.  Beside each launch, the bytes it
moves by construction (planes 1 bit, partial distances 2 bytes, per field; outputs 4 bytes each).

  python tools/esdf_time.py [--workload C2] [--frames N] [--rounds R] [--radii 16 64 255] [--unknown keep|free|occupied] [--max-voxels N]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bytes_by_construction(dims, radius, blocks_met):
    """(classify, x, y, z) bytes: what each launch reads and writes when every array is touched once."""
    dx, dy, dz = (int(d) for d in dims)
    gy, gz = dy + 2 * radius, dz + 2 * radius
    words = (dx + 2 * radius + 7 + 63) // 64
    planes = 2 * gz * gy * words * 8
    rows, cols, out = 2 * gz * gy * dx * 2, 2 * gz * dy * dx * 2, 2 * dx * dy * dz * 4
    return (4096 * blocks_met + planes, planes + rows, rows + cols, cols + out + dx * dy * dz // 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--radii", type=int, nargs="+", default=[16, 64, 255])
    ap.add_argument("--unknown", choices=("keep", "free", "occupied"), default="keep",
                    help="what an unknown voxel counts as; under free / occupied no row of the grown box is empty")
    ap.add_argument("--max-voxels", type=int, default=0, help="shrink the box around its centre to at most this many voxels (0: the whole box)")
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
    lo = keys.min(0) * 8
    dims = (keys.max(0) + 1) * 8 - lo
    while a.max_voxels and int(np.prod(dims)) > a.max_voxels:
        axis = int(np.argmax(dims))
        lo[axis] += dims[axis] // 4
        dims[axis] -= dims[axis] // 2
    count = int(np.prod(dims))
    unknown = {"keep": V.ESDF_UNKNOWN_KEEP, "free": V.ESDF_UNKNOWN_FREE, "occupied": V.ESDF_UNKNOWN_OCCUPIED}[a.unknown]
    print(f"{a.workload}: {n} poses, {len(keys)} blocks, voxel {t.params.voxelSize} m; unknown voxels: {a.unknown}; box lo={tuple(int(v) for v in lo)} "
          f"dims={tuple(int(v) for v in dims)} voxels={count}")

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    sdf = torch.empty((count,), dtype=torch.float32, device="cuda")
    w = torch.empty((count,), dtype=torch.float32, device="cuda")
    d2 = torch.empty((count,), dtype=torch.int32, device="cuda")
    dist = torch.empty((count,), dtype=torch.float32, device="cuda")
    sample = lambda: t.sample_lattice_into(lo, dims, sdf, w)
    for radius in a.radii:
        need = t.esdf_workspace_bytes(dims, radius)
        free = torch.cuda.mem_get_info()[0]
        if need > free * 0.9:
            print(f"  R={radius:3d}: the workspace of {need / 2**30:.1f} GiB does not fit the {free / 2**30:.1f} GiB that are free: skipped "
                  "(use --max-voxels)")
            continue
        work = torch.empty((need,), dtype=torch.uint8, device="cuda")

        def esdf(k):
            t.set_option("esdf_launches", k)
            t.esdf_lattice_into(lo, dims, radius, d2, dist, unknown, work)
        for k in (1, 2, 3, 4):
            esdf(k)
        sample()
        us = np.array([[one(sample)] + [one(lambda k=k: esdf(k)) for k in (1, 2, 3, 4)] for _ in range(a.rounds)])
        t.set_option("esdf_launches", 0)
        med, best = np.median(us, 0), us.min(0)
        lo_g, hi_g = lo - radius, lo + dims + radius
        met = int((((keys * 8 + 7) >= lo_g) & ((keys * 8) < hi_g)).all(1).sum())
        nbytes = bytes_by_construction(dims, radius, met)
        near = int(((d2 != V.ESDF_NONE) & (d2.abs() < V.ESDF_FAR)).sum())
        print(f"  R={radius:3d}: workspace {need / 2**20:9.1f} MiB, voxels with a distance {near / count:.3f}")
        print(f"    vh_sample_lattice (floor)  median {med[0]:10.1f} us  min {best[0]:10.1f} us")
        for k, name in enumerate(("classify", "x pass", "y pass", "z pass + select")):
            m = med[k + 1] - (med[k] if k else 0.0)
            b = best[k + 1] - (best[k] if k else 0.0)
            print(f"    {name:26s} median {m:10.1f} us  min {b:10.1f} us  {nbytes[k] / 1e6:10.1f} MB by construction  "
                  f"{nbytes[k] / max(m, 1e-3) / 1e3:8.1f} GB/s")
        print(f"    whole call                 median {med[4]:10.1f} us  min {best[4]:10.1f} us  {count / med[4]:8.1f} Mvoxels/s  "
              f"ratio to vh_sample_lattice (medians) {med[4] / med[0]:.1f}")
        del work


if __name__ == "__main__":
    main()
