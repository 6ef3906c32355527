#!/usr/bin/env python3
"""Time of vh_cast_rays after a workload's pose loop, in-process and warm, with HIP events around the call, median of --rounds
(as tools/sample_time.py times its own).  Ray sets:
  (a) the rays of a loop pose's pinhole view with the shared plane (row 2 of the inverse pose), in 8x8-patch order -- the rays
      of a wave are the pixels of a patch, as in vh_raycast -- next to vh_raycast with raycast_beam 0 (the same per-lane walk
      from t_min) and with the default form, for the same view;
  (b) the same rays in row-major order, and shuffled with a fixed seed;
  (c) from every vertex of the indexed mesh, a ray along its normal (an occlusion query): origin = the vertex, t from two
      voxels to --reach metres, samples along each ray.
Per set: microseconds (median, min), rays/s, hits, and for (a) the bits of t against the raycast's depth image.

  python tools/rays_time.py [--workload C2] [--frames N] [--rounds R] [--reach 1.0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def patch_order(W, H):
    """Pixel indices of the image in the order of 8x8 patches (patches row-major, pixels row-major inside a patch)."""
    v, u = np.divmod(np.arange(W * H), W)
    key = (((v // 8) * ((W + 7) // 8) + u // 8) * 64 + (v % 8) * 8 + u % 8)
    return np.argsort(key, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reach", type=float, default=1.0, help="length of the occlusion rays of set (c), metres")
    ap.add_argument("--t", type=float, nargs=2, default=(0.1, 5.0), help="t_min t_max of the view of sets (a) and (b)")
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
    vs = t.params.voxelSize
    print(f"{a.workload}: {n} poses, {len(t.allocated())} blocks, voxel {vs} m; library {V._lib.LIB_PATH}")

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

    def report(label, count, med, best, extra=""):
        print(f"  {label:58s} n={count:8d}  median {med:9.1f} us  min {best:9.1f} us  {count / med:8.1f} Mrays/s  {extra}")

    # ---- the view: vh_raycast, per-lane walk from t_min and the default form
    pose = np.asarray(poses[len(poses) // 2], np.float32).reshape(4, 4)
    fx, fy, cx, cy = 525.0 * Wd / 640, 525.0 * Wd / 640, Wd / 2.0, Ht / 2.0
    t.set_raycast_intrinsics(fx, fy, cx, cy)
    depth = torch.empty((Ht, Wd), dtype=torch.float32, device="cuda")
    for beam, name in ((0, "vh_raycast, raycast_beam 0 (the same walk)"), (3, "vh_raycast, default form")):
        t.set_option("raycast_beam", beam)
        med, best = timed(lambda: t.raycast(pose, depth, *a.t))
        image = depth.cpu().numpy().reshape(-1)
        report(name, Wd * Ht, med, best, f"hits {float((image != 0).mean()):.3f}")
    t.set_option("raycast_beam", 3)            # (the library's default)
    # the shared plane: row 2 of the cofactor inverse, from the oracle (the library's own arithmetic, so that t has the bits of
    # the depth image; the count of equal words is reported below)
    import oracle
    plane = np.asarray(oracle.invert4x4(pose), np.float32).reshape(4, 4)[2]
    rays = V.pinhole_rays(pose, fx, fy, cx, cy, Wd, Ht, *a.t)
    order = patch_order(Wd, Ht)
    shuffle = np.random.RandomState(0).permutation(len(rays))
    sets = (("(a) pinhole rays, shared plane, 8x8-patch order", order), ("(b) the same, row-major order", np.arange(len(rays))),
            ("(b) the same, shuffled", shuffle))
    out_t = torch.empty((len(rays),), dtype=torch.float32, device="cuda")
    out_n = torch.empty((len(rays), 3), dtype=torch.float32, device="cuda")
    out_v = torch.empty((len(rays), 4), dtype=torch.int32, device="cuda")
    for label, idx in sets:
        d = torch.from_numpy(np.ascontiguousarray(rays[idx])).cuda()
        med, best = timed(lambda: t.cast_rays_into(d, out_t, depth_plane=plane))
        got = np.empty(len(rays), np.float32)
        got[idx] = out_t.cpu().numpy()
        same = int(((got.view(np.uint32) == image.view(np.uint32)) | (np.isnan(got) & (image == 0))).sum())
        report(label + ", t only", len(rays), med, best, f"hits {float((~np.isnan(got)).mean()):.3f}  equal to the depth image {same}/{len(rays)}")
        med, best = timed(lambda: t.cast_rays_into(d, out_t, out_n, out_v, depth_plane=plane))
        report(label + ", t + normals + voxels", len(rays), med, best)

    # ---- (c) occlusion rays from the mesh
    verts, _, normals = t.extract_mesh_indexed(normals=True)
    occ = np.zeros((len(verts), 8), np.float32)
    occ[:, 0:3], occ[:, 4:7] = verts, normals
    occ[:, 3], occ[:, 7] = 2 * vs, a.reach
    occ = occ[np.isfinite(occ).all(1) & (np.abs(normals).sum(1) > 0)]
    d = torch.from_numpy(occ).cuda()
    ot = torch.empty((len(occ),), dtype=torch.float32, device="cuda")
    med, best = timed(lambda: t.cast_rays_into(d, ot))
    report(f"(c) mesh vertices along their normals, {2 * vs:g}..{a.reach:g} m, t only", len(occ), med, best,
           f"occluded {float((~torch.isnan(ot)).float().mean()):.3f}")


if __name__ == "__main__":
    main()
