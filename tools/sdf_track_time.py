#!/usr/bin/env python3
"""Time of tracking against the model itself (vh_sdf_build_system, vh_sdf_align) next to what a tracked frame does today
(vh_icp_build_system, vh_icp_align, vh_raycast_maps), all on the same model and the same frame, alternating in one process.

  python tools/sdf_track_time.py [--workload C2] [--frames N] [--truncation 0.06] [--cycles K] [--warmup W] [--color]

The model is the workload's pose loop fused with --truncation (the SDF tracker is for truncations of a few voxels; the
workload's own default is 1.0).  The frame is the one after the last fused pose; both trackers start from the last fused pose.
Every call is followed by a synchronisation and timed on the host clock from before the call to after it: four of the five
calls read a result back and synchronise by themselves, so the time a caller waits is what there is to compare.  After
--warmup cycles, --cycles cycles are recorded: median, mean, minimum and 90th percentile per call.
--color fuses a texture fixed to the scene with every frame (vh_integrate_depth_color, a band of three voxels) and times the
joint tracker instead of the ICP: one round and one 10-round Align of vh_sdf_color_* next to vh_sdf_*'s, same model, same frame.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=60, help="poses fused before the measurement")
    ap.add_argument("--truncation", type=float, default=0.06)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--color", action="store_true", help="time vh_sdf_color_* next to vh_sdf_* on a coloured model")
    a = ap.parse_args()
    import torch

    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import synth, tracking
    if not torch.cuda.is_available():
        raise SystemExit("sdf_track_time.py needs a GPU: there is nothing to time without one")
    wl = WORKLOADS[a.workload]
    Wd, Ht = wl["width"], wl["height"]
    poses = synth.camera_loop(wl.get("loop", wl["frames"]))[:a.frames + 1]
    prims = synth.room_primitives()
    t = V.SDFHashtable(V.default_params(numBuckets=wl["buckets"], numVoxelBlocks=wl["blocks"], voxelSize=wl["voxel"],
                                        truncation=a.truncation), Wd, Ht, V.SEM_PINHOLE)
    K = synth.K_matrix(Wd, Ht)
    kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)

    def sensor(p):
        z = synth.render_room_verts(p, Wd, Ht, prims, device="cuda")[..., 2]
        return torch.round(z * 5000.0).clamp(0, 65535).to(torch.int32).to(torch.uint16).contiguous()

    def textured(p):
        """The colour image of pose p: a smooth texture of the world position each pixel sees."""
        v = synth.render_room_verts(p, Wd, Ht, prims, device="cuda")
        T = torch.as_tensor(np.asarray(p, np.float32).reshape(4, 4), device="cuda")
        x, y, z = (v[..., :3] @ T[:3, :3].T + T[:3, 3]).unbind(-1)
        r = 128 + 100 * torch.sin(7.0 * x + 3.0 * z + 0.3) * torch.cos(5.0 * y)
        g = 128 + 100 * torch.sin(4.0 * x - 6.0 * y + 5.0 * z + 1.0)
        b = 128 + 100 * torch.cos(6.5 * y - 0.7) * torch.cos(3.0 * x - 4.0 * z + 0.2)
        r, g, b = (c.round().to(torch.int32) for c in (r, g, b))
        return (r | (g << 8) | (b << 16)).contiguous()

    for p in poses[:-1]:
        if a.color:
            t.integrate_depth_color(p, sensor(p), kinv, textured(p), 3.0 * wl["voxel"])
        else:
            t.integrate_depth(p, sensor(p), kinv)
    t.synchronize()
    last = np.asarray(poses[-2], np.float64).reshape(4, 4)
    truth = np.asarray(poses[-1], np.float64).reshape(4, 4)
    new = lambda: torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    in_v, in_n, model_v, model_n = new(), new(), new(), new()
    depth = torch.empty((Ht, Wd), dtype=torch.float32, device="cuda")
    V.preprocess(sensor(poses[-1]), kinv, in_v, in_n)
    sdf = tracking.SdfTracking(t, K, dist_thres=0.08, max_iters=10)
    icp = tracking.CameraTracking(Wd, Ht, K, flags=tracking.ICP_ABS_DISTANCE | tracking.ICP_NEED_TARGET, max_iters=20)
    eye = np.eye(4, dtype=np.float32)
    calls = [
        ("vh_sdf_build_system (one round)", lambda: sdf.build_system(in_v, last)),
        ("vh_sdf_align, 10 rounds", lambda: sdf.Align(in_v, last)),
        ("vh_icp_build_system (one round)", lambda: icp.build_system(in_v, model_v, model_n, eye)),
        ("vh_icp_align, 20 rounds", lambda: icp.Align(in_v, model_v, model_n)),
        ("vh_raycast_maps", lambda: t.raycast_maps(last.astype(np.float32), depth, model_v, model_n)),
    ]
    t.raycast_maps(last.astype(np.float32), depth, model_v, model_n)
    joint = None
    if a.color:
        joint = tracking.SdfColorTracking(t, K=K, dist_thres=0.08, max_iters=10)
        rgba = textured(poses[-1])
        calls = calls[:2] + [
            ("vh_sdf_color_build_system (one round)", lambda: joint.build_system(in_v, rgba, last)),
            ("vh_sdf_color_align, 10 rounds", lambda: joint.Align(in_v, rgba, last)),
        ]
    t.synchronize()
    us = {name: [] for name, _ in calls}
    for cycle in range(a.warmup + a.cycles):
        for name, call in calls:
            t0 = time.perf_counter()
            call()
            t.synchronize()
            if cycle >= a.warmup:
                us[name].append(1e6 * (time.perf_counter() - t0))
    err = lambda T: 1e3 * float(np.abs(np.asarray(T, np.float64)[:3, 3] - truth[:3, 3]).max())
    print(f"{a.workload}: {a.frames} poses fused with truncation {a.truncation}, {len(t.allocated())} blocks, {Wd}x{Ht}; "
          f"start {err(last):.2f} mm from the truth, vh_sdf_align ends {err(sdf.pose):.2f} mm ({sdf.last[3]} kept), "
          + (f"vh_sdf_color_align {err(joint.pose):.2f} mm ({joint.last[3]} rows, color_weight {joint.color_weight})" if joint else
             f"vh_icp_align {err(last @ icp.delta.astype(np.float64)):.2f} mm ({icp.last[3]} pairs)"))
    for name, _ in calls:
        v = np.array(us[name])
        print(f"  {name:34s} median {np.median(v):8.1f} us  mean {v.mean():8.1f} us  min {v.min():8.1f} us  "
              f"p90 {np.percentile(v, 90):8.1f} us  over {len(v)} calls")
    sdf.close()
    if joint:
        joint.close()
    icp.close()
    t.close()


if __name__ == "__main__":
    main()
