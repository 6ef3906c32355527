#!/usr/bin/env python3
"""Time of the label calls after a workload's pose loop, each next to its yardstick in the same process, alternating cycle by
cycle.

  label launch    integrate_ms of vh_integrate_labels_map (label_integrate_kernel alone, from the per-dispatch HIP events of
                  vh_set_profiling), against integrate_ms of vh_integrate_color_map (color_integrate_kernel alone) with the same
                  pose, vertex map and band over the same compact list.  Both move at most 8 KiB per block (4 KiB TSDF in, 2 KiB
                  of words in, at most 2 KiB out); the label launch gathers 2 bytes per voxel from its image, colour 4.
  label sampler   vh_sample_labels against vh_sample_color in nearest mode over the same points -- the voxel positions of the
                  visible blocks, each moved within its cell -- between HIP events on the context's stream.
  counting        vh_label_counts (whole model, 65 536 bins, then a stream synchronisation) and vh_remove_label of a label
                  nobody carries (the whole call: list, pass over every block, read-back, the empty deletion path) against the
                  count-only vh_extract_mesh_indexed, host time around each call: all three list every block and read it once.
  removing        after the cycles, one vh_remove_label of the commonest label, timed once with what it removed.

The label image is coherent in the world, as a segmentation is: the label of a pixel is a function of the half-metre cell
its surface point lies in.  After --warmup cycles, --cycles cycles are recorded: median and minimum per call, and the ratios of
the medians.

  python tools/labels_time.py [--workload C2] [--frames N] [--cycles K] [--warmup W] [--band METRES] [--vote-max N]
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
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--band", type=float, default=0.0, help="label and colour band in metres (0: three voxels)")
    ap.add_argument("--vote-max", type=int, default=8)
    a = ap.parse_args()
    import torch

    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("labels_time.py needs a GPU: there is nothing to time without one")
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
    verts = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")
    nrm = torch.empty((Ht, Wd, 4), dtype=torch.float32, device="cuda")

    def sensor(p):
        z = synth.render_room_verts(p, Wd, Ht, prims, device="cuda")[..., 2]
        return torch.round(z * 5000.0).clamp(0, 65535).to(torch.int32).to(torch.uint16).contiguous()

    def picture():
        return torch.randint(0, 1 << 24, (Ht, Wd), dtype=torch.int32, device="cuda", generator=gen)

    def segmentation(p, d16):
        """Labels 1..20 by the half-metre world cell of the pixel's surface point; 0 where the sensor saw nothing."""
        V.preprocess(d16, kinv, verts, nrm)
        T = torch.from_numpy(np.asarray(p, np.float32).reshape(4, 4)).cuda()
        w = verts[..., :3] @ T[:3, :3].T + T[:3, 3]
        c = torch.floor(w / 0.5).to(torch.int64)
        lab = 1 + (c[..., 0] + 3 * c[..., 1] + 7 * c[..., 2]) % 20
        return torch.where(verts[..., 2] != 0, lab, torch.zeros_like(lab)).to(torch.int16).contiguous()

    for p in poses:
        d16 = sensor(p)
        t.integrate_depth_color(p, d16, kinv, picture(), band)
        t.integrate_labels(p, d16, kinv, segmentation(p, d16), band, a.vote_max)
    t.synchronize()
    pose = poses[len(poses) // 2]
    d16, rgba = sensor(pose), picture()
    seg = segmentation(pose, d16)                         # (leaves the pose's vertex map in `verts`)
    torch.cuda.synchronize()
    t.set_pose(pose)
    visible = t.flatten()
    keys = torch.from_numpy(np.ascontiguousarray(t.compact()["pos"]).astype(np.int64)).cuda()
    i = torch.arange(512, device="cuda")
    local = torch.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    g = (keys[:, None, :] * 8 + local[None, :, :]).reshape(-1, 3).to(torch.float32)
    points = ((g + torch.rand(g.shape, device="cuda", generator=gen) - 0.5) * wl["voxel"]).contiguous()
    words = torch.empty(len(points), dtype=torch.int32, device="cuda")
    col = torch.empty(len(points), dtype=torch.int32, device="cuda")
    counts = torch.empty(65536, dtype=torch.int32, device="cuda")
    print(f"{a.workload}: {n} poses, {len(t.allocated())} blocks, {visible} visible from pose {len(poses) // 2}, {Wd}x{Ht}, "
          f"band {band:g} m, vote_max {a.vote_max}, {len(points)} sample points")
    t.set_profiling(True)

    def host_us(call):
        t.synchronize()
        t0 = time.perf_counter()
        call()
        t.synchronize()
        return 1e6 * (time.perf_counter() - t0)

    rows = []
    for cycle in range(a.warmup + a.cycles):
        t.kernel_times()                                      # (reset)
        t.integrate_labels_map(pose, verts, seg, band, a.vote_max)
        label = t.kernel_times()
        t.integrate_color_map(pose, verts, rgba, band)
        colour = t.kernel_times()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        t.sample_labels_into(points, words)
        e[1].record()
        e[2].record()
        t.sample_color_into(points, col, V.SAMPLE_NEAREST)
        e[3].record()
        torch.cuda.synchronize()
        count_us = host_us(lambda: t.label_counts_into(counts, 65536))
        remove_us = host_us(lambda: t.remove_label(60000))    # (no pixel carried it: nothing is removed, every block is read)
        mesh_us = host_us(lambda: t.mesh_counts())
        if cycle >= a.warmup:
            rows.append((1e3 * label["integrate_ms"], 1e3 * colour["integrate_ms"], 1e3 * e[0].elapsed_time(e[1]),
                         1e3 * e[2].elapsed_time(e[3]), count_us, remove_us, mesh_us))
    r = np.array(rows)
    c = counts.cpu().numpy()
    print(f"  {int(c[1:].sum())} labelled valid voxels of {int(c.sum())} valid, {int((c[1:] != 0).sum())} labels; "
          f"{int((words != 0).sum())} of the points have a label, {int((col != 0).sum())} a colour")
    for name, k in (("label launch", 0), ("colour launch (yardstick)", 1), ("vh_sample_labels", 2), ("vh_sample_color nearest (yardstick)", 3),
                    ("vh_label_counts + sync (host)", 4), ("vh_remove_label, nothing removed (host)", 5),
                    ("vh_extract_mesh_indexed count-only (host, yardstick)", 6)):
        print(f"  {name:52s} median {np.median(r[:, k]):9.1f} us  min {r[:, k].min():9.1f} us  over {len(r)} cycles")
    print(f"  ratio of medians (label launch / colour launch): {np.median(r[:, 0]) / np.median(r[:, 1]):.3f}")
    print(f"  ratio of medians (vh_sample_labels / vh_sample_color nearest): {np.median(r[:, 2]) / np.median(r[:, 3]):.3f}")
    print(f"  ratio of medians (vh_label_counts / mesh count): {np.median(r[:, 4]) / np.median(r[:, 6]):.3f}")
    print(f"  ratio of medians (vh_remove_label / mesh count): {np.median(r[:, 5]) / np.median(r[:, 6]):.3f}")
    top = int(np.argmax(c[1:])) + 1
    t.synchronize()
    t0 = time.perf_counter()
    st = t.remove_label(top)
    once = 1e6 * (time.perf_counter() - t0)
    print(f"  one vh_remove_label of label {top}: {once:.1f} us (host), {st['removed_voxels']} voxels cleared in {st['blocks']} blocks, "
          f"{st['freed_blocks']} blocks freed")


if __name__ == "__main__":
    main()
