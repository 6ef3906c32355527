#!/usr/bin/env python3
"""Time of vh_extract_mesh after a workload's pose loop, in-process and warm, with HIP events around the call: count-only,
positions, positions + normals, for the 9^3-apron kernels (mesh_variant 0) and the direct-from-global ones (1); triangles,
Mtriangles/s, and the share of the byte floor (allocated blocks x 4 KB read + triangles x 36 B written, x 2 with normals)
at --hbm TB/s (tools/micro/membw).  gc_identify_kernel, which also reads every listed block once, is timed beside it on the
same table (the blocks of the last frame's compact list).  Then vh_extract_mesh_indexed on the same table: count only,
vertices + indices, with normals (byte floor: blocks x 4 KB per pass + 12 B per vertex, x 2 with normals, + 12 B per
triangle), and end to end on the host clock, download included: extract_mesh_indexed() against extract_mesh(weld=True).

  python tools/mesh_time.py [--workload C2|C3] [--frames N] [--rounds R] [--hbm 4.0]
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--weld-rounds", type=int, default=3, help="rounds of the host weld (a sort of every vertex row)")
    ap.add_argument("--hbm", type=float, default=4.0, help="measured HBM rate of the box, TB/s")
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
    blocks = int((t.hash_table()["ptr"] != -1).sum())
    count = t.mesh_count()
    pos = torch.empty((count, 3, 3), dtype=torch.float32, device="cuda")
    nrm = torch.empty((count, 3, 3), dtype=torch.float32, device="cuda")
    print(f"{a.workload}: {n} poses, {blocks} blocks, {count} triangles ({count / max(1, blocks):.1f} per block)")

    def timed(fn):
        fn()
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms))

    for variant, name in ((0, "apron in LDS"), (1, "direct from global")):
        t.set_option("mesh_variant", variant)
        for label, fn, out_bytes in (("count only", lambda: t.mesh_count(), 0),
                                     ("positions", lambda: t.extract_mesh_into(count, pos), 36 * count),
                                     ("positions + normals", lambda: t.extract_mesh_into(count, pos, nrm), 72 * count)):
            med, best = timed(fn)
            floor_ms = (blocks * 4096 * (2 if out_bytes else 1) + out_bytes) / (a.hbm * 1e12) * 1e3
            print(f"  {name:20s} {label:20s} median {med:8.3f} ms  min {best:8.3f} ms  {count / med / 1e3:8.1f} Mtri/s  "
                  f"byte floor {floor_ms:.4f} ms = {100 * floor_ms / med:.1f} %  ({1e6 * med / max(1, blocks):.1f} ns per block)")
    t.set_option("mesh_variant", 0)
    nv, nt = t.mesh_counts()
    assert nt == count
    vtx = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    vnr = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    print(f"  indexed: {nv} vertices ({nv / max(1, nt):.3f} per triangle)")
    for label, fn, out_bytes in (("count only", lambda: t.mesh_counts(), 0),
                                 ("vertices + indices", lambda: t.extract_mesh_indexed_into(nv, nt, vtx, idx), 12 * nv + 12 * nt),
                                 ("with normals", lambda: t.extract_mesh_indexed_into(nv, nt, vtx, idx, vnr), 24 * nv + 12 * nt)):
        med, best = timed(fn)
        floor_ms = (blocks * 4096 * (2 if out_bytes else 1) + out_bytes) / (a.hbm * 1e12) * 1e3
        print(f"  {'indexed':20s} {label:20s} median {med:8.3f} ms  min {best:8.3f} ms  {count / med / 1e3:8.1f} Mtri/s  "
              f"byte floor {floor_ms:.4f} ms = {100 * floor_ms / med:.1f} %  ({1e6 * med / max(1, blocks):.1f} ns per block)")
    # end to end, download included, on the host clock: the GPU's indexed mesh against the weld by position on the host
    import time

    def wall(fn, rounds):
        s = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            s.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(s)), float(min(s))
    for label, fn, rounds in (("extract_mesh_indexed()", lambda: t.extract_mesh_indexed(), a.rounds),
                              ("extract_mesh_indexed(normals=True)", lambda: t.extract_mesh_indexed(normals=True), a.rounds),
                              ("extract_mesh(weld=True)", lambda: t.extract_mesh(weld=True), a.weld_rounds)):
        fn()
        med, best = wall(fn, rounds)
        print(f"  end to end {label:36s} median {med:10.3f} ms  min {best:10.3f} ms  ({rounds} rounds)")
    # the neighbour: one read of every block of the last frame's compact list
    t.integrate(poses[-1], synth.render_room_verts(poses[-1], Wd, Ht, prims, device="cuda"))
    seen = t.counters()["occupied"]
    t.set_profiling(True)
    t.kernel_times(reset=True)
    t.garbage_collect(1e9)                        # a threshold nothing reaches: identify reads, nothing is freed
    kt = t.kernel_times(reset=True)
    print(f"  vh_garbage_collect (identify + sweep + release, {seen} blocks of the last frame): {kt['gc_ms']:.3f} ms "
          f"= {1e6 * kt['gc_ms'] / max(1, seen):.1f} ns per block")


if __name__ == "__main__":
    main()
