#!/usr/bin/env python3
"""Time of vh_components and vh_remove_components after a workload's pose loop, in-process and warm, with HIP events around the
call: the inside components at connectivity 6 and at 14, next to a count-only vh_extract_mesh_indexed over the same model
(it walks the same block list and stages the same aprons).  The calls alternate, round by round; medians and minima of
--rounds.  The stages of the labelling are separated with the diagnostics option "components_launches" (the call stops behind
its first k stages): stage k = the k-stage call minus the (k - 1)-stage call, medians of alternating rounds.  Every call
synchronises, so each figure includes one read-back of the stats.  vh_remove_components(min_size) is timed last: the first
call (it clears and frees) and the median of the calls after it (they find nothing to remove).

  python tools/components_time.py [--workload C2] [--frames N] [--rounds R] [--min-size 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("block list (+ 3 memsets)", "local pass", "seam pass", "flatten", "count", "scan + records")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-size", type=int, default=64)
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
    blocks = len(t.allocated())
    print(f"{a.workload}: {n} poses, {blocks} blocks, voxel {t.params.voxelSize} m")

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    def comp(conn, k=0):
        t.set_option("components_launches", k)
        return t.components_into(0, None, target="inside", connectivity=conn)

    mesh = lambda: t.mesh_counts()
    mesh()
    for conn in (6, 14):
        stats = comp(conn)
        for k in range(1, 7):
            comp(conn, k)
        us = np.array([[one(mesh)] + [one(lambda k=k: comp(conn, k)) for k in range(1, 7)] + [one(lambda: comp(conn))]
                       for _ in range(a.rounds)])
        t.set_option("components_launches", 0)
        med, best = np.median(us, 0), us.min(0)
        print(f"  inside, connectivity {conn}: nodes {stats['nodes']}, components {stats['components']}, largest {stats['largest']}")
        print(f"    vh_extract_mesh_indexed, count only  median {med[0]:9.1f} us  min {best[0]:9.1f} us")
        for k, name in enumerate(STAGES):
            m = med[k + 1] - (med[k] if k else 0.0)
            b = best[k + 1] - (best[k] if k else 0.0)
            print(f"    {name:36s} median {m:9.1f} us  min {b:9.1f} us" + ("   (with the read-back)" if k == 0 else ""))
        print(f"    whole call, count only               median {med[7]:9.1f} us  min {best[7]:9.1f} us  "
              f"ratio to the mesh count (medians) {med[7] / med[0]:.2f}")
    first_stats = {}
    first = one(lambda: first_stats.update(t.remove_components(a.min_size)))
    rest = np.array([one(lambda: t.remove_components(a.min_size)) for _ in range(a.rounds)])
    print(f"  vh_remove_components(min_size={a.min_size}), inside at 14: removed {first_stats['removed_components']} components, "
          f"{first_stats['removed_voxels']} voxels, freed {first_stats['freed_blocks']} blocks")
    print(f"    first call {first:9.1f} us;  calls after it  median {np.median(rest):9.1f} us  min {rest.min():9.1f} us")
    t.close()


if __name__ == "__main__":
    main()
