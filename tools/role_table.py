#!/usr/bin/env python3
"""flatten_kernel alone, the two-launch frame and the pipelined launch role by role, interleaved in ONE process.

Needs the diagnostics build for the role masks (make EXTRA=-DVH_DEBUG_SKIP_ROLES; VOXELHASH_LIB=<that library>); with the
production library only mask 0 is run.  C2, flatten_variant 3, vh_integrate_batch of 8; per round and walk direction
(option walk_reverse 0 / 1): HIP-event us per launch, median / min / max / spread over the rounds.

    VOXELHASH_LIB=... python tools/role_table.py --out profiles/<name>.txt [--masks 0 3 7 8] [--rounds 10] [--per-round 200]

Masks: bit 0 commit, bit 1 TSDF update, bit 2 claim, bit 3 walk return at once."""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    return f"med {np.median(xs):.3f} min {np.min(xs):.3f} max {np.max(xs):.3f} spread {np.max(xs) - np.min(xs):.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=200)
    ap.add_argument("--masks", type=int, nargs="+", default=[0, 3, 7, 8])
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    import torch
    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import synth
    wl = WORKLOADS["C2"]
    Wd, Ht = wl["width"], wl["height"]
    frames = 60
    dev = torch.device("cuda", 0)
    poses = synth.camera_loop(wl["loop"])[:frames]
    prims = synth.room_primitives()
    verts = [synth.render_room_verts(p, Wd, Ht, prims, device=dev) for p in poses]
    t = V.SDFHashtable(V.default_params(numBuckets=wl["buckets"], numVoxelBlocks=wl["blocks"], voxelSize=wl["voxel"]),
                       Wd, Ht, V.SEM_PINHOLE, stream=torch.cuda.Stream(device=dev))
    t.set_option("flatten_variant", 3)
    for i in range(frames):
        t.integrate(poses[i], verts[i])
    t.synchronize()
    have_skip = True
    try:
        t.set_option("debug_skip_roles", 0)
    except Exception:
        have_skip = False
    res = {}
    B = 8
    for r in range(a.rounds):
        for rev in (0, 1):
            t.set_option("walk_reverse", rev)
            # flatten_kernel alone
            t.set_option("pipeline", 0)
            t.set_profiling(True)
            for i in range(a.per_round):
                t.flatten(sync=False)
            kt = t.kernel_times(reset=True)
            t.set_profiling(False)
            res.setdefault(("flatten_kernel alone", rev), []).append(1e3 * kt["flatten_ms"] / a.per_round)
            # the two-launch frame
            t.set_profiling(True)
            for i in range(a.per_round):
                k = (r * a.per_round + i) % frames
                t.integrate(poses[k], verts[k])
            kt = t.kernel_times(reset=True)
            t.set_profiling(False)
            res.setdefault(("two-launch: launch 1 (scan_claim)", rev), []).append(1e3 * kt["frame_scan_claim_ms"] / kt["launches"])
            res.setdefault(("two-launch: launch 2 (commit_integrate)", rev), []).append(1e3 * kt["frame_commit_integrate_ms"] / kt["launches"])
            # the pipelined launch by role
            t.set_option("pipeline", 1)
            for m in (a.masks if have_skip else [0]):
                if have_skip:
                    t.set_option("debug_skip_roles", m)
                t.set_profiling(True)
                for i in range(0, a.per_round, B):
                    ks = [(r * a.per_round + i + j) % frames for j in range(B)]
                    t.integrate_batch([poses[k] for k in ks], [verts[k] for k in ks])
                kt = t.kernel_times(reset=True)
                t.set_profiling(False)
                res.setdefault((f"skip={m}", rev), []).append(1e3 * kt["frame_pipelined_ms"] / kt["launches"])
            if have_skip:
                t.set_option("debug_skip_roles", 0)
            t.synchronize()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        if a.title:
            f.write(a.title + "\n")
        for (name, rev), xs in res.items():
            line = f"C2 {name} reverse={rev}".ljust(58) + stats(xs)
            print(line)
            f.write(line + "\n")
    print("counters", t.counters())


if __name__ == "__main__":
    main()
