#!/usr/bin/env python3
"""Time of block streaming after a workload's pose loop: every block of the coloured model is streamed out and back in, once per
cycle, in one process.  Reported, as medians and minima over the cycles:

  pack launch          view_export_ms of vh_set_profiling: stream_pack_kernel alone (4 KiB + 2 KiB per block)
  place launch         view_import_ms: stream_place_kernel alone
  device-to-device     hipMemcpyAsync of the same bytes (records and colour words), alternating with the two in the same cycle
  allocation rounds    alloc_claim_ms + alloc_commit_ms of the stream-in: per round the bin claim, the commit and the missing-key count
  whole calls          vh_stream_out and vh_stream_in, device form (HIP events around the call: it synchronises, so the host time
                       between launches is in it) and host form (wall clock: staging copies and the numpy side included)

and the payload, 6 KiB per block, over each launch time as a fraction of the 8 TB/s HBM peak.

  python tools/stream_time.py [--workload C2] [--frames N] [--cycles K]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK = 8e12          # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--frames", type=int, default=0, help="poses fused before the measurement (0: the workload's)")
    ap.add_argument("--cycles", type=int, default=9)
    a = ap.parse_args()
    import torch

    import voxelhashing_demo_amd as V
    from bench import WORKLOADS
    from voxelhashing_demo_amd import streaming, synth
    if not torch.cuda.is_available():
        raise SystemExit("stream_time.py needs a GPU: there is nothing to time without one")
    wl = WORKLOADS[a.workload]
    Wd, Ht = wl["width"], wl["height"]
    n = a.frames or wl["frames"]
    poses = synth.camera_loop(wl.get("loop", wl["frames"]))[:n]
    prims = synth.room_primitives()
    kw = dict(numBuckets=wl["buckets"], numVoxelBlocks=wl["blocks"], voxelSize=wl["voxel"])
    gt = V.SDFHashtable(V.default_params(**kw), Wd, Ht, V.SEM_PINHOLE)
    kinv = np.linalg.inv(synth.K_matrix(Wd, Ht).astype(np.float64)).astype(np.float32)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in poses:
        z = synth.render_room_verts(p, Wd, Ht, prims, device="cuda")[..., 2]
        d16 = torch.round(z * 5000.0).clamp(0, 65535).to(torch.int32).to(torch.uint16).contiguous()
        rgba = torch.randint(0, 1 << 24, (Ht, Wd), dtype=torch.int32, device="cuda", generator=gen)
        gt.integrate_depth_color(p, d16, kinv, rgba, 3.0 * wl["voxel"])
    gt.synchronize()
    everything = streaming.box((-(1 << 31),) * 3, ((1 << 31) - 1,) * 3)
    blocks = gt.stream_count(everything)
    payload = blocks * 6144
    print(f"{a.workload}: {n} poses, {blocks} blocks = {payload / 1e6:.1f} MB of voxels and colour words, {Wd}x{Ht}, voxel {wl['voxel']}")
    records = torch.empty((blocks, 4112), dtype=torch.uint8, device="cuda")
    colors = torch.empty((blocks, 512), dtype=torch.int32, device="cuda")
    records2, colors2 = torch.empty_like(records), torch.empty_like(colors)
    status = torch.empty((blocks,), dtype=torch.int32, device="cuda")
    gt.set_profiling(True)
    rows, st = [], None
    for cycle in range(a.cycles + 1):                        # (cycle 0 warms up: scratch allocation, code load)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        gt.kernel_times()
        e[0].record()
        sel, wr = gt.stream_out_into(everything, blocks, records, colors)
        e[1].record()
        out_kt = gt.kernel_times()
        e[2].record()
        records2.copy_(records)                              # hipMemcpyAsync, device to device, the same bytes
        colors2.copy_(colors)
        e[3].record()
        e[4].record()
        st = gt.stream_in_from(records, blocks, colors, status)
        e[5].record()
        in_kt = gt.kernel_times()
        torch.cuda.synchronize()
        assert (sel, wr) == (blocks, blocks) and st["placed"] == blocks, (sel, wr, st)
        t0 = time.perf_counter()
        chunk = gt.stream_out(everything)
        t1 = time.perf_counter()
        back = gt.stream_in(chunk)
        t2 = time.perf_counter()
        assert len(chunk["keys"]) == blocks and back["placed"] == blocks
        if cycle:
            rows.append((1e3 * out_kt["view_export_ms"], 1e3 * in_kt["view_import_ms"], 1e3 * e[2].elapsed_time(e[3]),
                         1e3 * (in_kt["alloc_claim_ms"] + in_kt["alloc_commit_ms"]), 1e3 * e[0].elapsed_time(e[1]),
                         1e3 * e[4].elapsed_time(e[5]), 1e6 * (t1 - t0), 1e6 * (t2 - t1)))
    r = np.array(rows)
    print(f"  vh_stream_stats of the last stream-in: {st}")
    names = ("pack launch", "place launch", "hipMemcpyAsync D2D (yardstick)", "allocation rounds", "vh_stream_out, device form",
             "vh_stream_in, device form", "stream_out, host form", "stream_in, host form")
    for c, name in enumerate(names):
        med, low = np.median(r[:, c]), r[:, c].min()
        frac = f"  {100 * payload / (med * 1e-6) / PEAK:5.1f} % of 8 TB/s" if c < 3 else ""
        print(f"  {name:32s} median {med:10.1f} us  min {low:10.1f} us  over {len(r)} cycles{frac}")
    gt.close()


if __name__ == "__main__":
    main()
