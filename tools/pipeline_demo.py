#!/usr/bin/env python3
"""The whole reconstruction loop of the demo on synthetic sensor data, every stage on the GPU
through the C-ABI: uint16 depth -> vertex/normal maps (preProcess) -> pose from frame-to-model ICP
against a raycast of the model (CameraTracking::Align; bypassed in the reference, Application.cpp:75)
-> TSDF integration (SDF_Hashtable::integrate) -> periodic garbage collection.  Prints the time per
stage and the drift against the true trajectory; --mesh writes the fused model as a triangle mesh at the end
(welded by position on the host), --mesh-indexed the indexed mesh the GPU makes (one vertex per cell edge).  --color fuses a
synthetic colour image with every frame (vh_integrate_color_map, a band of three voxels); --snapshot writes the model at the end
(vh_save_snapshot) and, where the model is coloured, its colour words beside it as <path>.color (vh_save_color): the pair
load_snapshot + load_color resumes from.  --tracker sdf-color (with --color) takes the pose from the model's own distance field and
colour instead of a raycast and the ICP (vh_sdf_color_align): the model is then fused with a truncation of three voxels, which
that tracker is for, and the colour images are a texture fixed to the scene instead of noise.  --stream-radius R keeps only the blocks within R metres of the camera on the GPU: after
every frame a streaming.BlockStore moves the blocks beyond R to the host and those within 0.8 R back (vh_stream_out / vh_stream_in);
at the end every stored block is streamed back in, so a mesh or snapshot holds the whole model.  R should exceed the depth range:
a block the camera still sees beyond R is allocated again by the next frame and streamed out again, replacing its stored record.
--esdf out.npy writes the Euclidean signed distance to the surface (metres, float32 [z, y, x]; vh_esdf_lattice) over the bounding
box of the model's blocks, up to --esdf-radius voxels (default 16), unknown voxels kept unknown (NaN).
--min-component N takes the floaters out before --mesh, --mesh-indexed, --esdf and --snapshot: every inside component (at
connectivity 14, the mesh's own) with fewer than N voxels is cleared out of the volume and the blocks that emptied are freed
(vh_remove_components); the stats are printed.
--mesh-live out.ply keeps a meshing.MeshCache across the run: after every frame (and whatever collected, streamed or removed
blocks) one update() re-meshes only the blocks vh_changes lists (vh_extract_mesh_blocks); its final state is written, three
vertices per triangle with normals, blocks in ascending key order.
tools/pipeline_demo.py [frames] [--mesh out.ply] [--mesh-indexed out.ply] [--mesh-live out.ply] [--color]
                       [--tracker icp|sdf-color] [--snapshot out.vhsnap] [--stream-radius R]
                       [--esdf out.npy] [--esdf-radius R] [--min-component N]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import voxelhashing_demo_amd as V
from voxelhashing_demo_amd import synth, tracking

W, H = 640, 480
argv = sys.argv[1:]
MESH = MESH_INDEXED = None
if "--mesh-indexed" in argv:
    MESH_INDEXED = argv[argv.index("--mesh-indexed") + 1]
    del argv[argv.index("--mesh-indexed"):argv.index("--mesh-indexed") + 2]
MESH_LIVE = None
if "--mesh-live" in argv:
    MESH_LIVE = argv[argv.index("--mesh-live") + 1]
    del argv[argv.index("--mesh-live"):argv.index("--mesh-live") + 2]
if "--mesh" in argv:
    MESH = argv[argv.index("--mesh") + 1]
    del argv[argv.index("--mesh"):argv.index("--mesh") + 2]
COLOR = "--color" in argv
if COLOR:
    argv.remove("--color")
TRACKER = "icp"
if "--tracker" in argv:
    TRACKER = argv[argv.index("--tracker") + 1]
    del argv[argv.index("--tracker"):argv.index("--tracker") + 2]
if TRACKER not in ("icp", "sdf-color") or (TRACKER == "sdf-color" and not COLOR):
    raise SystemExit("--tracker is icp or sdf-color, and sdf-color needs --color")
SNAPSHOT = None
if "--snapshot" in argv:
    SNAPSHOT = argv[argv.index("--snapshot") + 1]
    del argv[argv.index("--snapshot"):argv.index("--snapshot") + 2]
STREAM_RADIUS = None
if "--stream-radius" in argv:
    STREAM_RADIUS = float(argv[argv.index("--stream-radius") + 1])
    del argv[argv.index("--stream-radius"):argv.index("--stream-radius") + 2]
ESDF, ESDF_RADIUS = None, 16
if "--esdf-radius" in argv:
    ESDF_RADIUS = int(argv[argv.index("--esdf-radius") + 1])
    del argv[argv.index("--esdf-radius"):argv.index("--esdf-radius") + 2]
if "--esdf" in argv:
    ESDF = argv[argv.index("--esdf") + 1]
    del argv[argv.index("--esdf"):argv.index("--esdf") + 2]
MIN_COMPONENT = 0
if "--min-component" in argv:
    MIN_COMPONENT = int(argv[argv.index("--min-component") + 1])
    del argv[argv.index("--min-component"):argv.index("--min-component") + 2]
N = int(argv[0]) if argv else 60
gt = synth.camera_loop(500)[200:200 + N]
prims = synth.room_primitives()
K = synth.K_matrix(W, H)
kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
# synthetic sensor frames: depth in 1/5000 m, as the TUM sequences the demo reads (Application.cpp:38-42)
depth16 = [(synth.render_room_verts(p, W, H, prims, device="cuda")[..., 2] * 5000.0).round().clamp(0, 65535).to(torch.uint16)
           for p in gt]
torch.cuda.synchronize()           # the sensor frames were made on torch's default stream
stream = torch.cuda.Stream()
extra = dict(truncation=0.06) if TRACKER == "sdf-color" else {}
table = V.SDFHashtable(V.default_params(numBuckets=1 << 20, numVoxelBlocks=1 << 16, **extra), W, H, V.SEM_PINHOLE, stream=stream)
trk = tracking.CameraTracking(W, H, K, stream=stream, flags=tracking.ICP_ABS_DISTANCE | tracking.ICP_NEED_TARGET)
verts, normals = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 4), device="cuda")
tp, tn = torch.empty_like(verts), torch.empty_like(verts)
ray = torch.empty((H, W), device="cuda")
stage = dict(preprocess=0.0, raycast_target=0.0, align=0.0, integrate=0.0, collect=0.0)
store = None
if STREAM_RADIUS is not None:
    from voxelhashing_demo_amd import streaming
    store = streaming.BlockStore(table.params.voxelSize)
    stage["stream"] = 0.0
    streamed = dict(out=0, back=0, most=0)
cache = None
if MESH_LIVE:
    from voxelhashing_demo_amd import meshing
    with torch.cuda.stream(stream):
        cache = meshing.MeshCache(table, normals=True)
    stage["mesh_live"] = 0.0
    live = dict(extracted=0, removed=0, allocated=0)
if COLOR:
    stage["color"] = 0.0
    BAND = 3.0 * table.params.voxelSize
    paint = torch.Generator(device="cuda").manual_seed(1)
    if TRACKER == "sdf-color":
        def textured(p):
            """The colour image of pose p: a smooth texture of the world position each pixel sees."""
            v = synth.render_room_verts(p, W, H, prims, device="cuda")
            T = torch.as_tensor(np.asarray(p, np.float32).reshape(4, 4), device="cuda")
            x, y, z = (v[..., :3] @ T[:3, :3].T + T[:3, 3]).unbind(-1)
            r = 128 + 100 * torch.sin(7.0 * x + 3.0 * z + 0.3) * torch.cos(5.0 * y)
            g = 128 + 100 * torch.sin(4.0 * x - 6.0 * y + 5.0 * z + 1.0)
            b = 128 + 100 * torch.cos(6.5 * y - 0.7) * torch.cos(3.0 * x - 4.0 * z + 0.2)
            r, g, b = (c.round().to(torch.int32) for c in (r, g, b))
            return (r | (g << 8) | (b << 16)).contiguous()
        rgba = [textured(p) for p in gt]
        ctrk = tracking.SdfColorTracking(table, K=K, stream=stream)
    else:
        rgba = [torch.randint(0, 1 << 24, (H, W), dtype=torch.int32, device="cuda", generator=paint) for _ in range(N)]
    torch.cuda.synchronize()


def timed(name, fn):
    stream.synchronize()
    t = time.perf_counter()
    fn()
    stream.synchronize()
    stage[name] += time.perf_counter() - t


pose = np.asarray(gt[0], np.float64).reshape(4, 4)
errs = []
with torch.cuda.stream(stream):
    for k in range(N):
        timed("preprocess", lambda: V.preprocess(depth16[k], kinv, verts, normals, stream=stream))
        if k > 0 and TRACKER == "sdf-color":
            found = [None]
            timed("align", lambda: found.__setitem__(0, ctrk.Align(verts, rgba[k], pose)))
            pose = found[0].copy()
        elif k > 0:
            def target():
                table.raycast(pose.astype(np.float32), ray)
                tracking.depth_to_maps(ray, kinv, tp, tn, stream=stream)
            timed("raycast_target", target)
            delta = [None]
            timed("align", lambda: delta.__setitem__(0, trk.Align(verts, tp, tn)))
            pose = pose @ delta[0].astype(np.float64)
        timed("integrate", lambda: table.integrate(pose.astype(np.float32), verts))
        if COLOR:
            timed("color", lambda: table.integrate_color_map(pose.astype(np.float32), verts, rgba[k], BAND))
        if k % 20 == 19:
            timed("collect", lambda: table.garbage_collect(0.5))
        if store is not None:
            moved = [None]
            timed("stream", lambda: moved.__setitem__(0, store.update(table, pose[:3, 3], 0.8 * STREAM_RADIUS, STREAM_RADIUS)))
            streamed["out"] += moved[0]["out"]
            streamed["back"] += moved[0]["in"]
            streamed["most"] = max(streamed["most"], moved[0]["stored"])
        if cache is not None:
            did = [None]
            timed("mesh_live", lambda: did.__setitem__(0, cache.update()))
            live["extracted"] += did[0]["extracted"]
            live["removed"] += did[0]["removed"]
            live["allocated"] += len(cache.blocks)
        errs.append(float(np.abs(pose[:3, 3] - np.asarray(gt[k], np.float64).reshape(4, 4)[:3, 3]).max()))
travel = float(np.linalg.norm(np.asarray(gt[-1], np.float64).reshape(4, 4)[:3, 3] - np.asarray(gt[0], np.float64).reshape(4, 4)[:3, 3]))
print(f"{N} frames, {travel:.2f} m between first and last camera, blocks {table.counters()['allocated_total']}")
for name, t in stage.items():
    n = N - 1 if name in ("raycast_target", "align") else (N // 20 if name == "collect" else N)
    print(f"  {name:15s} {1e6 * t / max(1, n):8.1f} us per call (host-timed, synchronised)")
print(f"  drift: max {1e3 * max(errs):.2f} mm, final {1e3 * errs[-1]:.2f} mm")
if store is not None:
    with torch.cuda.stream(stream):
        left = store.restore_all(table)
    print(f"  streaming: radius {STREAM_RADIUS} m, {streamed['out']} blocks out and {streamed['back']} back during the loop, at most "
          f"{streamed['most']} on the host; at the end {left['placed']} restored, {left['present']} met a block allocated again "
          f"under their key meanwhile (kept in the store), {left['unplaced']} unplaced")
if MIN_COMPONENT:
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        removed = table.remove_components(MIN_COMPONENT)
        dt = time.perf_counter() - t0
    print(f"components: blocks={removed['blocks']} inside voxels={removed['nodes']} components={removed['components']} "
          f"largest={removed['largest']}; below {MIN_COMPONENT} voxels: {removed['removed_components']} components, "
          f"{removed['removed_voxels']} voxels removed, {removed['freed_blocks']} blocks freed ({1e3 * dt:.1f} ms)")
if MESH_LIVE:
    from voxelhashing_demo_amd import mesh_io
    with torch.cuda.stream(stream):
        last = cache.update()                     # what the restore and the component removal above changed
    lp, ln = cache.triangles()
    mesh_io.save_ply(MESH_LIVE, lp.reshape(-1, 3), np.arange(3 * len(lp), dtype=np.int32).reshape(-1, 3), ln.reshape(-1, 3))
    print(f"mesh live: triangles={len(lp)} in {len(cache.blocks)} blocks; {live['extracted']} block extractions over {N} updates "
          f"where re-meshing every block each time would be {live['allocated']}, {live['removed']} blocks dropped; the last "
          f"update re-meshed {last['extracted']} -> {MESH_LIVE}")
if MESH:
    from voxelhashing_demo_amd import mesh_io
    with torch.cuda.stream(stream):
        count = table.mesh_count()
        t0 = time.perf_counter()
        mv, mf, mn = table.extract_mesh(normals=True, weld=True)
        dt = time.perf_counter() - t0
    mesh_io.save_ply(MESH, mv, mf, mn)
    print(f"mesh: triangles={count} vertices={len(mv)} ({1e3 * dt:.1f} ms with download and welding) -> {MESH}")
if MESH_INDEXED:
    from voxelhashing_demo_amd import mesh_io
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        mv, mf, mn = table.extract_mesh_indexed(normals=True)
        dt = time.perf_counter() - t0
    mesh_io.save_ply(MESH_INDEXED, mv, mf, mn)
    print(f"mesh indexed: triangles={len(mf)} vertices={len(mv)} ({1e3 * dt:.1f} ms with download) -> {MESH_INDEXED}")
if ESDF:
    keys = table.allocated()["pos"].astype(np.int64)
    lo = keys.min(0) * 8
    dims = (keys.max(0) + 1) * 8 - lo
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        dist = table.esdf_lattice(lo, dims, ESDF_RADIUS).cpu().numpy()
        dt = time.perf_counter() - t0
    np.save(ESDF, dist)
    known = ~np.isnan(dist)
    print(f"esdf: lo={tuple(int(v) for v in lo)} dims={tuple(int(v) for v in dims)} radius {ESDF_RADIUS} voxels, "
          f"{known.mean():.3f} of the voxels known, {np.isfinite(dist).mean():.3f} with a distance "
          f"({1e3 * dt:.1f} ms with download) -> {ESDF}")
if SNAPSHOT:
    table.save_snapshot(SNAPSHOT)
    print(f"snapshot -> {SNAPSHOT}")
    if table.has_color():
        table.save_color(SNAPSHOT + ".color")
        print(f"colour words -> {SNAPSHOT}.color (load_snapshot, then load_color)")
