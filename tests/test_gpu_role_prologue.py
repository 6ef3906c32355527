"""The pipelined launch reads its arguments role by role (vh_frame.hip: PipeLead, role_arguments): a workgroup decides its
role from the leading 64 bytes, a walk workgroup loads its ptr words from those alone, and `live` -- is the pending frame's
commit phase inserting or refusing? -- is asked inside each role, by the walk only in a wave that found an allocated entry.
None of that may change what a frame computes.

Every case feeds the same frames to a table at "pipeline" 1 (vh_integrate_batch, in runs of 1, 2 and 5 frames: a run of 1
is a first launch and a flush launch and nothing else) and to a twin at "pipeline" 0, and compares table, voxels, compact
set and counters of the two after every run, and with the oracle's snapshot of that frame.

Shapes, the smallest at which a moved evaluation can go wrong: images of 16x16 (one claim tile, which in a run's first
launch also leaves the free-block count for the next) and 64x48; tables of 2^8, 2^10 and 2^13 buckets x 5, that is 2, 5 and
40 walk tiles of 1024 entries, so that the last group of 8 has surplus workgroups and, at 2^8, a tile that reaches beyond the
last entry; bucket size 10 once; the generic build ("walk_short" 0: no lean build has those flags).  "walk_reverse" 0 and 1,
both input forms, the ray-DDA band (its lean builds), "walk_nt" 1.

Two sequences ask whether `live` still means the same in each role:
* a frame that allocates nothing behind one that does (asserted from the oracle's own statistics): walk workgroups that find
  no allocated entry beside ones that do, with an insertion in flight;
* a heap of 48 blocks: frames that are refused as a whole (`live` false, every winner counted as heap_exhausted) between
  frames that are served.  A refused frame is where the pipelined frame differs from vh_integrate BY DESIGN (it serves as
  many winners as there are blocks; test_gpu_pipeline.py: test_heap_shortage_refuses_whole_frames), so there the twin at
  "pipeline" 0 is no reference: the oracle is, stepped by hand -- a refused frame walks and updates but does not allocate --
  with the refusals decided from the oracle's own counts (winners of the frame against free blocks before it)."""
import numpy as np
import pytest

from conftest import entries_as_set
from test_gpu_parity import _compare, blocks_by_pos
from test_gpu_walk_order import _Snapshot, feed, kinv_of
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
I4 = np.eye(4, dtype=np.float32)
RUNS = (1, 2, 5)                      # frames per vh_integrate_batch call, in this order: 8 frames per case
BAND_RAY_DDA = 2                      # VH_BAND_RAY_DDA (include/voxelhash.h)
COUNTERS = ("occupied", "allocated_total", "freed_total", "heap_counter", "heap_exhausted", "cand_overflow", "bin_overflow",
            "spin_timeouts")

_oracle_runs = {}                     # the oracle's frames of a case, computed once (the two most recent are kept)


VOXEL = 0.04                          # a few dozen blocks per frame at these image sizes
# 8 frames each.  S: the sphere around the camera; R<i>: pose i of the room's camera loop.
# PLAIN: a pose repeated inserts less and less (the mutex lets one insertion per bucket through per frame) and then nothing.
# HEAP (48 blocks): S fits, R0 does not, S again fits (what its first frame left over, then nothing) ...
PLAIN = ("S", "S", "R0", "R0", "R0", "R0", "R3", "R40")
HEAP = ("S", "R0", "S", "R0", "S", "S", "R3", "S")


def frames_of(W, H, order):
    poses, prims = synth.camera_loop(500), synth.room_primitives()
    made = {"S": (I4, synth.sphere_inside_scene(W, H))}
    for name in set(order) - {"S"}:
        i = int(name[1:])
        made[name] = (poses[i], synth.render_room_verts(poses[i], W, H, prims).numpy())
    return [made[name] for name in order]


def given_of(oracle, verts, W, H, sensor):
    """-> (what the GPU is handed, the vertex map the oracle integrates)"""
    if not sensor:
        return np.ascontiguousarray(verts), verts
    raw = np.round(verts[..., 2] * 5000.0).clip(0, 65535).astype(np.uint16)
    return np.ascontiguousarray(raw), oracle.preprocess(raw, kinv_of(W, H))[0]


def oracle_run(oracle, W, H, kw, sensor=False, band=0.0, heap_refusals=False):
    """[(pose, input, snapshot, stats)] per frame.  heap_refusals: the pipelined frame's rule -- a frame whose winners
    outnumber the free blocks is refused as a whole -- stepped by hand on the oracle; stats then carries `refused`."""
    order = HEAP if heap_refusals else PLAIN
    key = (W, H, tuple(sorted(kw.items())), sensor, band, heap_refusals)
    if key in _oracle_runs:
        return _oracle_runs[key]

    def table():
        t = oracle.OracleTable(oracle.default_params(**kw), W, H, 1)
        if band:
            t.set_alloc_band(band, BAND_RAY_DDA)
        return t

    def step(t, pose, verts, refused):
        if not refused:
            t.integrate(pose, verts)
            return dict(t.last_stats)
        t.set_pose(pose)                  # walk and TSDF update of what is there; nothing is allocated
        t.flatten()
        t.integrate_depth_map(verts)
        return None

    frames = [(pose,) + given_of(oracle, verts, W, H, sensor) for pose, verts in frames_of(W, H, order)]
    refused, winners = [], []
    for i in range(len(frames) if heap_refusals else 0):
        # the decision for frame i needs its winners on the table frames 0 .. i-1 left: replayed on a fresh oracle (tiny frames)
        t = table()
        for j in range(i):
            step(t, frames[j][0], frames[j][2], refused[j])
        free = t.heap_counter() + 1
        st = step(t, frames[i][0], frames[i][2], False)
        winners.append(st["inserted"] + st["heap_exhausted"])       # (what a refused frame counts as heap_exhausted)
        refused.append(winners[i] > free)
        t.close()
    if not heap_refusals:
        refused, winners = [False] * len(frames), [None] * len(frames)
    ot, out = table(), []
    for (pose, given, verts), r, w in zip(frames, refused, winners):
        stats = step(ot, pose, verts, r) or {}
        stats.update(refused=r, winners=w)
        out.append((pose, given, _Snapshot(ot), stats))
    ot.close()
    while len(_oracle_runs) >= 2:
        _oracle_runs.pop(next(iter(_oracle_runs)))
    _oracle_runs[key] = out
    return out


def make_table(vh, W, H, kw, reverse, walk_nt, band, options=()):
    gt = vh.SDFHashtable(vh.default_params(**kw), W, H, 1)
    gt.set_option("flatten_variant", 3)
    gt.set_option("walk_nt", walk_nt)
    gt.set_option("walk_reverse", reverse)
    if band:
        gt.set_option("band_mode", BAND_RAY_DDA)
        gt.set_alloc_band(band)
    for name, value in options:
        gt.set_option(name, value)
    return gt


def same_model(a, b):
    """two GPU tables hold the same model: table, voxels (bit for bit, by block key), compact set, counters"""
    ta, tb = a.hash_table(), b.hash_table()
    assert np.array_equal(ta["ptr"] != -1, tb["ptr"] != -1)
    assert np.array_equal(ta["pos"], tb["pos"]) and np.array_equal(ta["offset"], tb["offset"])
    ca, cb = a.compact(), b.compact()
    assert len(ca) == len(cb) and entries_as_set(ca) == entries_as_set(cb) and len(entries_as_set(ca)) == len(ca)
    va, vb = blocks_by_pos(ta[ta["ptr"] != -1], a.sdf_blocks()), blocks_by_pos(tb[tb["ptr"] != -1], b.sdf_blocks())
    assert va.keys() == vb.keys()
    for pos in va:
        assert np.array_equal(va[pos].view(np.uint32), vb[pos].view(np.uint32)), f"block {pos} differs in bits"
    na, nb = a.counters(), b.counters()
    assert {k: na[k] for k in COUNTERS} == {k: nb[k] for k in COUNTERS}


def run_case(oracle, vh, torch, W, H, kw, reverse=1, sensor=False, walk_nt=0, band=0.0, options=()):
    seq = oracle_run(oracle, W, H, kw, sensor, band)
    inserted = [s[3]["inserted"] for s in seq]
    assert any(a > 0 and b == 0 for a, b in zip(inserted, inserted[1:])), f"no frame that allocates nothing behind one that does: {inserted}"
    assert all(s[3]["heap_exhausted"] == 0 for s in seq)
    piped, twin = (make_table(vh, W, H, kw, reverse, walk_nt, band, options) for _ in range(2))
    try:
        at = 0
        for n in RUNS:
            part = [tuple(s) for s in seq[at:at + n]]
            at += n
            feed(piped, torch, W, H, part, "pipelined", sensor)
            feed(twin, torch, W, H, part, "two_launch", sensor)
            _compare(seq[at - 1][2], piped)
            same_model(piped, twin)
        assert at == len(seq) and piped.counters()["spin_timeouts"] == 0
    finally:
        piped.close()
        twin.close()


def kw_of(log2_buckets, blocks=2048, **more):
    return dict(numBuckets=1 << log2_buckets, numVoxelBlocks=blocks, voxelSize=VOXEL, **more)


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("log2_buckets", [8, 10, 13])
@pytest.mark.parametrize("size", [(16, 16), (64, 48)])
def test_shapes(oracle, vh, torch_cuda, size, log2_buckets, reverse):
    """2, 5 and 40 walk tiles under 1 and 12 claim tiles, the walk always forward and alternating."""
    assert -(-(5 << log2_buckets) // 1024) == {8: 2, 10: 5, 13: 40}[log2_buckets]
    run_case(oracle, vh, torch_cuda, size[0], size[1], kw_of(log2_buckets), reverse=reverse)


@pytest.mark.parametrize("size", [(16, 16), (64, 48)])
def test_sensor_image(oracle, vh, torch_cuda, size):
    run_case(oracle, vh, torch_cuda, size[0], size[1], kw_of(10), sensor=True)


@pytest.mark.parametrize("sensor", [False, True])
def test_non_temporal_walk(oracle, vh, torch_cuda, sensor):
    """"walk_nt" 1: the lean builds of a table beyond the Infinity Cache, on a table of 5 tiles"""
    run_case(oracle, vh, torch_cuda, 64, 48, kw_of(10), sensor=sensor, walk_nt=1)


@pytest.mark.parametrize("walk_nt", [0, 1])
def test_ray_dda_band(oracle, vh, torch_cuda, walk_nt):
    """the band on: lean builds 3 / 4"""
    run_case(oracle, vh, torch_cuda, 64, 48, kw_of(10, blocks=8192), band=0.1, walk_nt=walk_nt)


def test_bucket_size_10(oracle, vh, torch_cuda):
    """2^9 buckets x 10 = the 5 tiles of 2^10 x 5; a listed entry's bucket (the claim word the walk looks up) is e / 10"""
    run_case(oracle, vh, torch_cuda, 64, 48, kw_of(9, bucketSize=10))


@pytest.mark.parametrize("log2_buckets", [8, 10])
def test_generic_build(oracle, vh, torch_cuda, log2_buckets):
    """"walk_short" 0: no lean build has these flags, so the generic one runs -- it reads the flags word before its loads
    -- with 8 entries per lane: 1 and 3 tiles of 2048 entries, the last one beyond the table's end"""
    run_case(oracle, vh, torch_cuda, 64, 48, kw_of(log2_buckets), options=(("walk_short", 0),))


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("size", [(16, 16), (64, 48)])
def test_heap_of_48_blocks(oracle, vh, torch_cuda, size, reverse):
    """Refused frames between served ones: against the oracle stepped by the pipelined frame's rule (module docstring)."""
    W, H = size
    kw = kw_of(10, blocks=48)
    seq = oracle_run(oracle, W, H, kw, heap_refusals=True)
    refused = [s[3]["refused"] for s in seq]
    assert any(refused) and not refused[0], refused
    assert any(a and not b for a, b in zip(refused, refused[1:])), f"no served frame behind a refused one: {refused}"
    gt = make_table(vh, W, H, kw, reverse, 0, 0.0)
    try:
        at, exhausted = 0, 0
        for n in RUNS:
            part = [tuple(s) for s in seq[at:at + n]]
            exhausted += sum(s[3]["winners"] if s[3]["refused"] else s[3]["heap_exhausted"] for s in seq[at:at + n])
            at += n
            feed(gt, torch_cuda, W, H, part, "pipelined", False)
            _compare(seq[at - 1][2], gt)
            c = gt.counters()
            assert c["heap_exhausted"] == exhausted and c["spin_timeouts"] == 0
    finally:
        gt.close()
