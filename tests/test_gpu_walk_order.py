"""The reference's table walk in groups of 8 workgroups, forward in one launch and backward in the next (vh_walk.hip:
walk_tile, vh_frame.hip: grouped_role; option "walk_reverse"): whatever the order, every tile is walked exactly once per
frame and every claim tile is served exactly once, so table, compact set and voxels stay the oracle's.

Tables of 1, 2, 7, 8, 9 and 17 walk tiles in both tile widths (1024 entries with 4 per lane, 2048 with 8: option
"walk_short"), images of 1, 6, 15 and 80 claim tiles, the pipelined launch, the two-launch frame and the step kernels.

Before the GPU is compared the ORACLE's table is asked, on the host, whether every walk tile holds an entry that was in
the table before the frame and is visible in it: a tile the walk skipped then shows as a block that was not updated.  (A
tile walked twice lists its entries twice: _compare's duplicate check.)  The first frame meets an empty table and is
exempt."""
import numpy as np
import pytest

from conftest import entries_as_set
from test_gpu_parity import _compare
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
I4 = np.eye(4, dtype=np.float32)
ROOM = (0, 1, 2, 3, 8, 9, 10)          # poses of the camera loop behind the two sphere frames: 9 frames, batches of 3 end on 2, 5, 8
BLOCKS = 1024                          # voxel blocks: the sequence allocates fewer than 500


class _Snapshot:
    """What _compare asks of an OracleTable, as it was after one frame."""

    def __init__(self, ot):
        self._t, self._c, self._v, self._h = ot.hash_table().copy(), ot.compact().copy(), ot.sdf_blocks().copy(), ot.heap_counter()

    def hash_table(self): return self._t
    def compact(self): return self._c
    def sdf_blocks(self): return self._v
    def heap_counter(self): return self._h


_sequences = {}            # the oracle's run of a sequence, computed once (the two most recent are kept)


def kinv_of(W, H):
    return np.linalg.inv(synth.K_matrix(W, H).astype(np.float64)).astype(np.float32)


def sequence(oracle, W, H, buckets, overflow=False, sensor=False):
    """[(pose, input, snapshot, slots)]: input = the vertex map or (sensor) the uint16 image; slots = table slots that were
    allocated BEFORE the frame and are on its compact list (what the walk has to find)."""
    key = (W, H, buckets, overflow, sensor)
    if key in _sequences:
        return _sequences[key]
    kw = dict(numBuckets=buckets, numVoxelBlocks=BLOCKS)
    if overflow:
        kw["attachedLinkedListSize"] = 6
    ot = oracle.OracleTable(oracle.default_params(**kw), W, H, 1)
    if overflow:
        ot.set_overflow(True)
    poses, prims = synth.camera_loop(500), synth.room_primitives()
    frames = [(I4, synth.sphere_inside_scene(W, H))] * 2 + [(poses[i], synth.render_room_verts(poses[i], W, H, prims).numpy()) for i in ROOM]
    out = []
    before = ot.hash_table()["ptr"] != -1
    for pose, verts in frames:
        given = verts
        if sensor:
            given = np.round(verts[..., 2] * 5000.0).clip(0, 65535).astype(np.uint16)
            verts = oracle.preprocess(given, kinv_of(W, H))[0]
        ot.integrate(pose, verts)
        snap = _Snapshot(ot)
        listed = entries_as_set(snap.compact())
        tab = snap.hash_table()
        slots = np.array([i for i in np.flatnonzero(before) if tuple(tab["pos"][i].tolist()) in listed], np.int64)
        out.append((pose, np.ascontiguousarray(given), snap, slots))
        before = tab["ptr"] != -1
    ot.close()
    while len(_sequences) >= 2:
        _sequences.pop(next(iter(_sequences)))
    _sequences[key] = out
    return out


def every_tile_is_seen(seq, frame, buckets, tile_entries):
    """The precondition, from the oracle alone."""
    tiles = -(-buckets * 5 // tile_entries)
    seen = set((seq[frame][3] // tile_entries).tolist())
    assert seen == set(range(tiles)), f"frame {frame}: walk tiles {sorted(set(range(tiles)) - seen)} hold no visible entry: the case proves nothing"


def make_table(vh, W, H, buckets, form, short=1, walk_nt=0, overflow=False, options=()):
    kw = dict(numBuckets=buckets, numVoxelBlocks=BLOCKS)
    if overflow:
        kw["attachedLinkedListSize"] = 6
    gt = vh.SDFHashtable(vh.default_params(**kw), W, H, 1)
    gt.set_option("flatten_variant", 3)
    gt.set_option("walk_short", short)
    gt.set_option("walk_nt", walk_nt)
    if overflow:
        gt.set_option("overflow_list", 1)
    if form == "step":
        gt.set_option("fused_frame", 0)
    for name, value in options:
        gt.set_option(name, value)
    return gt


def feed(gt, torch, W, H, part, form, sensor):
    dev = [torch.from_numpy(given).cuda() for _, given, _, _ in part]
    poses = [pose for pose, _, _, _ in part]
    if form == "pipelined":
        if sensor:
            gt.integrate_depth_batch(poses, dev, kinv_of(W, H))
        else:
            gt.integrate_batch(poses, dev)
        return
    for pose, d in zip(poses, dev):            # "two_launch" (pipeline 0) and "step" (fused_frame 0)
        if sensor:
            gt.integrate_depth(pose, d, kinv_of(W, H))
        else:
            gt.integrate(pose, d)
    gt.synchronize()


def run_and_compare(oracle, vh, torch, W, H, buckets, form, chunk, short=1, walk_nt=0, overflow=False, sensor=False, options=()):
    seq = sequence(oracle, W, H, buckets, overflow, sensor)
    tile_entries = 1024 if short else 2048
    gt = make_table(vh, W, H, buckets, form, short, walk_nt, overflow, options)
    try:
        for s in range(0, len(seq), chunk):
            part = seq[s:s + chunk]
            last = s + len(part) - 1
            if last > 0:
                every_tile_is_seen(seq, last, buckets, tile_entries)
            feed(gt, torch, W, H, part, form, sensor)
            _compare(seq[last][2], gt)
        assert gt.counters()["spin_timeouts"] == 0
        return gt.hash_table(), gt.compact(), gt.sdf_blocks()
    finally:
        gt.close()


# buckets (x 5 entries) whose walk has 1, 2, 7, 8, 9 and 17 tiles: ceil(5 * buckets / 1024) and ceil(5 * buckets / 2048)
SIZES = {1: {1: 204, 2: 409, 7: 1433, 8: 1638, 9: 1843, 17: 3481}, 0: {1: 409, 2: 819, 7: 2867, 8: 3276, 9: 3686, 17: 6963}}
FORMS = [("pipelined", 1, 0), ("pipelined", 3, 0), ("pipelined", 3, 1), ("two_launch", 1, 0), ("two_launch", 3, 1), ("step", 1, 0)]
TABLE_CASES = [pytest.param(short, tiles, form, chunk, nt, id=f"{'short' if short else 'long'}-{tiles}tiles-{form}-by{chunk}-nt{nt}")
               for short in (1, 0) for tiles in (1, 2, 7, 8, 9, 17) for form, chunk, nt in FORMS]


def test_sizes_have_the_tile_counts_they_are_named_for():
    for short, tile in ((1, 1024), (0, 2048)):
        for tiles, buckets in SIZES[short].items():
            assert -(-buckets * 5 // tile) == tiles


@pytest.mark.parametrize("short,tiles,form,chunk,walk_nt", TABLE_CASES)
def test_table_sizes(oracle, vh, torch_cuda, short, tiles, form, chunk, walk_nt):
    """160x120 (80 claim tiles) on tables of 1 .. 17 walk tiles: checked after every frame, or after batches of 3 (the
    checks then fall on frames 2, 5 and 8: a forward, a backward and a forward walk)."""
    run_and_compare(oracle, vh, torch_cuda, 160, 120, SIZES[short][tiles], form, chunk, short=short, walk_nt=walk_nt)


@pytest.mark.parametrize("form,chunk", [("pipelined", 1), ("pipelined", 3), ("two_launch", 1), ("step", 1)])
@pytest.mark.parametrize("size", [(16, 16), (48, 32), (80, 48)])
def test_image_sizes(oracle, vh, torch_cuda, size, form, chunk):
    """1, 6 and 15 claim tiles (one claim group filled up with 7, 2 and 1 idle workgroups) on a table of 9 walk tiles."""
    W, H = size
    assert ((W + 15) // 16) * ((H + 15) // 16) in (1, 6, 15)
    run_and_compare(oracle, vh, torch_cuda, W, H, 1843, form, chunk)


@pytest.mark.parametrize("size", [(160, 120), (48, 32)])
@pytest.mark.parametrize("form,chunk", [("pipelined", 1), ("pipelined", 3), ("two_launch", 1)])
def test_sensor_input(oracle, vh, torch_cuda, form, chunk, size):
    """The uint16 image as input (vh_integrate_depth, vh_integrate_depth_batch)."""
    run_and_compare(oracle, vh, torch_cuda, size[0], size[1], 1843, form, chunk, sensor=True)


@pytest.mark.parametrize("buckets", [204, 1843])
@pytest.mark.parametrize("form,chunk,pipeline_overflow", [("pipelined", 1, 2), ("pipelined", 3, 2), ("pipelined", 3, 1), ("pipelined", 3, 0),
                                                          ("two_launch", 1, 1), ("step", 1, 1)])
def test_overflow_list(oracle, vh, torch_cuda, form, chunk, pipeline_overflow, buckets):
    """With the overflow list a batch takes the serialised one-launch form (pipeline_overflow 2, or 1 at this size) or two
    launches per frame (0): both on the grouped layout."""
    run_and_compare(oracle, vh, torch_cuda, 160, 120, buckets, form, chunk, overflow=True, options=(("pipeline_overflow", pipeline_overflow),))


def test_role_counts_that_are_no_multiple_of_8(oracle, vh, torch_cuda):
    """commit_blocks 3: the launch rounds its commit role up, the walk ordinals keep their class."""
    run_and_compare(oracle, vh, torch_cuda, 160, 120, 3481, "pipelined", 3, options=(("commit_blocks", 3),))


@pytest.mark.parametrize("form", ["pipelined", "two_launch", "step"])
def test_walk_reverse_0_and_1_leave_the_same_model(oracle, vh, torch_cuda, form):
    """A/B of the option on one sequence: the same slots and keys, the same compact set, the same voxels bit for bit (block
    ids are dealt by an atomic race in either, so voxels are matched by key)."""
    got = [run_and_compare(oracle, vh, torch_cuda, 160, 120, 3481, form, 3, options=(("walk_reverse", value),)) for value in (0, 1)]
    (tab0, comp0, vol0), (tab1, comp1, vol1) = got
    assert np.array_equal(tab0["ptr"] != -1, tab1["ptr"] != -1)
    assert np.array_equal(tab0["pos"], tab1["pos"]) and np.array_equal(tab0["offset"], tab1["offset"])
    assert len(comp0) == len(comp1) and entries_as_set(comp0) == entries_as_set(comp1)
    live = np.flatnonzero(tab0["ptr"] != -1)
    assert len(live) > 400
    for i in live:
        a, b = int(tab0["ptr"][i]), int(tab1["ptr"][i])
        assert np.array_equal(vol0[a:a + 512].view(np.uint32), vol1[b:b + 512].view(np.uint32))
