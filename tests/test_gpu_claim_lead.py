"""The claim window with a lead (vh_frame.hip: grouped_role; vh_api_frame.hip: claim_lead; option "claim_lead"): the claim
tiles start that many groups of 8 workgroups into the claim + walk workgroups of a launch, the groups ahead of them walk.
Wherever the window sits, every claim tile is served once and every walk tile is walked once, so table, voxels and compact
set stay the oracle's, bit for bit.

Three frames per case, the second of which inserts blocks: in the pipelined form its commit phase is in flight beside the
third frame's shifted window.

* The sizes the layout can go wrong at with any window: tables of 1, 2, 7, 8, 9 and 17 walk tiles in both tile widths
  (option "walk_short"), images of 1, 6, 15 and 80 claim tiles.  The host keeps strictly more groups than claim groups in
  the window and takes the lead off the window's length, so on these the lead that reaches the kernel is 0 whatever is asked
  (asserted): they show that asking does no harm.
* Tables of 5, 9 and 17 walk GROUPS under images of 1, 2 and 10 claim groups, where a lead fits: the host's arithmetic is
  restated here (effective_lead) and every case asserts the lead it runs with -- 1 for 1, the rule's value, and for a lead
  far beyond the grid a positive value below the request.

Leads 0, 1, the host's rule (-1) and beyond; the pipelined and the two-launch frame; "walk_reverse" 0 and 1; vertex-map
and uint16 input; the overflow list (the generic build).

Before the GPU is compared the ORACLE alone is asked whether the second frame inserted a block and whether every walk tile
holds an entry that was in the table before the third frame and is listed in it (a tile the walk skipped then shows as a
block that was not updated; a tile walked twice as a duplicate in the list: _compare)."""
import numpy as np
import pytest

from conftest import entries_as_set
from test_gpu_parity import _compare
from test_gpu_walk_order import SIZES, _Snapshot, feed, kinv_of
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
I4 = np.eye(4, dtype=np.float32)
BLOCKS = 16384
VOXEL_FINE = 0.004                     # the tables of 5 .. 17 walk groups: a few thousand blocks, so that every tile holds a listed one
BEYOND = 1 << 20                       # a lead far beyond the number of walk groups of any case here
LEADS = (0, 1, -1, BEYOND)

_sequences = {}            # the oracle's three frames of a case, computed once (the two most recent are kept)


def claim_tiles(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def effective_lead(W, H, buckets, short, lead, form):
    """vh_api_frame.hip restated: claim_span (a table this small streams in under 1 us, so the share is its floor, 0.5) and
    claim_lead.  -> (lead that reaches the kernel, the window's length in groups)"""
    claim_groups = -(-claim_tiles(W, H) // 8)
    tile_entries = 1024 if short else 2048
    walk_groups = -(-(-(-buckets * 5 // tile_entries)) // 8)
    total = claim_groups + walk_groups
    assert buckets * 5 * 20 / 6.0e6 < 1.0
    span = min(total, max(claim_groups + 1, int(0.5 * total)))
    if lead >= 0:
        want = lead
    elif form == "pipelined":
        want = min((4 << 20) // (20 * tile_entries), walk_groups // 4)
    else:
        want = 0
    least = claim_groups + 1
    got = min(want, span - least) if span > least else 0
    return got, span - got


def sequence(oracle, W, H, buckets, overflow=False, sensor=False, voxel=None):
    """-> ([(pose, input, None, None)] * 3, snapshot after the third frame, slots the third frame's walk must find,
    blocks the second frame inserted)"""
    key = (W, H, buckets, overflow, sensor, voxel)
    if key in _sequences:
        return _sequences[key]
    kw = dict(numBuckets=buckets, numVoxelBlocks=BLOCKS)
    if voxel:
        kw["voxelSize"] = voxel
    if overflow:
        kw["attachedLinkedListSize"] = 6
    ot = oracle.OracleTable(oracle.default_params(**kw), W, H, 1)
    if overflow:
        ot.set_overflow(True)
    poses, prims = synth.camera_loop(500), synth.room_primitives()
    frames = [(I4, synth.sphere_inside_scene(W, H))] + [(poses[i], synth.render_room_verts(poses[i], W, H, prims).numpy()) for i in (0, 1)]
    part, allocated = [], []
    for pose, verts in frames:
        given = verts
        if sensor:
            given = np.round(verts[..., 2] * 5000.0).clip(0, 65535).astype(np.uint16)
            verts = oracle.preprocess(given, kinv_of(W, H))[0]
        before = ot.hash_table()["ptr"] != -1
        ot.integrate(pose, verts)
        allocated.append(int((ot.hash_table()["ptr"] != -1).sum()))
        part.append((pose, np.ascontiguousarray(given), None, None))
    snap = _Snapshot(ot)
    listed = entries_as_set(snap.compact())
    tab = snap.hash_table()
    slots = np.array([i for i in np.flatnonzero(before) if tuple(tab["pos"][i].tolist()) in listed], np.int64)
    ot.close()
    while len(_sequences) >= 2:
        _sequences.pop(next(iter(_sequences)))
    _sequences[key] = (part, snap, slots, allocated[1] - allocated[0])
    return _sequences[key]


def precondition(seq, buckets, tile_entries):
    """From the oracle alone: the case can show a skipped walk tile and has a commit in flight beside the third frame."""
    _, _, slots, inserted = seq
    assert inserted >= 1, "the second frame inserts no block: no commit phase runs beside the third frame's claim window"
    tiles = -(-buckets * 5 // tile_entries)
    seen = set((slots // tile_entries).tolist())
    assert seen == set(range(tiles)), f"walk tiles {sorted(set(range(tiles)) - seen)} hold no entry the third frame lists: the case proves nothing"


def make_table(vh, W, H, buckets, form, short, overflow, voxel, options):
    kw = dict(numBuckets=buckets, numVoxelBlocks=BLOCKS)
    if voxel:
        kw["voxelSize"] = voxel
    if overflow:
        kw["attachedLinkedListSize"] = 6
    gt = vh.SDFHashtable(vh.default_params(**kw), W, H, 1)
    gt.set_option("flatten_variant", 3)
    gt.set_option("walk_short", short)
    gt.set_option("walk_nt", 0)
    if overflow:
        gt.set_option("overflow_list", 1)
    for name, value in options:
        gt.set_option(name, value)
    return gt


def run_and_compare(oracle, vh, torch, W, H, buckets, form, lead, short=1, reverse=1, overflow=False, sensor=False, voxel=None, options=()):
    seq = sequence(oracle, W, H, buckets, overflow, sensor, voxel)
    precondition(seq, buckets, 1024 if short else 2048)
    gt = make_table(vh, W, H, buckets, form, short, overflow, voxel, (("walk_reverse", reverse), ("claim_lead", lead)) + tuple(options))
    try:
        feed(gt, torch, W, H, seq[0], form, sensor)
        _compare(seq[1], gt)
        assert gt.counters()["spin_timeouts"] == 0
    finally:
        gt.close()


# ---- the sizes of the layout's edge cases: no lead fits, whatever is asked ----

TABLE_CASES = [pytest.param(short, tiles, form, lead, id=f"{'short' if short else 'long'}-{tiles}tiles-{form}-lead{lead}")
               for short in (1, 0) for tiles in (1, 2, 7, 8, 9, 17) for form in ("pipelined", "two_launch") for lead in (1, BEYOND)]


@pytest.mark.parametrize("short,tiles,form,lead", TABLE_CASES)
def test_table_sizes(oracle, vh, torch_cuda, short, tiles, form, lead):
    """160x120 (80 claim tiles, 10 claim groups) on tables of 1 .. 17 walk tiles (1 .. 3 walk groups)."""
    assert effective_lead(160, 120, SIZES[short][tiles], short, lead, form)[0] == 0
    run_and_compare(oracle, vh, torch_cuda, 160, 120, SIZES[short][tiles], form, lead, short=short)


@pytest.mark.parametrize("lead", (1, BEYOND))
@pytest.mark.parametrize("form", ["pipelined", "two_launch"])
@pytest.mark.parametrize("size", [(16, 16), (48, 32), (80, 48)])
def test_image_sizes(oracle, vh, torch_cuda, size, form, lead):
    """1, 6 and 15 claim tiles on a table of 17 walk tiles (3 walk groups)."""
    W, H = size
    assert claim_tiles(W, H) in (1, 6, 15)
    assert effective_lead(W, H, SIZES[1][17], 1, lead, form)[0] == 0
    run_and_compare(oracle, vh, torch_cuda, W, H, SIZES[1][17], form, lead)


# ---- tables with room for a lead ----

def buckets_for(groups, short):
    """the largest table whose walk has exactly 8 * groups tiles"""
    return 8 * groups * (1024 if short else 2048) // 5


# (W, H, walk groups, walk_short): 1 claim group under 5, 9 and 17 walk groups, 2 under 9, 10 (80 claim tiles) under 17
SHAPES = [(48, 32, 5, 1), (48, 32, 9, 1), (48, 32, 17, 1), (48, 32, 9, 0), (80, 48, 9, 1), (160, 120, 17, 1), (160, 120, 17, 0)]
LEAD_CASES = [pytest.param(W, H, groups, short, form, lead, reverse, sensor,
                           id=f"{W}x{H}-{groups}groups-{'short' if short else 'long'}-{form}-lead{lead}-reverse{reverse}-{'uint16' if sensor else 'verts'}")
              for W, H, groups, short in SHAPES for form in ("pipelined", "two_launch") for lead in LEADS
              for reverse, sensor in ((1, False), (0, False), (0, True), (1, True))
              # every shape, form and lead with the alternating walk and the vertex map; always forward and the uint16 image
              # on one shape of each image size (leads 1 and the rule)
              if (reverse, sensor) == (1, False) or ((groups, short) in ((9, 1), (17, 0)) and lead in (1, -1))]


def test_shapes_have_the_groups_they_are_named_for():
    for W, H, groups, short in SHAPES:
        assert -(-buckets_for(groups, short) * 5 // (1024 if short else 2048)) == 8 * groups


@pytest.mark.parametrize("W,H,groups,short,form,lead,reverse,sensor", LEAD_CASES)
def test_a_lead_that_fits(oracle, vh, torch_cuda, W, H, groups, short, form, lead, reverse, sensor):
    buckets = buckets_for(groups, short)
    got, span = effective_lead(W, H, buckets, short, lead, form)
    claim_groups = -(-claim_tiles(W, H) // 8)
    assert span > claim_groups and got + span <= claim_groups + groups
    if lead == 0 or (lead == -1 and form == "two_launch"):
        assert got == 0
    elif lead == 1:
        assert got == 1
    elif lead == -1:
        assert got == min(groups // 4, effective_lead(W, H, buckets, short, BEYOND, form)[0]) >= 1
    else:
        assert 1 <= got < lead                 # clamped, and still a lead
    run_and_compare(oracle, vh, torch_cuda, W, H, buckets, form, lead, short=short, reverse=reverse, sensor=sensor, voxel=VOXEL_FINE)


@pytest.mark.parametrize("form,pipeline_overflow", [("pipelined", 2), ("two_launch", 1)])
def test_overflow_list(oracle, vh, torch_cuda, form, pipeline_overflow):
    """With the overflow list the pipelined launch is the generic build, serialised inside the launch; the lead holds there too."""
    buckets = buckets_for(9, 1)
    assert effective_lead(48, 32, buckets, 1, 2, form)[0] == 2
    run_and_compare(oracle, vh, torch_cuda, 48, 32, buckets, form, 2, overflow=True, voxel=VOXEL_FINE, options=(("pipeline_overflow", pipeline_overflow),))
