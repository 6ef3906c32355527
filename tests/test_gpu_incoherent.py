"""The frame path on incoherent depth and a loaded table, against the oracle: after every frame (or batch) the same slots
and keys, the same offset links, the compact set, the heap counter and the voxels bit for bit (test_gpu_parity._compare).
Inputs and census: tests/incoherent_cases.py; that they reach what they are meant to reach is asserted without a GPU in
tests/test_incoherent_cases_cpu.py, and every case here asserts on the oracle's side what makes it non-vacuous.

What the smooth scenes of the other suites never run (the two refills, the larger candidate list) or only touch (a second
pass of the index walk, slots 2..: DESIGN_LOG.md names the cases), and which case runs it:
  claim_tile_wave's refill (vh_alloc.hip, count + n > kWaveQueue)        test_tile_per_wave_refills_its_queue
  claim_tile's drain inside the sample loop (count + n > kClaimQueue)     test_band_queue_drains_inside_the_sample_loop*
  further passes of flatten_index_tile_to, slots 2.. behind a live slot 1 test_loaded_table*, walk 4
  a candidate list beyond W*H records for a band frame                    test_band_queue* (vh_api.hip: ensure_band_candidates)

The three refill paths, read for termination and barrier uniformity before the first run:
  flatten_index_tile_to's for (;;): a pass moves min(set bits of the wave, 512) buckets out of `bits` (the first lane with a set
    bit has excl < 512, so a wave with bits left always makes progress) and ends when __syncthreads_or sees none left in the
    workgroup.  Every barrier in the pass is reached by all four waves alike: `rounds` is the maximum over the waves' rounds_[],
    `total` the sum over hits_[], both read after a barrier, and rounds_ / hits_ / base_ are rewritten only behind the next one.
  claim_tile_wave's drain: called at count + n > kWaveQueue and once at the end; count, n and mask come from ballots, so the
    condition is wave-uniform, and the lambda holds no barrier (a lane probes queue[ln], ln < n <= 64).  After a drain count is
    0 and n <= 64 entries are written at 0 .. n - 1: the queue cannot overrun.
  claim_tile's drain: the same with kClaimQueue = 128 (count <= 128 before, n <= 64 after); its loop over `base` is bounded by
    the wave-uniform count, and the sample loop ends by wave_done(k), a ballot.  LDS accesses of one wave are served in order,
    so the queue's volatile reads of a drain precede the writes that refill it."""
import numpy as np
import pytest

import incoherent_cases as ic
from conftest import entries_as_set
from test_gpu_overflow import VARIANTS, pair
from test_gpu_parity import _compare
from test_overflow_cpu import chains_ok
from test_sharding_cpu import check_shard_against_full
from voxelhashing_demo_amd import dist as vdist
from voxelhashing_demo_amd import synth

pytestmark = pytest.mark.gpu
I4 = np.eye(4, dtype=np.float32)
S = ic.SIZE
PLAIN_KW = dict(numBuckets=4096, bucketSize=5, numVoxelBlocks=8192)
PLAIN_POSES = (I4, synth.yaw_pose(4.0, (0.02, 0.0, 0.01)), I4)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _clean(gt):
    c = gt.counters()
    assert c["cand_overflow"] == 0 and c["heap_exhausted"] == 0, c


# ---- a. the plain frame, every form ----
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("sem", [1, 0])
@pytest.mark.parametrize("scene", ["incoherent64", "duplicates64"])
def test_plain_frame_every_form(oracle, vh, torch_cuda, scene, sem, variant):
    """Three frames (seeds 5, 6 and 5 again: what lost its bucket in frame 0 comes back), PINHOLE and REFERENCE semantics:
    about 2 200 distinct blocks per frame of 4 000 pixels into 4 096 buckets -- hundreds of lock losses per frame, every one
    of which must go to the lowest launch rank, and with duplicates64 every key demanded by many lanes and waves."""
    make = ic.incoherent64 if scene == "incoherent64" else ic.duplicates64
    ot, gt = pair(oracle, vh, variant, S, S, sem, overflow=False, **PLAIN_KW)
    inserted = losses = 0
    for pose, seed in zip(PLAIN_POSES, ic.PLAIN_SEEDS + ic.PLAIN_SEEDS[:1]):
        verts = make(seed)
        ot.integrate(pose, verts)
        gt.integrate(pose, _dev(torch_cuda, verts))
        gt.synchronize()
        _compare(ot, gt)
        inserted += ot.last_stats["inserted"]
        losses += ot.last_stats["lock_losses"]
    print(f"{scene} sem {sem}: {inserted} blocks, {losses} lock losses")
    assert inserted > (1500 if scene == "incoherent64" else 600) and losses > 300
    _clean(gt)
    ot.close()
    gt.close()


@pytest.mark.parametrize("variant", ["fused-indexed-walk", "pipelined-ballot-walk"])
def test_plain_frame_from_the_sensor_image(oracle, vh, torch_cuda, variant):
    """The uint16 form through integrate_depth against oracle.preprocess + integrate."""
    ot, gt = pair(oracle, vh, variant, S, S, 1, overflow=False, **PLAIN_KW)
    kinv = ic.k_inv()
    inserted = 0
    for pose, seed in zip(PLAIN_POSES, ic.PLAIN_SEEDS + ic.PLAIN_SEEDS[:1]):
        d16 = ic.incoherent64_u16(seed)
        ot.integrate(pose, oracle.preprocess(d16, kinv)[0])
        gt.integrate_depth(pose, _dev(torch_cuda, d16), kinv)
        gt.synchronize()
        _compare(ot, gt)
        inserted += ot.last_stats["inserted"]
    assert inserted > 1500
    _clean(gt)


# ---- b. the launch tile per wave ----
@pytest.mark.parametrize("walk_nt", [0, 1])
@pytest.mark.parametrize("chunk", [1, 3])
def test_tile_per_wave_refills_its_queue(oracle, vh, torch_cuda, chunk, walk_nt):
    """large_patchy (1024x640 = 2560 launch tiles, tiles with ~240 survivors: claim_tile_wave probes and refills its 64-entry
    queue three times) through integrate_batch, four frames with new patches each, so that in a batch the claim of frame i+1
    runs beside the commit of frame i.  Lean builds 7 (walk_nt 0) and 8 (walk_nt 1).
    That claim_tile_wave is what runs: launch_pipelined (vh_api_frame.hip) sets claimPerWave when the frame is new,
    host_num_tiles > 2400 (2560 here, asserted through the census' tile count) and lean_for() names build 5 / 6 -- no overflow
    list, no band, the index walk (flatten_variant 4), and both frames' flags exactly kFlagWalkShort (| kFlagWalkNt): a context
    whose only options are walk_nt and flatten_variant, as here.  Checked by reading that rule; at run time the test asserts
    the pipelined launch itself (frame_pipelined_ms > 0, no two-launch phase)."""
    torch = torch_cuda
    W, H = ic.LARGE
    kw = dict(numBuckets=1 << 15, numVoxelBlocks=1 << 13)
    ot = oracle.OracleTable(oracle.default_params(**kw), W, H, 1)
    gt = vh.SDFHashtable(vh.default_params(**kw), W, H, 1)
    gt.set_option("walk_nt", walk_nt)
    gt.set_option("flatten_variant", 4)
    gt.set_profiling(True)
    frames = [(synth.yaw_pose(2.0 * i, (0.01 * i, 0.0, 0.0)), ic.large_patchy(seed)) for i, seed in enumerate(ic.PATCHY_SEEDS)]
    for pose, verts in frames:
        per_tile = ic.survivors(pose, verts)[1]
        assert len(per_tile) > 2400 and per_tile.max() >= 129 and per_tile[per_tile > 0].min() <= 8
    inserted = 0
    for s in range(0, len(frames), chunk):
        part = frames[s:s + chunk]
        d = [_dev(torch, v) for _, v in part]             # (alive until the batch has run: _compare synchronises)
        gt.integrate_batch([p for p, _ in part], d)
        for p, v in part:
            ot.integrate(p, v)
            inserted += ot.last_stats["inserted"]
        _compare(ot, gt)
    t = gt.kernel_times()
    assert t["frame_pipelined_ms"] > 0.0 and t["frame_commit_integrate_ms"] == 0.0 and t["frame_scan_claim_ms"] == 0.0
    assert inserted > 1000
    _clean(gt)
    ot.close()
    gt.close()


# ---- c. the band queue ----
BAND_FORMS = ["fused-ballot-walk", "four-kernel-reference-walk", "pipelined-ballot-walk"]
BAND_KW = dict(numBuckets=1 << 15, numVoxelBlocks=1 << 13)


def _band_frames(oracle, mode):
    """[(pose, verts, normals or None)]: two frames; NORMAL_DDA takes preProcess's maps of the sensor form."""
    out = []
    for pose, seed in zip(PLAIN_POSES, ic.PLAIN_SEEDS):
        if mode == oracle.BAND_NORMAL_DDA:
            v, n = oracle.preprocess(ic.incoherent64_u16(seed), ic.k_inv())
            out.append((pose, v, n))
        else:
            out.append((pose, ic.incoherent64(seed), None))
    return out


def _run_band(oracle, vh, torch, form, mode, band, min_keys, kw):
    ot, gt = pair(oracle, vh, form, S, S, 1, overflow=False, **kw)
    ot.set_alloc_band(band, mode)
    gt.set_alloc_band(band)
    gt.set_option("band_mode", mode)
    inserted = losses = 0
    for pose, verts, normals in _band_frames(oracle, mode):
        per_wave, keys = ic.band_keys_per_wave(oracle, pose, verts, band, mode, normals=normals)
        assert per_wave.max() >= min_keys, per_wave.max()      # the wave's queue overflows inside the sample loop
        assert keys > 2 * S * S, keys                          # more contenders than a W*H candidate list holds
        ot.integrate(pose, verts, normals)
        gt.integrate(pose, _dev(torch, verts), None if normals is None else _dev(torch, normals))
        gt.synchronize()
        _compare(ot, gt)
        inserted += ot.last_stats["inserted"]
        losses += ot.last_stats["lock_losses"]
    assert inserted > 3000 and losses > 1000
    _clean(gt)
    ot.close()
    gt.close()


@pytest.mark.parametrize("form", BAND_FORMS)
@pytest.mark.parametrize("mode", ["RAY", "RAY_DDA", "NORMAL_DDA"])
def test_band_queue_drains_inside_the_sample_loop(oracle, vh, torch_cuda, mode, form):
    """incoherent64 with a 10 cm band: the fullest wave produces 315-320 keys (RAY), ~200 (RAY_DDA), ~180 (NORMAL_DDA) for a
    queue of 128, so claim_tile drains it inside the sample loop; two frames, the second meets the first one's entries.  A frame
    demands 9 000 - 17 500 keys from 4 096 pixels (about 3 000 distinct new blocks)."""
    m = getattr(oracle, "BAND_" + mode)
    _run_band(oracle, vh, torch_cuda, form, m, 0.1, 257 if mode == "RAY" else 129, BAND_KW)


def test_band_queue_five_drains(oracle, vh, torch_cuda):
    """RAY mode at 33 cm: about 700 keys in the fullest wave, five drains; 38 000 keys per frame."""
    _run_band(oracle, vh, torch_cuda, "fused-ballot-walk", oracle.BAND_RAY, 0.33, 641, BAND_KW)


# ---- d. the loaded table ----
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_loaded_table(oracle, vh, torch_cuda, variant):
    """Six incoherent frames into 2048 buckets x 5 slots, no list: 1 200 - 1 800 occupied buckets in the one 8192-bucket span of
    an index-walk wave (three or four passes of its 512-bucket list), hundreds of buckets with entries in slots 2 .. 4, full
    buckets that refuse winners from frame 4 on, 1 400 lock losses in frame 0."""
    ot, gt = pair(oracle, vh, variant, S, S, 1, overflow=False, **ic.LOADED_KW)
    full_frames = 0
    for pose, verts in ic.sequence():
        ot.integrate(pose, verts)
        gt.integrate(pose, _dev(torch_cuda, verts))
        gt.synchronize()
        _compare(ot, gt)
        c = ic.table_census(ot)
        assert max(c["occupied_per_span"]) > ic.INDEX_QUEUE
        full_frames += ot.last_stats["bucket_full"] > 0
    assert c["buckets_3plus"] >= 100 and c["buckets_full"] >= 20 and full_frames >= 2
    _clean(gt)
    ot.close()
    gt.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_loaded_table_with_the_overflow_list(oracle, vh, torch_cuda, variant):
    """The same frames into 1024 x 2 with the list on (attachedLinkedListSize 8): chains from frame 2 on, load beyond 0.85."""
    ot, gt = pair(oracle, vh, variant, S, S, 1, overflow=True, **ic.CHAINED_KW)
    for pose, verts in ic.sequence():
        ot.integrate(pose, verts)
        gt.integrate(pose, _dev(torch_cuda, verts))
        gt.synchronize()
        _compare(ot, gt)
    c = ic.table_census(ot)
    assert c["links"] >= 20 and c["load"] > 0.85 and (gt.hash_table()["offset"] != 0).sum() == c["links"]
    chains_ok(oracle, ot)
    _clean(gt)
    ot.close()
    gt.close()


@pytest.mark.parametrize("walk", [3, 4])
def test_loaded_table_pipelined_batches(oracle, vh, torch_cuda, walk):
    """The 2048 x 5 sequence through integrate_batch in chunks of 2 (commit(i) beside claim(i+1) and walk(i+1): several
    passes of the index walk with insertions in flight), compared after every batch."""
    torch = torch_cuda
    ot = oracle.OracleTable(oracle.default_params(**ic.LOADED_KW), S, S, 1)
    gt = vh.SDFHashtable(vh.default_params(**ic.LOADED_KW), S, S, 1)
    gt.set_option("flatten_variant", walk)
    gt.set_profiling(True)
    frames = ic.sequence()
    full_frames = 0
    for s in range(0, len(frames), 2):
        part = frames[s:s + 2]
        d = [_dev(torch, v) for _, v in part]
        gt.integrate_batch([p for p, _ in part], d)
        for p, v in part:
            ot.integrate(p, v)
            full_frames += ot.last_stats["bucket_full"] > 0
        _compare(ot, gt)
        assert max(ic.table_census(ot)["occupied_per_span"]) > 2 * ic.INDEX_QUEUE
    c = ic.table_census(ot)
    assert c["buckets_3plus"] >= 100 and full_frames >= 2
    assert gt.kernel_times()["frame_pipelined_ms"] > 0.0
    _clean(gt)
    ot.close()
    gt.close()


def test_loaded_table_heap_runs_dry(oracle, vh, torch_cuda):
    """A heap of 1 500 blocks: frame 0 takes about 1 200, frame 1 wants 900 more.  As in test_heap_exhaustion_is_bounded the
    count is exact and the demanded set bounds the allocated set; which winners are refused is unspecified (atomic order)."""
    kw = dict(ic.LOADED_KW, numVoxelBlocks=1500)
    ot = oracle.OracleTable(oracle.default_params(**kw), S, S, 1)
    gt = vh.SDFHashtable(vh.default_params(**kw), S, S, 1)
    gt.set_option("pipeline", 0)
    demanded = set()
    for pose, verts in ic.sequence()[:2]:
        ot.integrate(pose, verts)
        gt.integrate(pose, _dev(torch_cuda, verts))
        gt.synchronize()
        keys = ic.block_keys(pose, verts)[verts[..., 2] != 0.0]
        demanded |= set(map(tuple, keys.tolist()))
    assert ot.last_stats["heap_exhausted"] > 100
    galloc, oalloc = gt.allocated(), ot.allocated()
    assert len(galloc) == 1500 == len(oalloc)
    c = gt.counters()
    assert c["heap_counter"] == -1 == ot.heap_counter() and c["heap_exhausted"] > 0
    assert sorted(galloc["ptr"].tolist()) == [512 * i for i in range(1500)]
    assert entries_as_set(galloc) <= demanded and len(entries_as_set(galloc)) == 1500


# ---- e. two shards ----
@pytest.mark.parametrize("band", [0.0, 0.1])
def test_two_shards(oracle, vh, torch_cuda, band):
    """Two cameras, two bucket-range shards in the loop-back rig, two steps of incoherent frames: every shard equals its slice
    of ONE unsharded oracle table.  Without a band generate_keys_groups, with the 10 cm ray band generate_keys_tile bins the
    keys: a launch tile has ~245 (~1 100 with the band) keys, half of them for either owner."""
    torch = torch_cuda
    world = 2
    kw = dict(numBuckets=1 << 13, numVoxelBlocks=1 << 13)
    plan = vdist.ShardPlan(kw["numBuckets"], world)
    shards = [vdist.HipShard(vh.default_params(**kw), S, S, 1, plan, r, 8 * S * S) for r in range(world)]
    full = oracle.OracleTable(oracle.default_params(**kw), S, S, 1)
    if band:
        full.set_alloc_band(band)
        for sh in shards:
            sh.table.set_alloc_band(band)
    for step in range(2):
        cams = [(ic.sequence_pose(2 * step + r), ic.incoherent64(ic.SHARD_SEEDS[2 * step + r])) for r in range(world)]
        for pose, verts in cams:
            per_tile = (ic.band_keys_per_wave(oracle, pose, verts, band, oracle.BAND_RAY)[0] if band else ic.survivors(pose, verts)[0])
            assert per_tile.reshape(-1, 4).sum(axis=1).max() >= (800 if band else 200)
        vdist.loopback_step(shards, [[c[0]] for c in cams], [[_dev(torch, c[1])] for c in cams])
        vdist.reference_multi_camera_frame(full, [c[0] for c in cams], [c[1] for c in cams])
    total = 0
    for r, sh in enumerate(shards):
        sh.table.synchronize()
        total += check_shard_against_full(sh.table, full, *plan.bucket_range(r), 5)
        c = sh.table.counters()
        assert c["bin_overflow"] == 0 and c["cand_overflow"] == 0 and c["heap_exhausted"] == 0
    assert total == len(full.allocated()) > (4000 if band else 3000)
    for sh in shards:
        sh.table.close()
    full.close()
