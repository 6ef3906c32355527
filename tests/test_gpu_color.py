"""The colour calls on the GPU against tests/color_ref.py: after every colour call the model is downloaded -- hash table, the TSDF
the GPU itself fused, the colour volume -- the rule is applied to the PREVIOUS colour volume, and every colour word is compared
bit for bit (the whole volume, so per block key too).  64x48 images of the synthetic room, at most 512 blocks
(tests/deintegrate_cases.py); colour images that differ per frame and per pixel."""
import ctypes as C

import numpy as np
import pytest

import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as R
import sample_ref as S
from voxelhashing_demo_amd import dist as vdist

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
W, H = DC.W, DC.H
VS = DC.KW["voxelSize"]
WORDS = DC.KW["numVoxelBlocks"] * 512
BAND = 1.5 * VS
NEAREST, TRILINEAR = 0, 1
INVALID = 1


def image(i):
    """The colour image of frame i: every pixel and every frame different; byte 3 is noise the library must ignore."""
    return np.random.default_rng(100 + i).integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(U)


def table(vh, sem, **kw):
    p = dict(DC.KW)
    p.update(kw)
    gt = vh.SDFHashtable(vh.default_params(**p), W, H, sem)
    gt.set_projection(DC.projection(sem))
    return gt


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def snapshot(gt):
    gt.synchronize()
    c = gt.counters()
    return dict(table=gt.hash_table(), heap=gt.heap(), vox=gt.sdf_blocks(), heap_counter=c["heap_counter"], occupied=c["occupied"],
                compact=gt.compact(), epoch=c["epoch"], color=gt.color_volume() if gt.has_color() else np.zeros(WORDS, U))


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


def colors_by_key(snap):
    tab = snap["table"]
    return {tuple(e["pos"].tolist()): snap["color"][int(e["ptr"]):int(e["ptr"]) + 512] for e in tab[tab["ptr"] != -1]}


def model_of(snap):
    tab, vox, col = snap["table"], snap["vox"], snap["color"]
    return {tuple(e["pos"].tolist()): (vox["sdf"][int(e["ptr"]):int(e["ptr"]) + 512], vox["weight"][int(e["ptr"]):int(e["ptr"]) + 512],
                                       col[int(e["ptr"]):int(e["ptr"]) + 512]) for e in tab[tab["ptr"] != -1]}


def expected(oracle, gt, pre, sem, pose, src, rgba, band, weight_max):
    """(colour volume, entries, stats) by the rule from the downloaded state `pre` (its TSDF is the one the call sees)."""
    proj, inv = DC.projection(sem), oracle.invert4x4(pose)
    entries = pre["table"][R.visible_entries(pre["table"], gt.params, sem, proj, pose, inv, W, H)]
    want, stats = CR.integrate(pre["color"], pre["vox"], entries, gt.params, sem, proj, inv, src, rgba, band, weight_max)
    return want, entries, stats


def check_against_rule(gt, pre, want, entries):
    post = snapshot(gt)
    for name in ("table", "heap", "vox"):                                 # the hash table, the heap, the SDF volume: unchanged
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    assert post["heap_counter"] == pre["heap_counter"] and post["epoch"] == pre["epoch"]
    assert post["occupied"] == len(entries)                               # the compact list: the flatten's
    assert keys_of(post["compact"]) == keys_of(entries)
    bad = np.nonzero(post["color"] != want)[0]
    assert len(bad) == 0, (len(bad), bad[:4], post["color"][bad[:4]], want[bad[:4]])
    return post


def color_call(torch, gt, frame, rgba, band, weight_max, sensor=True):
    pose, d16, verts = frame
    if sensor:
        gt.integrate_color(pose, dev(torch, d16), DC.k_inv(), dev(torch, rgba), band, weight_max)
    else:
        gt.integrate_color_map(pose, dev(torch, verts), dev(torch, rgba), band, weight_max)


def fuse_depth(torch, gt, frames, which):
    for i in which:
        gt.integrate_depth(frames[i][0], dev(torch, frames[i][1]), DC.k_inv())


# ---- 1. three frames, the cap reached -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("sensor", [False, True], ids=["vertex-map", "uint16"])
def test_three_frames_with_the_cap_reached(oracle, vh, torch_cuda, sem, sensor):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, sem)
    assert not gt.has_color()
    for i, (pose, d16, verts) in enumerate(frames):
        if sensor:
            gt.integrate_depth(pose, dev(torch, d16), DC.k_inv())
        else:
            gt.integrate(pose, dev(torch, verts))
        pre = snapshot(gt)
        want, entries, stats = expected(oracle, gt, pre, sem, pose, (d16, DC.k_inv()) if sensor else verts[..., 2], image(i), BAND, 2)
        assert stats["sampled"] > 1000 and stats["rejected"] > 0, stats
        color_call(torch, gt, frames[i], image(i), BAND, 2, sensor)
        assert gt.has_color()
        check_against_rule(gt, pre, want, entries)
    # a condition on the inputs: the reference itself has many coloured voxels, fresh ones and ones at the cap
    n = CR.count(want)
    print(f"sem {sem}: coloured {(want != 0).sum()}, w == 1: {(n == 1).sum()}, at the cap: {(n == 2).sum()}")
    assert (want != 0).sum() >= 1000 and (n == 1).sum() > 0 and (n == 2).sum() > 0 and n.max() == 2
    gt.close()


# ---- 2. the band -----------------------------------------------------------------------------------------------------------
def test_band_of_half_a_voxel_against_three_voxels(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [0, 1, 2])
    seen = []
    for band in (0.5 * VS, 3.0 * VS):
        pre = snapshot(gt)
        want, entries, stats = expected(oracle, gt, pre, 1, frames[1][0], (frames[1][1], DC.k_inv()), image(1), band, 255)
        color_call(torch, gt, frames[1], image(1), band, 255)
        seen.append(check_against_rule(gt, pre, want, entries)["color"])
        gt.clear_color()
        gt.synchronize()
        assert gt.has_color() and not gt.color_volume().any()
    thin, wide = seen
    assert 0 < (thin != 0).sum() < (wide != 0).sum() and not ((thin != 0) & (wide == 0)).any()
    gt.close()


# ---- 3. the stride loop and the empty list ---------------------------------------------------------------------------------
def test_two_workgroups_stride_over_the_list_and_an_empty_view(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    gt.set_option("integrate_grid", 2)
    fuse_depth(torch, gt, frames, [0, 1, 2])
    color_call(torch, gt, frames[0], image(0), BAND, 255)
    pre = snapshot(gt)
    assert pre["color"].any()
    # a pose that sees no block: nothing changes, occupied == 0
    nowhere = (DC.NOWHERE, frames[1][1], frames[1][2])
    want, entries, _ = expected(oracle, gt, pre, 1, DC.NOWHERE, (frames[1][1], DC.k_inv()), image(1), BAND, 255)
    assert len(entries) == 0 and np.array_equal(want, pre["color"])
    color_call(torch, gt, nowhere, image(1), BAND, 255)
    post = check_against_rule(gt, pre, want, entries)
    assert post["occupied"] == 0
    # two workgroups over many blocks
    want, entries, stats = expected(oracle, gt, post, 1, frames[1][0], (frames[1][1], DC.k_inv()), image(1), BAND, 255)
    assert len(entries) > 2 and stats["sampled"] > 1000
    color_call(torch, gt, frames[1], image(1), BAND, 255)
    check_against_rule(gt, post, want, entries)
    gt.close()


# ---- 4. the overflow list --------------------------------------------------------------------------------------------------
def test_chained_entries_are_coloured(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    nb, bs = 32, 2                                                        # (few buckets: that is what makes chains)
    gt = table(vh, 1, numBuckets=nb, bucketSize=bs, attachedLinkedListSize=8)
    gt.set_option("overflow_list", 1)
    for _ in range(6):                                                    # (a bucket takes one new entry per frame)
        fuse_depth(torch, gt, frames, [0, 1, 2])
    pre = snapshot(gt)
    want, entries, stats = expected(oracle, gt, pre, 1, pose, (d16, DC.k_inv()), image(1), BAND, 255)
    idx = R.visible_entries(pre["table"], gt.params, 1, DC.projection(1), pose, oracle.invert4x4(pose), W, H)
    chained = [int(i) for i in idx if oracle.hash_block(*[int(c) for c in pre["table"][i]["pos"]], nb) != i // bs]
    assert chained, "no chained entry is visible: the scene does not test the overflow list"
    assert any(want[int(pre["table"][i]["ptr"]):int(pre["table"][i]["ptr"]) + 512].any() for i in chained)
    color_call(torch, gt, frames[1], image(1), BAND, 255)
    check_against_rule(gt, pre, want, entries)
    gt.close()


# ---- 5. a pending pipelined frame ------------------------------------------------------------------------------------------
def test_pending_pipelined_frame_is_launched_first(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    snaps = []
    for pipeline in (1, 0):
        gt = table(vh, 1)
        gt.set_option("pipeline", pipeline)
        gt.set_profiling(True)
        fuse_depth(torch, gt, frames, [0, 1, 2])                          # pipelined: frame 2's commit + update are still pending
        color_call(torch, gt, frames[2], image(2), BAND, 255)
        snaps.append(snapshot(gt))
        t = gt.kernel_times()
        assert (t["frame_pipelined_ms"] > 0) == bool(pipeline) and t["integrate_ms"] > 0 and t["flatten_ms"] > 0
        gt.close()
    a, b = colors_by_key(snaps[0]), colors_by_key(snaps[1])
    assert a.keys() == b.keys() and sum(int(v.any()) for v in a.values()) > 10
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # frame 2's own voxels carry colour: its TSDF was in the model the colour call saw
    assert (snaps[0]["color"] != 0).sum() > 1000


# ---- 6. shards -------------------------------------------------------------------------------------------------------------
def test_two_shards_together_equal_the_unsharded_volume(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    world = 2
    params = vh.default_params(**DC.KW)
    plan = vdist.ShardPlan(DC.KW["numBuckets"], world)
    shards = [vdist.HipShard(params, W, H, 1, plan, r, W * H) for r in range(world)]
    full = table(vh, 1)
    for sh in shards:
        sh.table.set_projection(DC.projection(1))
    for a, b in ((0, 1), (2, 1)):
        cams = [frames[a], frames[b]]
        vdist.loopback_step(shards, [[c[0]] for c in cams], [[dev(torch, c[2])] for c in cams])
        vdist.reference_multi_camera_frame(full, [c[0] for c in cams], [dev(torch, c[2]) for c in cams])
    pre = snapshot(full)
    want, entries, stats = expected(oracle, full, pre, 1, pose, (d16, DC.k_inv()), image(1), BAND, 255)
    assert stats["sampled"] > 1000
    color_call(torch, full, frames[1], image(1), BAND, 255)
    whole = colors_by_key(check_against_rule(full, pre, want, entries))
    union = {}
    for sh in shards:
        spre = snapshot(sh.table)
        swant, sentries, sstats = expected(oracle, sh.table, spre, 1, pose, (d16, DC.k_inv()), image(1), BAND, 255)
        assert sstats["sampled"] > 0                                      # each shard has blocks of its own to colour
        color_call(torch, sh.table, frames[1], image(1), BAND, 255)
        part = colors_by_key(check_against_rule(sh.table, spre, swant, sentries))
        assert not set(part) & set(union)
        union.update(part)
    assert union.keys() == whole.keys()
    for k in whole:
        assert np.array_equal(union[k], whole[k]), k
    for sh in shards:
        sh.table.close()
    full.close()


# ---- 7. deletion and collection --------------------------------------------------------------------------------------------
def test_freed_blocks_lose_their_colour(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [1])
    color_call(torch, gt, frames[1], image(1), 3.0 * VS, 255)
    pre = snapshot(gt)
    alloc = pre["table"][pre["table"]["ptr"] != -1]
    coloured = [e for e in alloc if pre["color"][int(e["ptr"]):int(e["ptr"]) + 512].any()]
    victims = coloured[::2]
    assert len(victims) >= 5 and len(coloured) > len(victims)
    keys = np.array([list(e["pos"]) + [0] for e in victims], np.int32)
    gt.delete_blocks(dev(torch, keys))
    post = snapshot(gt)
    want = pre["color"].copy()
    for e in victims:
        want[int(e["ptr"]):int(e["ptr"]) + 512] = 0
    assert np.array_equal(post["color"], want)                            # the freed blocks' words, and only those
    assert gt.counters()["last_freed"] == len(victims)
    # the same frame again: the deleted keys come back in re-dealt blocks, which show no old colour
    fuse_depth(torch, gt, frames, [1])
    again = snapshot(gt)
    back = {tuple(e["pos"].tolist()): int(e["ptr"]) for e in again["table"][again["table"]["ptr"] != -1]}
    freed = {int(e["ptr"]) for e in victims}
    dealt = {back[tuple(e["pos"].tolist())] for e in victims}
    assert dealt & freed, "no freed block was handed out again: the scene does not test the re-deal"
    for p in dealt:
        assert not again["color"][p:p + 512].any()
    assert np.array_equal(again["color"], want)
    # garbage collection goes through the same release: the frame taken out again leaves blocks that hold nothing but whose
    # colour was never swept; collecting them zeroes it
    color_call(torch, gt, frames[1], image(1), 3.0 * VS, 255)
    for _ in range(2):                                                    # (the kept blocks hold the frame twice)
        gt.deintegrate_depth(frames[1][0], dev(torch, frames[1][1]), DC.k_inv())
    pre = snapshot(gt)
    assert pre["color"].any() and not pre["vox"].view(U).any()
    held = int((pre["table"]["ptr"] != -1).sum())                         # (the second pass of the frame may have placed keys
    assert held >= len(alloc)                                             # that lost their bucket's lock in the first)
    gt.garbage_collect(0.0)
    post = snapshot(gt)
    assert len(gt.allocated()) == 0 and gt.counters()["last_freed"] == held
    assert not post["color"].any()
    gt.close()


# ---- 8. de-integration and the sweep ---------------------------------------------------------------------------------------
def test_deintegrate_then_sweep_clears_exactly_the_emptied_voxels(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    gt = table(vh, 1)
    for i in (0, 1, 2):
        fuse_depth(torch, gt, frames, [i])
        color_call(torch, gt, frames[i], image(i), 3.0 * VS, 255)
    before = snapshot(gt)
    gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    pre = snapshot(gt)
    assert np.array_equal(pre["color"], before["color"])                  # a de-integration does not touch colour
    orphaned = (pre["color"] != 0) & ~(pre["vox"]["weight"] > 0)
    assert orphaned.sum() > 100
    want, entries, stats = expected(oracle, gt, pre, 1, pose, (d16, DC.k_inv()), image(1), 3.0 * VS, 0)
    assert stats["sampled"] == 0
    color_call(torch, gt, frames[1], image(1), 3.0 * VS, 0)
    post = check_against_rule(gt, pre, want, entries)
    changed = post["color"] != pre["color"]
    listed = np.zeros(WORDS, bool)
    listed[(entries["ptr"].astype(np.int64)[:, None] + np.arange(512)).ravel()] = True
    assert np.array_equal(changed, orphaned & listed) and changed.sum() > 100
    assert not post["color"][changed].any()                               # cleared, and nothing added anywhere
    gt.close()


# ---- 9. snapshots ----------------------------------------------------------------------------------------------------------
def test_load_snapshot_clears_the_colour(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [0, 1])
    color_call(torch, gt, frames[1], image(1), BAND, 255)
    pre = snapshot(gt)
    assert pre["color"].any()
    path = str(tmp_path / "model.vhsnap")
    gt.save_snapshot(path)
    gt.load_snapshot(path)
    post = snapshot(gt)
    assert gt.has_color() and not post["color"].any()
    assert np.array_equal(post["table"], pre["table"]) and np.array_equal(post["vox"].view(U), pre["vox"].view(U))
    # and colour fuses again on the loaded model, by the rule
    want, entries, stats = expected(oracle, gt, post, 1, frames[1][0], (frames[1][1], DC.k_inv()), image(2), BAND, 255)
    color_call(torch, gt, frames[1], image(2), BAND, 255)
    check_against_rule(gt, post, want, entries)
    gt.close()


# ---- 10. the composition ---------------------------------------------------------------------------------------------------
def test_integrate_depth_color_is_its_composition(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    a, b = table(vh, 1), table(vh, 1)
    for i in (0, 1):
        pose, d16, _ = frames[i]
        a.integrate_depth_color(pose, dev(torch, d16), DC.k_inv(), dev(torch, image(i)), BAND, 255)
        b.integrate_depth(pose, dev(torch, d16), DC.k_inv())
        b.integrate_color(pose, dev(torch, d16), DC.k_inv(), dev(torch, image(i)), BAND, 255)
    sa, sb = snapshot(a), snapshot(b)
    ma, mb = model_of(sa), model_of(sb)
    assert ma.keys() == mb.keys() and sa["occupied"] == sb["occupied"] and sa["color"].any()
    for k in ma:
        for x, y in zip(ma[k], mb[k]):
            assert np.array_equal(x.view(U), y.view(U)), k
    a.close()
    b.close()


# ---- 11. sampling ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coloured(oracle, vh, torch_cuda):
    """A model fused with a truncation equal to the colour band (three voxels), so that every voxel next to the zero level
    has a colour sample, and with blocks allocated over that band, so that cells at block corners have all their eight blocks;
    (context, snapshot, ColorField)."""
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1, truncation=3.0 * VS)
    gt.set_alloc_band(3.0 * VS)
    for i in (0, 1, 2):
        fuse_depth(torch, gt, frames, [i])
        color_call(torch, gt, frames[i], image(i), 3.0 * VS, 255)
    snap = snapshot(gt)
    yield gt, snap, CR.ColorField(model_of(snap))
    gt.close()


def gpu_sample(torch, gt, pts, mode):
    out = gt.sample_color(dev(torch, np.ascontiguousarray(pts, F)), mode)
    gt.synchronize()
    return out.cpu().numpy()


def corner_offsets():
    return [np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64) for c in range(8)]


def crafted_points(snap, field):
    """Named point sets [n, 3] float32, found in the model itself: points in cells whose eight corners are all coloured, by
    the number of block faces the cell crosses (0..3: the cell spans 1, 2, 4 or 8 blocks); points in cells with eight valid
    corners of which exactly one has no colour; lattice points; an absent block, NaN and out-of-domain points."""
    alloc = snap["table"][snap["table"]["ptr"] != -1]
    keys = alloc["pos"].astype(np.int64)
    rng = np.random.default_rng(7)
    lin = np.arange(512)
    g = (keys[:, None, :] * 8 + np.stack([lin & 7, (lin >> 3) & 7, lin >> 6], 1)[None, :, :]).reshape(-1, 3)
    have = np.stack([field.words(g + d) >> U(24) > 0 for d in corner_offsets()], 0)
    valid = np.stack([~np.isnan(field.voxels(g + d)[0]) for d in corner_offsets()], 0)
    crossed = ((g & 7) == 7).sum(1)
    out = {}
    for k in range(4):
        cells = g[valid.all(0) & have.all(0) & (crossed == k)][:150]
        out[f"span{k}"] = (cells + rng.random((len(cells), 3)).astype(F)).astype(F) * F(VS)
    seven = g[valid.all(0) & (have.sum(0) == 7)][:150]
    out["seven"] = (seven + F(0.5)).astype(F) * F(VS)
    out["lattice"] = g[rng.permutation(len(g))[:400]].astype(F) * F(VS)
    out["anywhere"] = (g[rng.permutation(len(g))[:400]] + rng.random((400, 3)).astype(F)).astype(F) * F(VS)
    out["special"] = np.array([[400.0, 400.0, 400.0], [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -3e30], [4.5e7, 0.1, 0.1]], F)
    return out


@pytest.mark.parametrize("mode", [NEAREST, TRILINEAR], ids=["nearest", "trilinear"])
def test_sampling_against_the_rule(coloured, torch_cuda, mode):
    gt, snap, field = coloured
    sets = crafted_points(snap, field)
    for name, pts in sets.items():                                        # conditions on the inputs, by the reference itself
        want = CR.sample(field, pts, VS, mode)
        print(name, len(pts), int((want != 0).sum()))
        assert len(pts) > 0, f"no {name} point: the scene does not test it"
        if name.startswith("span"):
            # (a few land in a neighbouring cell: p / voxelSize is rounded) nearly all have a colour in both modes
            assert (want != 0).sum() >= 0.9 * len(pts), name
        if name == "seven" and mode == TRILINEAR:
            assert not want.any()                                         # one uncoloured corner: no trilinear sample ...
            assert not np.isnan(S.sample(field, pts, VS, S.TRILINEAR)[0]).any()    # ... where the sdf has one
        if name == "special":
            assert not want.any()
        if name == "lattice":
            assert 0 < (want != 0).sum() < len(pts)
    pts = np.concatenate(list(sets.values())).astype(F)
    want = CR.sample(field, pts, VS, mode)
    got = gpu_sample(torch_cuda, gt, pts, mode)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), pts[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert (want != 0).sum() > 257
    for n in (1, 63, 257):                                                # a lone lane, a wave short of one, a block and a lane
        part = pts[::2][:n]
        assert len(part) == n
        assert np.array_equal(gpu_sample(torch_cuda, gt, part, mode), CR.sample(field, part, VS, mode))


def test_sampling_camera_frame_points(coloured, torch_cuda):
    torch = torch_cuda
    gt, snap, field = coloured
    pose = DC.POSES[1]
    sets = crafted_points(snap, field)
    world = np.concatenate([sets["span0"], sets["span3"], sets["anywhere"]])
    inv = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4))
    cam = np.concatenate([world.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3], np.ones((len(world), 1))], 1).astype(F)
    cam[::7, 2] = 0.0                                                     # no point
    for mode in (NEAREST, TRILINEAR):
        want = CR.sample_map(field, pose, cam, VS, mode)
        assert (want != 0).sum() > 100 and not want[::7].any()
        out = torch.empty((len(cam),), dtype=torch.uint32, device="cuda")
        gt.sample_color_map_into(pose, dev(torch, cam), out, mode)
        gt.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)


def test_mesh_vertices_have_colour(coloured, torch_cuda, tmp_path):
    from voxelhashing_demo_amd import mesh_io
    gt, snap, field = coloured
    verts, faces, colors = gt.extract_mesh_indexed(colors=True)
    assert len(verts) > 1000 and len(colors) == len(verts)
    near, tri = CR.sample(field, verts, VS, NEAREST), CR.sample(field, verts, VS, TRILINEAR)
    assert (near != 0).all()                                              # every vertex has a nearest colour ...
    assert (tri != 0).sum() >= 100                                        # ... and many a trilinear one, by the reference's count
    assert np.array_equal(gpu_sample(torch_cuda, gt, verts, NEAREST), near)
    assert np.array_equal(gpu_sample(torch_cuda, gt, verts, TRILINEAR), tri)
    assert np.array_equal(colors, np.where(tri != 0, tri, near))
    path = str(tmp_path / "mesh.ply")
    mesh_io.save_ply(path, verts, faces, colors=colors)
    v, f, n, c = mesh_io.load_ply(path)
    assert np.array_equal(v, verts) and np.array_equal(f, faces) and n is None
    assert np.array_equal(c, np.stack([(colors >> U(k)) & U(255) for k in (0, 8, 16)], 1).astype(np.uint8))
    plain = str(tmp_path / "plain.ply")
    mesh_io.save_ply(plain, verts, faces)
    assert len(mesh_io.load_ply(plain)) == 3


def test_raycast_color_is_raycast_maps_then_sample_color_map(coloured, torch_cuda):
    torch = torch_cuda
    gt, snap, field = coloured
    pose = DC.POSES[1]
    for mode in (NEAREST, TRILINEAR):
        depth, verts, nrm, rgba = gt.render_color(pose, 0.1, 5.0, mode)
        d2 = torch.empty_like(depth)
        v2, n2 = torch.empty_like(verts), torch.empty_like(nrm)
        gt.raycast_maps(pose, d2, v2, n2, 0.1, 5.0)
        c2 = torch.empty((H * W,), dtype=torch.uint32, device="cuda")
        gt.sample_color_map_into(pose, v2, c2, mode)
        gt.synchronize()
        got = rgba.cpu().numpy()
        assert np.array_equal(depth.cpu().numpy().view(U), d2.cpu().numpy().view(U))
        assert np.array_equal(verts.cpu().numpy().view(U), v2.cpu().numpy().view(U))
        assert np.array_equal(nrm.cpu().numpy().view(U), n2.cpu().numpy().view(U))
        assert np.array_equal(got.ravel(), c2.cpu().numpy())
        assert (got != 0).sum() >= 100, (got != 0).sum()
        assert ((got >> U(24)) == 255)[got != 0].all()
        assert np.array_equal(got.ravel(), CR.sample_map(field, pose, verts.cpu().numpy().reshape(-1, 4), VS, mode))


# ---- 12. no volume, refusals -----------------------------------------------------------------------------------------------
def test_no_volume_and_refusals(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, verts = frames[1]
    L = vh.load()
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [0, 1])
    # before any colour: every sample is 0, nothing is allocated
    alloc = gt.allocated()
    pts = (alloc["pos"].astype(np.int64) * 8 + 3).astype(F) * F(VS)
    for mode in (NEAREST, TRILINEAR):
        out = torch.full((len(pts),), 0x55, dtype=torch.int32, device="cuda")
        gt.sample_color_into(dev(torch, pts), out, mode)
        gt.synchronize()
        assert not out.cpu().numpy().any()
    assert not gt.has_color()
    host = np.zeros(4, U)
    hp = host.ctypes.data_as(C.c_void_p)
    assert L.vh_download_color(gt._h, 0, hp, 4) == INVALID                # no volume
    gt.clear_color()                                                      # nothing to clear: fine
    pre = snapshot(gt)
    p16 = np.ascontiguousarray(pose, F).reshape(16)
    pp = p16.ctypes.data_as(C.POINTER(C.c_float))
    k = DC.k_inv().reshape(9).copy()
    kp = k.ctypes.data_as(C.POINTER(C.c_float))
    dd, dv, dc = dev(torch, d16), dev(torch, verts), dev(torch, image(1))
    h, band = gt._h, C.c_float(BAND)
    d, v, c = dd.data_ptr(), dv.data_ptr(), dc.data_ptr()
    for fn in (L.vh_integrate_color, L.vh_integrate_depth_color):
        assert fn(None, pp, d, kp, c, band, 255) == INVALID
        assert fn(h, None, d, kp, c, band, 255) == INVALID
        assert fn(h, pp, None, kp, c, band, 255) == INVALID
        assert fn(h, pp, d, None, c, band, 255) == INVALID
        assert fn(h, pp, d, kp, None, band, 255) == INVALID
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            assert fn(h, pp, d, kp, c, C.c_float(bad), 255) == INVALID
        for bad in (-1, 256):
            assert fn(h, pp, d, kp, c, band, bad) == INVALID
    assert L.vh_integrate_color_map(None, pp, v, c, band, 255) == INVALID
    assert L.vh_integrate_color_map(h, None, v, c, band, 255) == INVALID
    assert L.vh_integrate_color_map(h, pp, None, c, band, 255) == INVALID
    assert L.vh_integrate_color_map(h, pp, v, None, band, 255) == INVALID
    assert L.vh_integrate_color_map(h, pp, v, c, C.c_float(0.0), 255) == INVALID
    assert L.vh_integrate_color_map(h, pp, v, c, band, 256) == INVALID
    out = torch.zeros((W * H,), dtype=torch.int32, device="cuda")
    o = out.data_ptr()
    assert L.vh_sample_color(None, 0, 4, v, o) == INVALID
    assert L.vh_sample_color(h, 2, 4, v, o) == INVALID
    assert L.vh_sample_color(h, 0, 4, None, o) == INVALID
    assert L.vh_sample_color(h, 0, 4, v, None) == INVALID
    assert L.vh_sample_color(h, 0, 1 << 31, v, o) == INVALID
    assert L.vh_sample_color(h, 0, 0, None, None) == 0
    assert L.vh_sample_color_map(h, 0, None, 4, v, o) == INVALID
    assert L.vh_sample_color_map(h, 0, pp, 4, None, o) == INVALID
    assert L.vh_raycast_color(h, pp, 0.1, 5.0, o, v, v, 0, None) == INVALID
    assert L.vh_raycast_color(h, pp, 0.1, 5.0, o, v, v, 7, o) == INVALID
    with pytest.raises(ValueError):
        gt.integrate_color(pose, dd, k, dc[:-1], BAND)
    with pytest.raises(ValueError):
        gt.integrate_color(pose, dd, k, dc.cpu(), BAND)
    with pytest.raises(ValueError):
        gt.integrate_color_map(pose, dv, dv[..., 0].contiguous(), BAND)
    post = snapshot(gt)
    assert not gt.has_color()                                             # a refused call allocates nothing
    for name in ("table", "heap", "vox", "compact"):
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    assert post["occupied"] == pre["occupied"] and post["epoch"] == pre["epoch"]
    # with a volume: a download range beyond it
    gt.integrate_color(pose, dd, k, dc, BAND)
    assert gt.has_color()
    assert L.vh_download_color(h, WORDS - 3, hp, 4) == INVALID
    assert L.vh_download_color(h, WORDS + 1, hp, 0) == INVALID
    assert L.vh_download_color(h, 0, None, 4) == INVALID
    assert L.vh_download_color(h, WORDS - 4, hp, 4) == 0
    ptr = int(gt.allocated()["ptr"][0])
    assert np.array_equal(gt.block_colors(ptr), gt.color_volume()[ptr:ptr + 512])
    # a context that holds an imported view
    ot = DC.oracle_table(oracle, 1)
    for i in (0, 1):
        ot.integrate(frames[i][0], frames[i][2])
    records, n = ot.export_view(pose, 512)
    view = vdist.HipViewTable(vh.default_params(**DC.KW), W, H, 1, 1, 512)
    view.recv[:n] = torch.from_numpy(records).cuda()
    torch.cuda.synchronize()
    view.table.import_view(view.recv, n)
    vpre = view.table.hash_table()
    assert L.vh_integrate_color(view.table._h, pp, d, kp, c, band, 255) == INVALID
    assert L.vh_integrate_color_map(view.table._h, pp, v, c, band, 255) == INVALID
    assert L.vh_integrate_depth_color(view.table._h, pp, d, kp, c, band, 255) == INVALID
    assert not view.table.has_color() and np.array_equal(view.table.hash_table(), vpre)
    torch.cuda.synchronize()
    assert np.array_equal(view.recv[:n].cpu().numpy(), records)
    view.table.close()
    ot.close()
    gt.close()
