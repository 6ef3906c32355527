"""The label calls on the GPU against tests/labels_ref.py: around every call the model is downloaded -- hash table, heap, the TSDF
the GPU itself fused, the colour and the label volume -- the rule is applied to the PREVIOUS label volume, and every label word
is compared (the whole volume, so per block key too).  The rule is all integers: no tolerance anywhere.  64x48 images of the
synthetic room, at most 512 blocks (tests/deintegrate_cases.py); label images of tests/labels_cases.py."""
import ctypes as C

import numpy as np
import pytest

import deintegrate_cases as DC
import deintegrate_ref as R
import labels_cases as LC
import labels_ref as LR
from voxelhashing_demo_amd import dist as vdist

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
VS = DC.KW["voxelSize"]
WORDS = DC.KW["numVoxelBlocks"] * 512
BAND = 1.5 * VS
INVALID = 1


def table(vh, sem, width=DC.W, height=DC.H, **kw):
    p = dict(DC.KW)
    p.update(kw)
    gt = vh.SDFHashtable(vh.default_params(**p), width, height, sem)
    gt.set_projection(DC.projection(sem, width, height))
    return gt


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def snapshot(gt):
    gt.synchronize()
    c = gt.counters()
    return dict(table=gt.hash_table(), heap=gt.heap(), vox=gt.sdf_blocks(), heap_counter=c["heap_counter"], occupied=c["occupied"],
                compact=gt.compact(), epoch=c["epoch"], color=gt.color_volume() if gt.has_color() else np.zeros(WORDS, U),
                labels=gt.label_volume() if gt.has_labels() else np.zeros(WORDS, U))


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


def model_of(snap):
    """{key: (sdf, weight, labels, colour)} of the allocated blocks."""
    tab, vox = snap["table"], snap["vox"]
    out = {}
    for e in tab[tab["ptr"] != -1]:
        p = int(e["ptr"])
        out[tuple(e["pos"].tolist())] = (vox["sdf"][p:p + 512], vox["weight"][p:p + 512], snap["labels"][p:p + 512], snap["color"][p:p + 512])
    return out


def labels_by_key(snap):
    return {k: v[2] for k, v in model_of(snap).items()}


def expected(oracle, gt, pre, sem, pose, src, image, band, vote_max):
    """(label volume, entries, stats) by the rule from the downloaded state `pre` (its TSDF is the one the call sees)."""
    proj, inv = DC.projection(sem, gt.width, gt.height), oracle.invert4x4(pose)
    entries = pre["table"][R.visible_entries(pre["table"], gt.params, sem, proj, pose, inv, gt.width, gt.height)]
    want, stats = LR.integrate(pre["labels"], pre["vox"], entries, gt.params, sem, proj, inv, src, image, band, vote_max)
    return want, entries, stats


def check_against_rule(gt, pre, want, entries):
    post = snapshot(gt)
    for name in ("table", "heap", "vox", "color"):                        # the hash table, the heap, the TSDF, colour: unchanged
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    assert post["heap_counter"] == pre["heap_counter"] and post["epoch"] == pre["epoch"]
    assert post["occupied"] == len(entries)                               # the compact list: the flatten's
    assert keys_of(post["compact"]) == keys_of(entries)
    bad = np.nonzero(post["labels"] != want)[0]
    assert len(bad) == 0, (len(bad), bad[:4], post["labels"][bad[:4]], want[bad[:4]], pre["labels"][bad[:4]])
    return post


def unchanged(gt, pre):
    """A reading call changed nothing."""
    post = snapshot(gt)
    for name in ("table", "heap", "vox", "color", "labels", "compact"):
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    assert post["heap_counter"] == pre["heap_counter"] and post["epoch"] == pre["epoch"] and post["occupied"] == pre["occupied"]


def label_call(torch, gt, frame, image, band, vote_max, sensor=True, k_inv=None):
    pose, d16, verts = frame
    if sensor:
        gt.integrate_labels(pose, dev(torch, d16), DC.k_inv() if k_inv is None else k_inv, dev(torch, image), band, vote_max)
    else:
        gt.integrate_labels_map(pose, dev(torch, verts), dev(torch, image), band, vote_max)


def fuse_depth(torch, gt, frames, which, k_inv=None):
    for i in which:
        gt.integrate_depth(frames[i][0], dev(torch, frames[i][1]), DC.k_inv() if k_inv is None else k_inv)


def rgba(i):
    return np.random.default_rng(100 + i).integers(0, 1 << 32, (DC.H, DC.W), dtype=np.uint64).astype(U)


# ---- 1, 2. seven label calls over the three fused frames, at 64x48 and at 33x17 -------------------------------------------------
def seven_calls(oracle, vh, torch, sem, sensor, width, height):
    frames = DC.frames(oracle, width, height)
    kinv = DC.k_inv(width, height)
    gt = table(vh, sem, width, height)
    assert not gt.has_labels()
    for pose, d16, verts in frames:
        if sensor:
            gt.integrate_depth(pose, dev(torch, d16), kinv)
        else:
            gt.integrate(pose, dev(torch, verts))
    total = {}
    for i, f in enumerate(LC.POSE_ORDER):
        pose, d16, verts = frames[f]
        image = LC.image(i, width, height)
        pre = snapshot(gt)
        want, entries, stats = expected(oracle, gt, pre, sem, pose, (d16, kinv) if sensor else verts[..., 2], image, BAND, LC.VOTE_MAX)
        label_call(torch, gt, frames[f], image, BAND, LC.VOTE_MAX, sensor, kinv)
        assert gt.has_labels()
        check_against_rule(gt, pre, want, entries)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    # a condition on the inputs, asserted on the reference alone: every transition of the vote table occurs often, and pixels
    # without a label meet in-band voxels, labelled ones among them
    print(f"{width}x{height} sem {sem}:", total, "votes", np.bincount(LR.votes_of(want)).tolist())
    for k in LR.TRANSITIONS:
        assert total[k] >= 100, (k, total)
    assert total["unlabelled"] >= 100 and total["spared"] > 0 and total["rejected"] > 0
    assert LR.votes_of(want).max() == LC.VOTE_MAX and not gt.has_color()
    gt.close()


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("sensor", [False, True], ids=["vertex-map", "uint16"])
def test_seven_label_calls_over_three_frames(oracle, vh, torch_cuda, sem, sensor):
    seven_calls(oracle, vh, torch_cuda, sem, sensor, DC.W, DC.H)


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("sensor", [False, True], ids=["vertex-map", "uint16"])
def test_seven_label_calls_at_33_by_17(oracle, vh, torch_cuda, sem, sensor):
    """An odd row stride of 2-byte pixels: a kernel that read labels in pairs would show here."""
    seven_calls(oracle, vh, torch_cuda, sem, sensor, 33, 17)


def test_two_workgroups_stride_over_the_list_an_empty_view_and_a_colour_volume(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    gt.set_option("integrate_grid", 2)
    for i in (0, 1, 2):
        gt.integrate_depth_color(frames[i][0], dev(torch, frames[i][1]), DC.k_inv(), dev(torch, rgba(i)), BAND, 255)
    label_call(torch, gt, frames[0], LC.image(0), BAND, 3)
    pre = snapshot(gt)
    assert pre["labels"].any() and pre["color"].any()
    nowhere = (DC.NOWHERE, frames[1][1], frames[1][2])                    # a pose that sees no block: nothing changes
    want, entries, _ = expected(oracle, gt, pre, 1, DC.NOWHERE, (frames[1][1], DC.k_inv()), LC.image(1), BAND, 3)
    assert len(entries) == 0 and np.array_equal(want, pre["labels"])
    label_call(torch, gt, nowhere, LC.image(1), BAND, 3)
    post = check_against_rule(gt, pre, want, entries)
    assert post["occupied"] == 0
    want, entries, stats = expected(oracle, gt, post, 1, frames[1][0], (frames[1][1], DC.k_inv()), LC.image(1), BAND, 3)
    assert len(entries) > 2 and stats["voted"] > 1000
    label_call(torch, gt, frames[1], LC.image(1), BAND, 3)
    check_against_rule(gt, post, want, entries)                           # (colour compared unchanged in there)
    gt.close()


def test_pending_pipelined_frame_is_launched_first(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    snaps = []
    for pipeline in (1, 0):
        gt = table(vh, 1)
        gt.set_option("pipeline", pipeline)
        fuse_depth(torch, gt, frames, [0, 1, 2])                          # pipelined: frame 2's commit + update are still pending
        label_call(torch, gt, frames[2], LC.image(2), BAND, 3)
        snaps.append(snapshot(gt))
        gt.close()
    a, b = labels_by_key(snaps[0]), labels_by_key(snaps[1])
    assert a.keys() == b.keys() and sum(int(v.any()) for v in a.values()) > 10
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert (snaps[0]["labels"] != 0).sum() > 1000


# ---- 3. the sweep ------------------------------------------------------------------------------------------------------------
def test_deintegrate_then_vote_max_zero_clears_exactly_the_emptied_voxels(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    gt = table(vh, 1)
    for i in (0, 1, 2):
        fuse_depth(torch, gt, frames, [i])
        label_call(torch, gt, frames[i], LC.image(i), 3.0 * VS, 3)
    before = snapshot(gt)
    gt.deintegrate_depth(pose, dev(torch, d16), DC.k_inv())
    pre = snapshot(gt)
    assert np.array_equal(pre["labels"], before["labels"])                # a de-integration does not touch labels
    orphaned = (pre["labels"] != 0) & ~(pre["vox"]["weight"] > 0)
    assert orphaned.sum() > 100
    want, entries, stats = expected(oracle, gt, pre, 1, pose, (d16, DC.k_inv()), LC.image(1), 3.0 * VS, 0)
    assert stats["voted"] == 0 and stats["swept"] > 100
    label_call(torch, gt, frames[1], LC.image(1), 3.0 * VS, 0)
    post = check_against_rule(gt, pre, want, entries)
    changed = post["labels"] != pre["labels"]
    listed = np.zeros(WORDS, bool)
    listed[(entries["ptr"].astype(np.int64)[:, None] + np.arange(512)).ravel()] = True
    assert np.array_equal(changed, orphaned & listed) and changed.sum() > 100
    assert not post["labels"][changed].any()                              # cleared, and nothing added anywhere
    gt.close()


# ---- 4, 5. reading and counting ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def labelled(oracle, vh, torch_cuda):
    """A model fused with a truncation equal to the label band (three voxels), labelled by seven calls with one image from the
    three poses and a cap of 5: the views agree except at patch borders and noise pixels, so votes run from 1 to 5; (context,
    snapshot, LabelField)."""
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1, truncation=3.0 * VS)
    gt.set_alloc_band(3.0 * VS)
    fuse_depth(torch, gt, frames, [0, 1, 2])
    for i, f in enumerate(LC.POSE_ORDER):
        label_call(torch, gt, frames[f], LC.image(0, noise=0.1), 3.0 * VS, 5)
    snap = snapshot(gt)
    yield gt, snap, LR.LabelField(model_of(snap))
    gt.close()


def crafted_points(snap):
    """World points [n, 3] float32: inside labelled voxels of every vote count (jittered within the voxel), inside voxels of
    allocated blocks that are not valid, then a far point, NaN, infinities and an out-of-domain point."""
    rng = np.random.default_rng(7)
    model = model_of(snap)
    lin = np.arange(512)
    local = np.stack([lin & 7, (lin >> 3) & 7, lin >> 6], 1)
    g, words, valid = [], [], []
    for k, v in model.items():
        g.append(np.array(k, np.int64) * 8 + local)
        words.append(v[2])
        valid.append(LR.valid_mask(v[0], v[1]))
    g, words, valid = np.concatenate(g), np.concatenate(words), np.concatenate(valid)
    votes = LR.votes_of(words)
    picks = [np.nonzero(valid & (votes == n))[0][:300] for n in range(1, 6)]
    assert all(len(p) > 0 for p in picks), [len(p) for p in picks]
    invalid = np.nonzero(~valid)[0][:100]
    assert len(invalid) > 0
    at = np.concatenate(picks + [invalid])
    jitter = (rng.random((len(at), 3)) * 0.98 - 0.49)
    pts = ((g[at] + jitter).astype(F) * F(VS)).astype(F)
    special = np.array([[400.0, 400.0, 400.0], [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -3e30], [4.5e7, 0.1, 0.1]], F)
    return np.concatenate([pts, special]).astype(F), len(at) - len(invalid), len(invalid)


def gpu_sample(torch, gt, pts, min_votes):
    out = gt.sample_labels(dev(torch, np.ascontiguousarray(pts, F)), min_votes)
    gt.synchronize()
    return out.cpu().numpy()


def test_sampling_against_the_rule(labelled, torch_cuda):
    gt, snap, field = labelled
    pts, n_labelled, n_invalid = crafted_points(snap)
    seen = []
    for min_votes in (1, 2, 4):
        want = LR.sample(field, pts, VS, min_votes)
        # conditions on the inputs, by the reference itself: nearly all labelled points read a word (a few land in a
        # neighbouring voxel: p / voxelSize is rounded), the rest read none, and every threshold cuts some away
        assert not want[n_labelled:].any()
        assert (LR.votes_of(want[want != 0]) >= min_votes).all()
        seen.append(int((want != 0).sum()))
        got = gpu_sample(torch_cuda, gt, pts, min_votes)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (min_votes, len(bad), pts[bad[:4]], got[bad[:4]], want[bad[:4]])
    print("points with a word at min_votes 1, 2, 4:", seen, "of", n_labelled)
    assert seen[0] >= 0.9 * n_labelled and seen[0] > seen[1] > seen[2] > 0
    assert np.array_equal(gpu_sample(torch_cuda, gt, pts, 0), gpu_sample(torch_cuda, gt, pts, 1))      # max(min_votes, 1)
    assert np.array_equal(gpu_sample(torch_cuda, gt, pts, -5), gpu_sample(torch_cuda, gt, pts, 1))
    for n in (1, 63, 257):                                                # a lone lane, a wave short of one, a block and a lane
        part = pts[::2][:n]
        assert np.array_equal(gpu_sample(torch_cuda, gt, part, 1), LR.sample(field, part, VS, 1))
    unchanged(gt, snap)


def test_sampling_camera_frame_points_and_the_raycast(labelled, torch_cuda):
    torch = torch_cuda
    gt, snap, field = labelled
    pose = DC.POSES[1]
    pts, n_labelled, _ = crafted_points(snap)
    world = pts[:n_labelled]
    inv = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4))
    cam = np.concatenate([world.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3], np.ones((len(world), 1))], 1).astype(F)
    cam[::7, 2] = 0.0                                                     # no point
    for min_votes in (1, 2, 4):
        want = LR.sample_map(field, pose, cam, VS, min_votes)
        assert (want != 0).sum() > 100 and not want[::7].any()
        out = torch.full((len(cam),), 0x55, dtype=torch.int32, device="cuda")
        gt.sample_labels_map_into(pose, dev(torch, cam), out, min_votes)
        gt.synchronize()
        assert np.array_equal(out.cpu().numpy().view(U), want)
    for min_votes in (1, 4):
        depth, verts, nrm, words = gt.render_labels(pose, 0.1, 5.0, min_votes)
        d2 = torch.empty_like(depth)
        v2, n2 = torch.empty_like(verts), torch.empty_like(nrm)
        gt.raycast_maps(pose, d2, v2, n2, 0.1, 5.0)
        w2 = torch.empty((DC.H * DC.W,), dtype=torch.uint32, device="cuda")
        gt.sample_labels_map_into(pose, v2, w2, min_votes)
        gt.synchronize()
        got = words.cpu().numpy()
        assert np.array_equal(depth.cpu().numpy().view(U), d2.cpu().numpy().view(U))
        assert np.array_equal(verts.cpu().numpy().view(U), v2.cpu().numpy().view(U))
        assert np.array_equal(nrm.cpu().numpy().view(U), n2.cpu().numpy().view(U))
        assert np.array_equal(got.ravel(), w2.cpu().numpy())
        assert min_votes > 1 or (got != 0).sum() >= 100, (got != 0).sum()
        assert np.array_equal(got.ravel(), LR.sample_map(field, pose, verts.cpu().numpy().reshape(-1, 4), VS, min_votes))
    unchanged(gt, snap)


def test_mesh_vertices_have_labels(labelled, torch_cuda):
    gt, snap, field = labelled
    verts, faces = gt.extract_mesh_indexed()
    v2, f2, words = gt.extract_mesh_indexed(labels=True)
    assert np.array_equal(verts, v2) and np.array_equal(faces, f2) and len(words) == len(verts) > 1000
    want = LR.sample(field, verts, VS, 1)
    assert np.array_equal(words, want) and (want != 0).sum() > 100


def test_a_table_without_a_volume_reads_zeros(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [0, 1])
    alloc = gt.allocated()
    pts = (alloc["pos"].astype(np.int64) * 8 + 3).astype(F) * F(VS)
    out = torch.full((len(pts),), 0x55, dtype=torch.int32, device="cuda")
    gt.sample_labels_into(dev(torch, pts), out)
    gt.synchronize()
    assert not out.cpu().numpy().any()
    _, _, _, words = gt.render_labels(DC.POSES[1], 0.1, 5.0)
    gt.synchronize()
    assert not words.cpu().numpy().any()
    snap = snapshot(gt)
    model = model_of(snap)
    valid = sum(int(LR.valid_mask(v[0], v[1]).sum()) for v in model.values())
    got = gt.label_counts(4).cpu().numpy()
    assert got.tolist() == [valid, 0, 0, 0] and valid > 1000              # no volume: everything goes to bin 0
    assert not gt.has_labels()
    gt.close()


def test_label_counts_against_bincount(labelled, torch_cuda):
    torch = torch_cuda
    gt, snap, field = labelled
    model = model_of(snap)
    valid = sum(int(LR.valid_mask(v[0], v[1]).sum()) for v in model.values())
    keys = np.array(list(model))
    mid = (keys.min(0) + keys.max(0)) // 2
    regions = [None, (keys.min(0), mid + 1), (mid, keys.max(0) + 1), ((0, 0, 0), (0, 5, 5))]
    assert 0 < sum(LR.in_region(k, regions[1]) for k in model) < len(model)
    for region in regions:
        inside = {k: v for k, v in model.items() if LR.in_region(k, region)}
        total = sum(int(LR.valid_mask(v[0], v[1]).sum()) for v in inside.values())
        for n_bins in (1, 3, 65536):
            for min_votes in (1, 3):
                # numpy.bincount over the downloaded model, written out here (labels_ref.counts is the same thing)
                l = np.concatenate([np.where(LR.votes_of(v[2]) >= min_votes, LR.label_of(v[2]), 0)[LR.valid_mask(v[0], v[1])]
                                    for v in inside.values()] + [np.zeros(0, U)]).astype(np.int64)
                want = np.bincount(np.where(l < n_bins, l, 0), minlength=n_bins)
                assert np.array_equal(want, LR.counts(model, n_bins, min_votes, region))
                counts = torch.full((n_bins + 1,), 0x55, dtype=torch.int32, device="cuda")     # (the call zeroes the buffer itself)
                gt.label_counts_into(counts, n_bins, region, min_votes)
                gt.synchronize()
                got = counts.cpu().numpy()
                assert got[n_bins] == 0x55
                assert np.array_equal(got[:n_bins], want), (region, n_bins, min_votes, got[:8], want[:8])
                assert got[:n_bins].sum() == total                        # the bins sum to the valid voxels of the region
    full = gt.label_counts(65536).cpu().numpy()
    assert full.sum() == valid and set(np.nonzero(full)[0].tolist()) == {0, 1, 2, 3} and full[1:4].min() > 100
    assert gt.label_counts(3).cpu().numpy()[0] == full[0] + full[3]       # a label >= n_bins is counted in bin 0
    unchanged(gt, snap)


# ---- 6. removing a label -------------------------------------------------------------------------------------------------------
def same_model(a, b):
    assert a.keys() == b.keys()
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(np.asarray(x).view(U), np.asarray(y).view(U)), k


def pool_invariant(snap):
    """A pool block that is not allocated has 512 zero label (and colour) words."""
    free = np.ones(WORDS, bool)
    for e in snap["table"][snap["table"]["ptr"] != -1]:
        free[int(e["ptr"]):int(e["ptr"]) + 512] = False
    assert not snap["labels"][free].any() and not snap["color"][free].any()


@pytest.mark.parametrize("band, colour, frees", [(10.0, True, True), (1.5 * VS, False, False)], ids=["band-10", "band-1.5-voxels"])
def test_remove_label(oracle, vh, torch_cuda, band, colour, frees):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [1])
    if colour:
        gt.integrate_color(pose, dev(torch, d16), DC.k_inv(), dev(torch, rgba(1)), band, 255)
    label_call(torch, gt, frames[1], LC.halves(), band, 3)
    pre = snapshot(gt)
    pool_invariant(pre)
    model = model_of(pre)
    want, want_stats, freed = LR.remove(model, 7)
    touched = [k for k, v in model.items() if (LR.label_of(v[2]) == 7).any()]
    kept = [k for k in touched if k in want]
    print(f"band {band}: touched {len(touched)}, freed {len(freed)}, kept {len(kept)}")
    assert len(touched) > 0 and (pre["color"].any() == colour)
    if frees:
        assert len(freed) > 0 and len(kept) > 0
    else:
        assert len(freed) == 0
    stats = gt.remove_label(7)
    assert stats == want_stats, (stats, want_stats)
    post = snapshot(gt)
    same_model(model_of(post), want)                                      # the allocated keys; voxels, labels, colour per key
    pool_invariant(post)
    assert gt.counters()["last_freed"] == len(freed)
    assert (LR.label_of(post["labels"]) == 9).any() and not (LR.label_of(post["labels"]) == 7).any()
    # a region that holds no block, min_votes above every count, and the same label again: nothing more goes
    assert gt.remove_label(9, region=((0, 0, 0), (0, 9, 9))) == dict(blocks=0, removed_voxels=0, freed_blocks=0)
    assert gt.remove_label(9, min_votes=2)["removed_voxels"] == 0
    assert gt.remove_label(7) == dict(blocks=len(want), removed_voxels=0, freed_blocks=0)
    same_model(model_of(snapshot(gt)), want)
    # the same frame again: the freed keys come back in re-dealt blocks, which show no old label
    fuse_depth(torch, gt, frames, [1])
    again = snapshot(gt)
    back = model_of(again)
    assert not freed or any(k in back for k in freed), "no freed key came back: the scene does not test the re-deal"
    for k in freed:
        assert k not in back or (not back[k][2].any() and not back[k][3].any())
    assert np.array_equal(again["labels"], post["labels"])
    pool_invariant(again)
    gt.close()


def test_remove_label_in_a_region_with_min_votes(labelled_copy, torch_cuda):
    gt, pre = labelled_copy
    model = model_of(pre)
    keys = np.array(list(model))
    region = (keys.min(0), (keys.min(0) + keys.max(0)) // 2 + 1)
    want, want_stats, freed = LR.remove(model, 2, min_votes=2, region=region)
    assert 0 < want_stats["blocks"] < len(model) and want_stats["removed_voxels"] > 0
    assert any((LR.label_of(v[2]) == 2).any() for k, v in want.items() if LR.in_region(k, region))      # the one-vote words stay
    stats = gt.remove_label(2, min_votes=2, region=region)
    assert stats == want_stats
    post = snapshot(gt)
    same_model(model_of(post), want)
    pool_invariant(post)


@pytest.fixture()
def labelled_copy(oracle, vh, torch_cuda):
    """A labelled, coloured model of its own for a test that changes it; (context, snapshot)."""
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    for i in (0, 1, 2):
        gt.integrate_depth_color(frames[i][0], dev(torch, frames[i][1]), DC.k_inv(), dev(torch, rgba(i)), 3.0 * VS, 255)
    for i, f in enumerate(LC.POSE_ORDER[:4]):
        label_call(torch, gt, frames[f], LC.image(0, noise=0.1), 3.0 * VS, 5)
    yield gt, snapshot(gt)
    gt.close()


# ---- 7. housekeeping -----------------------------------------------------------------------------------------------------------
def test_freed_blocks_lose_their_labels(labelled_copy, oracle, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt, pre = labelled_copy
    alloc = pre["table"][pre["table"]["ptr"] != -1]
    with_labels = [e for e in alloc if pre["labels"][int(e["ptr"]):int(e["ptr"]) + 512].any()]
    victims = with_labels[::2]
    assert len(victims) >= 5 and len(with_labels) > len(victims)
    keys = np.array([list(e["pos"]) + [0] for e in victims], np.int32)
    gt.delete_blocks(dev(torch, keys))
    post = snapshot(gt)
    want = pre["labels"].copy()
    for e in victims:
        want[int(e["ptr"]):int(e["ptr"]) + 512] = 0
    assert np.array_equal(post["labels"], want)                           # the freed blocks' words, and only those
    assert gt.counters()["last_freed"] == len(victims)
    pool_invariant(post)


def test_collected_blocks_lose_their_labels(oracle, vh, torch_cuda):
    """Garbage collection goes through the same release: a frame taken out again leaves blocks that hold nothing but whose
    labels were never swept; collecting them zeroes the words."""
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [1])
    label_call(torch, gt, frames[1], LC.image(1), 3.0 * VS, 3)
    gt.deintegrate_depth(frames[1][0], dev(torch, frames[1][1]), DC.k_inv())
    mid = snapshot(gt)
    assert mid["labels"].any() and not mid["vox"].view(U).any()
    held = int((mid["table"]["ptr"] != -1).sum())
    gt.garbage_collect(0.0)
    post = snapshot(gt)
    assert len(gt.allocated()) == 0 and gt.counters()["last_freed"] == held and not post["labels"].any()
    gt.close()


def test_load_snapshot_clears_the_labels(labelled_copy, oracle, torch_cuda, tmp_path):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt, pre = labelled_copy
    path = str(tmp_path / "model.vhsnap")
    gt.save_snapshot(path)
    gt.load_snapshot(path)
    post = snapshot(gt)
    assert gt.has_labels() and pre["labels"].any() and not post["labels"].any()
    assert np.array_equal(post["table"], pre["table"]) and np.array_equal(post["vox"].view(U), pre["vox"].view(U))
    # and labels fuse again on the loaded model, by the rule
    want, entries, stats = expected(oracle, gt, post, 1, frames[1][0], (frames[1][1], DC.k_inv()), LC.image(2), BAND, 3)
    label_call(torch, gt, frames[1], LC.image(2), BAND, 3)
    check_against_rule(gt, post, want, entries)
    gt.clear_labels()
    gt.synchronize()
    assert gt.has_labels() and not gt.label_volume().any()


# ---- 8. the overflow list, and two shards --------------------------------------------------------------------------------------
def test_chained_entries_are_labelled_counted_and_removed(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    nb, bs = 32, 2                                                        # (few buckets: that is what makes chains)
    gt = table(vh, 1, numBuckets=nb, bucketSize=bs, attachedLinkedListSize=8)
    gt.set_option("overflow_list", 1)
    for _ in range(6):                                                    # (a bucket takes one new entry per frame)
        fuse_depth(torch, gt, frames, [0, 1, 2])
    pre = snapshot(gt)
    want, entries, stats = expected(oracle, gt, pre, 1, pose, (d16, DC.k_inv()), LC.halves(), 10.0, 3)
    idx = R.visible_entries(pre["table"], gt.params, 1, DC.projection(1), pose, oracle.invert4x4(pose), DC.W, DC.H)
    chained = [int(i) for i in idx if oracle.hash_block(*[int(c) for c in pre["table"][i]["pos"]], nb) != i // bs]
    assert chained, "no chained entry is visible: the scene does not test the overflow list"
    assert any(want[int(pre["table"][i]["ptr"]):int(pre["table"][i]["ptr"]) + 512].any() for i in chained)
    label_call(torch, gt, frames[1], LC.halves(), 10.0, 3)
    post = check_against_rule(gt, pre, want, entries)
    model = model_of(post)
    assert np.array_equal(gt.label_counts(16).cpu().numpy(), LR.counts(model, 16))
    after, want_stats, freed = LR.remove(model, 9)
    assert len(freed) > 0
    assert gt.remove_label(9) == want_stats
    end = snapshot(gt)
    same_model(model_of(end), after)
    pool_invariant(end)
    gt.close()


def test_two_shards_together_equal_the_unsharded_volume(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, _ = frames[1]
    world = 2
    params = vh.default_params(**DC.KW)
    plan = vdist.ShardPlan(DC.KW["numBuckets"], world)
    shards = [vdist.HipShard(params, DC.W, DC.H, 1, plan, r, DC.W * DC.H) for r in range(world)]
    full = table(vh, 1)
    for sh in shards:
        sh.table.set_projection(DC.projection(1))
    for a, b in ((0, 1), (2, 1)):
        cams = [frames[a], frames[b]]
        vdist.loopback_step(shards, [[c[0]] for c in cams], [[dev(torch, c[2])] for c in cams])
        vdist.reference_multi_camera_frame(full, [c[0] for c in cams], [dev(torch, c[2]) for c in cams])
    pre = snapshot(full)
    want, entries, stats = expected(oracle, full, pre, 1, pose, (d16, DC.k_inv()), LC.image(1), BAND, 3)
    assert stats["voted"] > 1000
    label_call(torch, full, frames[1], LC.image(1), BAND, 3)
    whole_snap = check_against_rule(full, pre, want, entries)
    whole = labels_by_key(whole_snap)
    union, counts = {}, np.zeros(8, np.int64)
    for sh in shards:
        spre = snapshot(sh.table)
        swant, sentries, sstats = expected(oracle, sh.table, spre, 1, pose, (d16, DC.k_inv()), LC.image(1), BAND, 3)
        assert sstats["voted"] > 0                                        # each shard has blocks of its own to label
        label_call(torch, sh.table, frames[1], LC.image(1), BAND, 3)
        part = labels_by_key(check_against_rule(sh.table, spre, swant, sentries))
        assert not set(part) & set(union)
        union.update(part)
        counts += sh.table.label_counts(8).cpu().numpy()
    assert union.keys() == whole.keys()
    for k in whole:
        assert np.array_equal(union[k], whole[k]), k
    assert np.array_equal(counts, full.label_counts(8).cpu().numpy()) and counts[1:4].min() > 0
    for sh in shards:
        sh.table.close()
    full.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    pose, d16, verts = frames[1]
    L = vh.load()
    gt = table(vh, 1)
    fuse_depth(torch, gt, frames, [0, 1])
    host = np.zeros(4, U)
    hp = host.ctypes.data_as(C.c_void_p)
    assert L.vh_download_labels(gt._h, 0, hp, 4) == INVALID               # no volume
    assert L.vh_remove_label(gt._h, None, 7, 1, None) == INVALID          # no volume
    gt.clear_labels()                                                     # nothing to clear: fine
    pre = snapshot(gt)
    p16 = np.ascontiguousarray(pose, F).reshape(16)
    pp = p16.ctypes.data_as(C.POINTER(C.c_float))
    k = DC.k_inv().reshape(9).copy()
    kp = k.ctypes.data_as(C.POINTER(C.c_float))
    dd, dv, dl = dev(torch, d16), dev(torch, verts), dev(torch, LC.image(1))
    h, band = gt._h, C.c_float(BAND)
    d, v, l = dd.data_ptr(), dv.data_ptr(), dl.data_ptr()
    fn = L.vh_integrate_labels
    assert fn(None, pp, d, kp, l, band, 3) == INVALID
    assert fn(h, None, d, kp, l, band, 3) == INVALID
    assert fn(h, pp, None, kp, l, band, 3) == INVALID
    assert fn(h, pp, d, None, l, band, 3) == INVALID
    assert fn(h, pp, d, kp, None, band, 3) == INVALID
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert fn(h, pp, d, kp, l, C.c_float(bad), 3) == INVALID
    for bad in (-1, 65536):
        assert fn(h, pp, d, kp, l, band, bad) == INVALID
    fm = L.vh_integrate_labels_map
    assert fm(None, pp, v, l, band, 3) == INVALID
    assert fm(h, None, v, l, band, 3) == INVALID
    assert fm(h, pp, None, l, band, 3) == INVALID
    assert fm(h, pp, v, None, band, 3) == INVALID
    assert fm(h, pp, v, l, C.c_float(0.0), 3) == INVALID
    assert fm(h, pp, v, l, band, 65536) == INVALID
    out = torch.zeros((DC.W * DC.H,), dtype=torch.int32, device="cuda")
    o = out.data_ptr()
    assert L.vh_sample_labels(None, 4, v, 1, o) == INVALID
    assert L.vh_sample_labels(h, 4, None, 1, o) == INVALID
    assert L.vh_sample_labels(h, 4, v, 1, None) == INVALID
    assert L.vh_sample_labels(h, 1 << 31, v, 1, o) == INVALID
    assert L.vh_sample_labels(h, 0, None, 1, None) == 0
    assert L.vh_sample_labels_map(h, None, 4, v, 1, o) == INVALID
    assert L.vh_sample_labels_map(h, pp, 4, None, 1, o) == INVALID
    assert L.vh_raycast_labels(h, pp, 0.1, 5.0, o, v, v, 1, None) == INVALID
    assert L.vh_label_counts(None, None, 1, 4, o) == INVALID
    assert L.vh_label_counts(h, None, 1, 4, None) == INVALID
    assert L.vh_label_counts(h, None, 1, 0, o) == INVALID
    assert L.vh_label_counts(h, None, 1, 65537, o) == INVALID
    with pytest.raises(ValueError):
        gt.integrate_labels(pose, dd, k, dl[:-1], BAND)
    with pytest.raises(ValueError):
        gt.integrate_labels(pose, dd, k, dl.cpu(), BAND)
    with pytest.raises(ValueError):
        gt.integrate_labels_map(pose, dv, dv[..., 0].contiguous(), BAND)
    with pytest.raises(ValueError):
        gt.label_counts(0)
    post = snapshot(gt)
    assert not gt.has_labels()                                            # a refused call allocates nothing
    for name in ("table", "heap", "vox", "compact"):
        assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
    assert post["occupied"] == pre["occupied"] and post["epoch"] == pre["epoch"]
    # with a volume: a download range beyond it, and the removal's own refusals
    gt.integrate_labels(pose, dd, k, dl, BAND, 3)
    assert gt.has_labels()
    assert L.vh_download_labels(h, WORDS - 3, hp, 4) == INVALID
    assert L.vh_download_labels(h, WORDS + 1, hp, 0) == INVALID
    assert L.vh_download_labels(h, 0, None, 4) == INVALID
    assert L.vh_download_labels(h, WORDS - 4, hp, 4) == 0
    pre = snapshot(gt)
    assert pre["labels"].any()
    for bad in (0, -1, 65536):
        assert L.vh_remove_label(h, None, bad, 1, None) == INVALID
    assert L.vh_remove_label(None, None, 7, 1, None) == INVALID
    unchanged(gt, pre)
    # a context that holds an imported view
    ot = DC.oracle_table(oracle, 1)
    for i in (0, 1):
        ot.integrate(frames[i][0], frames[i][2])
    records, n = ot.export_view(pose, 512)
    view = vdist.HipViewTable(vh.default_params(**DC.KW), DC.W, DC.H, 1, 1, 512)
    view.recv[:n] = torch.from_numpy(records).cuda()
    torch.cuda.synchronize()
    view.table.import_view(view.recv, n)
    vpre = view.table.hash_table()
    assert fn(view.table._h, pp, d, kp, l, band, 3) == INVALID
    assert fm(view.table._h, pp, v, l, band, 3) == INVALID
    assert L.vh_remove_label(view.table._h, None, 7, 1, None) == INVALID
    assert not view.table.has_labels() and np.array_equal(view.table.hash_table(), vpre)
    out.fill_(0x55)
    view.table.sample_labels_into(dv.reshape(-1, 4)[:, :3].contiguous(), out, n=64)      # a view table: zeros, VH_OK
    view.table.synchronize()
    assert not out.cpu().numpy()[:64].any()
    got = view.table.label_counts(4).cpu().numpy()                        # its valid voxels, all in bin 0
    assert got[0] > 0 and not got[1:].any()
    torch.cuda.synchronize()
    assert np.array_equal(view.recv[:n].cpu().numpy(), records)
    view.table.close()
    ot.close()
    gt.close()
