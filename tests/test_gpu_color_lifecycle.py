"""Colour through de-integration and saved models on the GPU: vh_deintegrate_color against tests/merge_color_ref.py (the whole
colour volume, bit for bit), its two compositions against the calls they are defined as, and vh_save_color / vh_load_color beside
a snapshot.  64x48 frames of the synthetic room, at most 512 blocks (tests/deintegrate_cases.py), a colour image per frame
(tests/merge_color_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as D
import merge_cases as MC
import merge_color_cases as CC
import merge_color_ref as M

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
W, H = DC.W, DC.H
BAND = CC.BAND
INVALID = 1


def coloured(vh, torch, oracle, sem=1, which=(0, 1, 2), bucket_range=None, **kw):
    """A table with the frames `which` fused, depth and colour (image i with frame i), one RGB-D frame after the other."""
    gt = CC.table(vh, DC.KW, sem, bucket_range=bucket_range, **kw)
    frames = DC.frames(oracle)
    for i in which:
        gt.integrate_depth_color(frames[i][0], CC.dev(torch, frames[i][1]), DC.k_inv(), CC.dev(torch, CC.image(i)), BAND, 255)
    return gt


def keys_of(entries):
    return sorted(tuple(p) for p in entries["pos"].tolist())


def same_model(a, b):
    """Two tables built separately: which slot and heap block a key got is free, so per block key."""
    ma, mb = CC.model(a), CC.model(b)
    assert ma.keys() == mb.keys() and a["counters"]["occupied"] == b["counters"]["occupied"]
    assert keys_of(a["compact"][:a["counters"]["occupied"]]) == keys_of(b["compact"][:b["counters"]["occupied"]])
    assert a["counters"]["heap_counter"] == b["counters"]["heap_counter"] and a["counters"]["epoch"] == b["counters"]["epoch"]
    for k in ma:
        for x, y in zip(ma[k], mb[k]):
            assert np.array_equal(x.view(U), y.view(U)), k


def call_frame(torch, frames, i, seed=None):
    pose, d16, _ = frames[i]
    return pose, CC.dev(torch, d16), DC.k_inv(), CC.dev(torch, CC.image(i if seed is None else seed))


# ---- de-integration --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1])
def test_deintegrate_color_against_the_rule(oracle, vh, torch_cuda, sem):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = coloured(vh, torch, oracle, sem)
    proj = DC.projection(sem)
    # the last frame with its own image, then frame 1 with an image that was never fused (the clamp is reached)
    for i, seed in ((2, 2), (1, 7)):
        pose, d16, _ = frames[i]
        pre = CC.snapshot(gt)
        inv = oracle.invert4x4(pose)
        entries = pre["table"][D.visible_entries(pre["table"], gt.params, sem, proj, pose, inv, W, H)]
        want, stats = M.deintegrate(pre["color"], pre["vox"], entries, gt.params, sem, proj, inv, (d16, DC.k_inv()), CC.image(seed), BAND)
        print(f"sem {sem} frame {i}: {stats}")
        assert stats["removed"] > 1000 and stats["emptied"] > 0 and (seed == i or stats["clamped"] > 0)
        gt.deintegrate_color(*call_frame(torch, frames, i, seed), BAND)
        post = CC.snapshot(gt)
        for name in ("table", "heap", "vox"):                                     # only the colour volume changes
            assert np.array_equal(post[name].view(np.uint8), pre[name].view(np.uint8)), name
        assert post["counters"]["occupied"] == len(entries) and post["counters"]["epoch"] == pre["counters"]["epoch"]
        bad = np.nonzero(post["color"] != want)[0]
        assert len(bad) == 0, (len(bad), bad[:4], post["color"][bad[:4]], want[bad[:4]])
        if seed == i:                                                             # the frame added last: within 1 of what was there
            earlier = coloured_before_last(vh, torch, oracle, sem)
            before, after = CC.model(CC.snapshot(earlier)), CC.model(post)
            earlier.close()
            assert before.keys() == after.keys()
            for k in before:
                assert np.array_equal(CR.count(after[k][2]), CR.count(before[k][2])), k
                for a, b in zip(CR.channels(after[k][2]), CR.channels(before[k][2])):
                    assert int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()) <= 1, k
    gt.close()


def coloured_before_last(vh, torch, oracle, sem):
    """All three depth frames, the colour of the first two: what taking frame 2's colour out must come back to."""
    gt = CC.table(vh, DC.KW, sem)
    frames = DC.frames(oracle)
    for i in (0, 1):
        gt.integrate_depth_color(frames[i][0], CC.dev(torch, frames[i][1]), DC.k_inv(), CC.dev(torch, CC.image(i)), BAND, 255)
    gt.integrate_depth(frames[2][0], CC.dev(torch, frames[2][1]), DC.k_inv())
    return gt


def test_compositions_equal_their_definitions(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    a, b = coloured(vh, torch, oracle), coloured(vh, torch, oracle)
    a.deintegrate_depth_color(*call_frame(torch, frames, 1), BAND)
    pose, depth, k, rgba = call_frame(torch, frames, 1)
    b.deintegrate_color(pose, depth, k, rgba, BAND)
    b.deintegrate_depth(pose, depth, k)
    b.integrate_color(pose, depth, k, rgba, BAND, 0)
    sa = CC.snapshot(a)
    same_model(sa, CC.snapshot(b))
    assert not sa["color"][~(sa["vox"]["weight"] > 0)].any()                      # the sweep: nothing that holds nothing keeps colour
    # the frame in again at another pose
    a.reintegrate_depth_color(frames[2][0], frames[0][0], CC.dev(torch, frames[2][1]), DC.k_inv(), CC.dev(torch, CC.image(2)), BAND, 2)
    b.deintegrate_depth_color(*call_frame(torch, frames, 2), BAND)
    b.integrate_depth_color(frames[0][0], CC.dev(torch, frames[2][1]), DC.k_inv(), CC.dev(torch, CC.image(2)), BAND, 2)
    same_model(CC.snapshot(a), CC.snapshot(b))
    a.close()
    b.close()


def test_a_frame_in_and_out_of_an_empty_model_leaves_no_colour(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = coloured(vh, torch, oracle, which=(0,))
    assert (CC.snapshot(gt)["color"] != 0).sum() > 1000
    gt.deintegrate_depth_color(*call_frame(torch, frames, 0), BAND)
    snap = CC.snapshot(gt)
    assert gt.has_color() and not snap["color"].any() and not (snap["vox"]["weight"] > 0).any()
    gt.close()


def test_shards_take_out_their_own(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    whole = coloured(vh, torch, oracle)
    n = DC.KW["numBuckets"]
    # each shard receives its part of the model, colour included (a nearest identity merge into an empty shard is a copy)
    shards = [CC.table(vh, DC.KW, bucket_range=r) for r in ((0, n // 2), (n // 2, n))]
    for sh in shards:
        sh.merge(whole, MC.IDENTITY, 0, colors=True)
        sh.garbage_collect(float("inf"))
    for t in [whole] + shards:
        t.deintegrate_color(*call_frame(torch, frames, 2), BAND)
    want = {k: v[2] for k, v in CC.model(CC.snapshot(whole)).items() if v[1].any()}
    union = {}
    for sh in shards:
        part = {k: v[2] for k, v in CC.model(CC.snapshot(sh)).items()}
        assert part and not set(part) & set(union)
        union.update(part)
    assert union.keys() == want.keys()
    for k in want:
        assert np.array_equal(union[k], want[k]), k
    for t in [whole] + shards:
        t.close()


def test_removal_refusals_change_nothing(oracle, vh, torch_cuda):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = coloured(vh, torch, oracle)
    bare = CC.table(vh, DC.KW)
    bare.integrate_depth(frames[0][0], CC.dev(torch, frames[0][1]), DC.k_inv())
    pre, bare_pre = CC.snapshot(gt), CC.snapshot(bare)
    lib = vh.load()
    fp = C.POINTER(C.c_float)
    pose = np.ascontiguousarray(np.asarray(frames[1][0], F).reshape(16))
    pp, kk = pose.ctypes.data_as(fp), np.ascontiguousarray(DC.k_inv().reshape(9)).ctypes.data_as(fp)
    depth, rgba = CC.dev(torch, frames[1][1]), CC.dev(torch, CC.image(1))
    d, c = depth.data_ptr(), rgba.data_ptr()
    for fn in (lib.vh_deintegrate_color, lib.vh_deintegrate_depth_color):
        assert fn(None, pp, d, kk, c, BAND) == INVALID and fn(gt._h, None, d, kk, c, BAND) == INVALID
        assert fn(gt._h, pp, None, kk, c, BAND) == INVALID and fn(gt._h, pp, d, None, c, BAND) == INVALID
        assert fn(gt._h, pp, d, kk, None, BAND) == INVALID
        for band in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(gt._h, pp, d, kk, c, band) == INVALID
        assert fn(bare._h, pp, d, kk, c, BAND) == INVALID                         # no colour volume: nothing to remove
    re = lib.vh_reintegrate_depth_color
    assert re(gt._h, None, pp, d, kk, c, BAND, 255) == INVALID and re(gt._h, pp, None, d, kk, c, BAND, 255) == INVALID
    assert re(gt._h, pp, pp, d, kk, None, BAND, 255) == INVALID and re(gt._h, pp, pp, d, kk, c, 0.0, 255) == INVALID
    for weight_max in (-1, 256):
        assert re(gt._h, pp, pp, d, kk, c, BAND, weight_max) == INVALID
    assert re(bare._h, pp, pp, d, kk, c, BAND, 255) == INVALID
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), W, H, 1)
    assert lib.vh_deintegrate_color(view._h, pp, d, kk, c, BAND) == INVALID
    with pytest.raises(vh.VoxelHashError, match="invalid argument"):
        bare.deintegrate_depth_color(frames[1][0], depth, DC.k_inv(), rgba, BAND)
    CC.unchanged(pre, CC.snapshot(gt))
    CC.unchanged(bare_pre, CC.snapshot(bare))
    for t in (gt, bare, view):
        t.close()


# ---- save and load ---------------------------------------------------------------------------------------------------------------
def test_snapshot_and_colour_round_trip_and_fusing_goes_on(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    frames = DC.frames(oracle)
    gt = coloured(vh, torch, oracle, which=(0, 1))
    saved = CC.snapshot(gt)
    snap_path, color_path = str(tmp_path / "model.vhs"), str(tmp_path / "model.vhc")
    gt.save_snapshot(snap_path)
    gt.save_color(color_path)
    assert not os.path.exists(color_path + ".partial")
    alloc = int((saved["table"]["ptr"] != -1).sum())
    assert os.path.getsize(color_path) == 32 + alloc * (12 + 2048)
    CC.unchanged(saved, CC.snapshot(gt))                                          # saving changes nothing
    # into a context that holds another coloured model
    other = coloured(vh, torch, oracle, which=(2,))
    other.load_snapshot(snap_path)
    assert other.has_color() and not CC.snapshot(other)["color"].any()            # (the snapshot alone clears the colour)
    other.load_color(color_path)
    loaded = CC.snapshot(other)
    for name in ("table", "heap", "vox", "color"):
        assert np.array_equal(loaded[name].view(np.uint8), saved[name].view(np.uint8)), name
    # and into one that never had a volume
    bare = CC.table(vh, DC.KW)
    bare.load_snapshot(snap_path)
    bare.load_color(color_path)
    assert bare.has_color() and np.array_equal(CC.snapshot(bare)["color"], saved["color"])
    # fusing colour continues as if never interrupted
    for t in (gt, other):
        t.integrate_depth_color(*call_frame(torch, frames, 2), BAND, 255)
    a, b = CC.snapshot(gt), CC.snapshot(other)
    assert (a["color"] != saved["color"]).any()
    same_model(a, b)
    for t in (gt, other, bare):
        t.close()


def test_bad_colour_files_are_refused_with_nothing_changed(oracle, vh, torch_cuda, tmp_path):
    torch = torch_cuda
    gt = coloured(vh, torch, oracle, which=(0, 1))
    other = coloured(vh, torch, oracle, which=(2,))
    bare = CC.table(vh, DC.KW)
    good, foreign = str(tmp_path / "good.vhc"), str(tmp_path / "foreign.vhc")
    gt.save_color(good)
    other.save_color(foreign)
    data = open(good, "rb").read()
    files = {"foreign": foreign}
    for name, content in (("truncated", data[:-100]), ("header-only", data[:32]), ("short-header", data[:10]),
                          ("trailing", data + b"\0" * 4), ("magic", b"VHSNAP01" + data[8:])):
        files[name] = str(tmp_path / (name + ".vhc"))
        open(files[name], "wb").write(content)
    # the same block count and other keys: the sequence of pos is what is compared
    swapped = bytearray(data)
    swapped[32:44] = np.array([1 << 20, 5, -7], np.int32).tobytes()
    files["keys"] = str(tmp_path / "keys.vhc")
    open(files["keys"], "wb").write(bytes(swapped))
    files["missing"] = str(tmp_path / "none.vhc")
    pre = CC.snapshot(gt)
    for name, path in files.items():
        with pytest.raises(vh.VoxelHashError, match="invalid argument"):
            gt.load_color(path)
        CC.unchanged(pre, CC.snapshot(gt))
    with pytest.raises(vh.VoxelHashError, match="invalid argument"):
        bare.save_color(str(tmp_path / "bare.vhc"))                               # no volume to save
    assert not os.path.exists(str(tmp_path / "bare.vhc"))
    small = CC.table(vh, DC.KW, numVoxelBlocks=256)
    with pytest.raises(vh.VoxelHashError, match="invalid argument"):
        small.load_color(good)                                                    # another configuration
    assert not small.has_color()
    gt.load_color(good)                                                           # and the good one still loads
    CC.unchanged(pre, CC.snapshot(gt))
    for t in (gt, other, bare, small):
        t.close()
