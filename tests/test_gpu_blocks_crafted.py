"""vh_render_blocks on the GPU against the rule (tests/blocks_ref.py: every block against every pixel, no culling), both images
bit for bit, on the crafted cases of tests/blocks_cases.py -- whose conditions tests/test_blocks_ref_cpu.py asserts on the rule
alone -- and on tables of every kind the list kernel reads: an overflow list with holes, shards whose bitmap ends in a partial
word, a table after each model-changing call, a pending pipelined frame, a view context that regrows its record list.  The
outputs are slices of larger buffers whose canary words on both sides must stay as they were."""
import ctypes as C

import numpy as np
import pytest

import blocks_cases as bc
import blocks_ref as br
import mesh_models as mm
from merge_cases import rigid
from voxelhashing_demo_amd import dist as vdist
from voxelhashing_demo_amd import streaming, synth

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
GUARD = 1021                     # canary words on each side of an image (odd: the images start at no rounder address than a float's)
CANARY = 0x5A5A5A5A


class Images:
    """front and back of W x H pixels, each in the middle of a canary-filled buffer."""

    def __init__(self, torch, W, H):
        self.torch, self.n, self.shape = torch, W * H, (H, W)
        self.raw = [torch.full((self.n + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda") for _ in range(2)]
        self.front, self.back = (r.view(torch.float32)[GUARD:GUARD + self.n] for r in self.raw)

    def refill(self):
        for r in self.raw:
            r.fill_(CANARY)

    def host(self):
        """(front, back) as float32 [H, W], after checking the canaries."""
        self.torch.cuda.synchronize()
        out = []
        for r in self.raw:
            h = r.cpu().numpy().view(U)
            assert (h[:GUARD] == CANARY).all() and (h[GUARD + self.n:] == CANARY).all(), "a write outside the image"
            out.append(h[GUARD:GUARD + self.n].view(F).reshape(self.shape).copy())
        return out

    def untouched(self):
        self.torch.cuda.synchronize()
        return all((r.cpu().numpy().view(U) == CANARY).all() for r in self.raw)


def same_as_rule(gt, img, view, want, what):
    img.refill()
    gt.render_blocks(view.pose, img.front, img.back, view.t_min, view.t_max)
    front, back = img.host()
    for name, got, exp in (("front", front, want[0]), ("back", back, want[1])):
        diff = got.view(U) != exp.view(U)
        assert not diff.any(), f"{what}: {name} differs in {int(diff.sum())} of {diff.size} pixels, first at (y, x) = {tuple(np.argwhere(diff)[0])}"


def context_of(vh, case, tmp_path):
    gt = vh.SDFHashtable(vh.default_params(**case.table), case.W, case.H, 1)
    gt.set_raycast_intrinsics(case.fx, case.fy, case.cx, case.cy)
    return mm.load_model(gt, case.model(), tmp_path)


def on_keys(gt, img, keys, views, size, intrinsics, what, need=0):
    """The silhouettes of `gt` in every view against the rule on `keys`; returns the pixels that hold a block, all views together."""
    seen = 0
    for i, v in enumerate(views):
        want = br.render(keys, gt.params.voxelSize, *size, *intrinsics, v.pose, v.t_min, v.t_max)
        same_as_rule(gt, img, v, want, f"{what} view {i}")
        seen += int((want[1] > 0).sum())
    assert seen > need, (what, seen)
    return seen


# ---- 1. the crafted cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in bc.names() if n != "calls"])
def test_crafted_case(vh, torch_cuda, tmp_path, name):
    case = bc.case(name)
    gt = context_of(vh, case, tmp_path)
    img = Images(torch_cuda, case.W, case.H)
    for i, v in enumerate(case.views):
        want = case.expected(i)
        facts = bc.check(case, i, *want)
        print(f"{name} view {i}: blocks={facts['blocks']} kept={facts['kept']} region max={int(facts['regions'].max())}")
        same_as_rule(gt, img, v, want, f"{name} view {i}")
    gt.close()


def test_successive_calls_on_one_context(vh, torch_cuda, tmp_path):
    """2049 blocks, then fewer than 10, then none, then 2049 again: each call appends through one of two counter words and
    zeroes the other for the next."""
    case = bc.case("calls")
    gt = context_of(vh, case, tmp_path)
    img = Images(torch_cuda, case.W, case.H)
    kept = []
    for turn in range(2):                                            # twice: both parities meet every size
        for i, v in enumerate(case.views):
            want = case.expected(i)
            kept.append(bc.check(case, i, *want)["kept"])
            same_as_rule(gt, img, v, want, f"calls turn {turn} view {i}")
        same_as_rule(gt, img, case.views[2], case.expected(2), f"calls turn {turn}, nothing again")     # (an odd number of calls per turn)
    assert kept[:4] == [2049, kept[1], 0, 2049] and 1 <= kept[1] < 10
    gt.close()


# ---- 2. tables the frame path filled -----------------------------------------------------------------------------------
RW, RH = bc.ROOM_SIZE
ROOM = dict(numBuckets=4096, bucketSize=5, numVoxelBlocks=8192)


def room_frames(n, first=0):
    prims = synth.room_primitives()
    poses = synth.camera_loop(60)
    return [(poses[(5 * i) % 60], synth.render_room_verts(poses[(5 * i) % 60], RW, RH, prims).numpy()) for i in range(first, first + n)]


def room_table(vh, overflow=False, band=0.0, **kw):
    gt = vh.SDFHashtable(vh.default_params(**(kw or ROOM)), RW, RH, 1)
    if overflow:
        gt.set_option("overflow_list", 1)
    if band:
        gt.set_alloc_band(band)
    gt.set_raycast_intrinsics(*bc.ROOM_INTRINSICS)
    return gt


def fuse(torch, gt, frames):
    for pose, verts in frames:
        gt.integrate(pose, torch.from_numpy(verts).cuda())
    return gt


def key_set(gt):
    return set(map(tuple, gt.allocated()["pos"].tolist()))


def room_check(gt, img, what, need=200):
    keys = gt.allocated()["pos"]
    return on_keys(gt, img, keys, bc.room_views(keys), bc.ROOM_SIZE, bc.ROOM_INTRINSICS, what, need)


def device_keys(torch, keys):
    k4 = np.zeros((len(keys), 4), np.int32)
    k4[:, :3] = np.asarray(keys, np.int32).reshape(-1, 3)
    return torch.from_numpy(k4).cuda()


def test_overflow_list_with_holes(vh, torch_cuda):
    """Buckets of two slots with chains behind them, a third of the blocks deleted: free slots BEFORE used ones, which the list
    kernel has to step over instead of ending the bucket there."""
    torch = torch_cuda
    gt = fuse(torch, room_table(vh, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096, attachedLinkedListSize=8),
              room_frames(6))
    img = Images(torch, RW, RH)
    table = gt.hash_table()
    assert (table["offset"] != 0).sum() > 20                         # chains did form
    room_check(gt, img, "overflow list, fused")
    used = np.nonzero(table["ptr"] != -1)[0]
    heads = used[(used < 1024) & (used % 2 == 1) & (table["offset"][used] != 0)]
    assert len(heads) > 10
    gone = np.union1d(used[::3], heads[:10])
    before = key_set(gt)
    gt.delete_blocks(device_keys(torch, table["pos"][gone]))
    table = gt.hash_table()
    assert len(key_set(gt)) == len(before) - len(gone)
    assert (table["offset"] != 0).sum() > 20                         # chains still exist
    slots = table["ptr"][:1024].reshape(512, 2)
    holes = int(((slots[:, 0] == -1) & (slots[:, 1] != -1)).sum())
    print(f"overflow: {len(before)} blocks, {len(gone)} deleted, {holes} buckets with a free slot before a used one")
    assert holes > 10
    room_check(gt, img, "overflow list, holes")
    gt.close()


def test_three_shards_with_a_partial_bitmap_word(vh, torch_cuda):
    """4093 buckets over three ranks: 1365, 1365 and 1363 buckets, none a multiple of 32.  The keys are the 2049 of the `calls`
    case plus, for every rank, the blocks right behind that wall whose bucket lies in the rank's last, partial, bitmap word
    (the farthest block of their pixels: without them the back image differs).  Each shard takes the keys it owns and must
    equal the rule on them."""
    torch = torch_cuda
    case = bc.case("calls")
    nb = case.table["numBuckets"]
    plan = vdist.ShardPlan(nb, 3)
    behind = case.keys + (0, 0, 1)
    local = mm.hash_block(behind, nb) % plan.per_shard
    keys = np.concatenate([case.keys, behind[local >= plan.per_shard // 32 * 32]])
    bucket = mm.hash_block(keys, nb)
    params = dict(case.table, numVoxelBlocks=len(keys) + 8)
    img = Images(torch, case.W, case.H)
    total, in_last_word = 0, 0
    for rank in range(3):
        lo, hi = plan.bucket_range(rank)
        assert (hi - lo) % 32 != 0
        gt = vh.SDFHashtable(vh.default_params(**params), case.W, case.H, 1, bucket_range=(lo, hi))
        gt.set_raycast_intrinsics(case.fx, case.fy, case.cx, case.cy)
        gt.stream_in({"keys": keys.astype(np.int32), "voxels": np.zeros((len(keys), 512), mm.VOXEL)})
        own = keys[(bucket >= lo) & (bucket < hi)]
        assert key_set(gt) == set(map(tuple, own.tolist())) and len(own) > 500
        last = (bucket[(bucket >= lo) & (bucket < hi)] - lo) >= (hi - lo) // 32 * 32
        in_last_word += int(last.sum())
        assert last.any(), rank                                      # an entry the last, partial, bitmap word names
        on_keys(gt, img, own, case.views[:2], (case.W, case.H), (case.fx, case.fy, case.cx, case.cy), f"shard {rank}", 100)
        total += len(own)
        gt.close()
    print(f"shards: {in_last_word} entries in the last bitmap words")
    assert total == len(keys)


def test_after_every_model_changing_call(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    frames = room_frames(6)
    gt = fuse(torch, room_table(vh, band=0.06), frames[:3])
    src = fuse(torch, room_table(vh), frames[3:])
    img = Images(torch, RW, RH)
    sets = [key_set(gt)]
    path = str(tmp_path / "start.snap")
    gt.save_snapshot(path)

    def step(what):
        sets.append(key_set(gt))
        print(f"{what}: {len(sets[-2])} -> {len(sets[-1])} blocks")
        assert sets[-1] != sets[-2], what                            # the call did change the key set
        room_check(gt, img, what)

    room_check(gt, img, "fused")
    keys = gt.allocated()["pos"]
    gt.delete_blocks(device_keys(torch, keys[::3]))
    step("delete_blocks")
    assert len(sets[-1]) == len(sets[-2]) - len(keys[::3])
    gt.integrate(frames[3][0], torch.from_numpy(frames[3][1]).cuda())          # (a frame: the collector works on its block list)
    step("integrate")
    gt.garbage_collect(0.03)
    step("garbage_collect")
    assert sets[-1] < sets[-2]
    stats = gt.merge(src, rigid((0.0, 1.0, 0.0), 10.0, (0.1, 0.0, 0.05)))
    step("merge")
    assert sets[-1] > sets[-2], stats
    mid = np.median(gt.allocated()["pos"], axis=0).astype(np.int64)
    chunk = gt.stream_out(streaming.box(mid - 3, mid + 4))
    assert len(chunk["keys"]) > 10
    step("stream_out")
    assert sets[-1] == sets[-2] - set(map(tuple, chunk["keys"].tolist()))
    gt.stream_in(chunk)
    step("stream_in")
    assert sets[-1] == sets[-3]
    gt.load_snapshot(path)
    step("load_snapshot")
    assert sets[-1] == sets[0]
    gt.close()
    src.close()


def test_pending_pipelined_frame(vh, torch_cuda):
    """The call sees the queued half of a pipelined frame by itself, and changes nothing of the model."""
    torch = torch_cuda
    frames = room_frames(6)
    gt = room_table(vh)
    keep = [torch.from_numpy(v).cuda() for _, v in frames]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([p for p, _ in frames[:5]], keep[:5])
    gt.integrate(frames[5][0], keep[5])                              # pipelined: its second half is still pending, no flush
    plain = fuse(torch, room_table(vh), frames)
    keys = plain.allocated()["pos"]
    views = bc.room_views(keys)
    img = Images(torch, RW, RH)
    gt.render_blocks(views[0].pose, img.front, img.back, views[0].t_min, views[0].t_max)
    before = img.host()
    gt.flush()
    assert key_set(gt) == key_set(plain)
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    want = br.render(keys, gt.params.voxelSize, RW, RH, *bc.ROOM_INTRINSICS, views[0].pose, views[0].t_min, views[0].t_max)
    same_as_rule(gt, img, views[0], want, "after the flush")
    assert br.same_bits(before[0], want[0]) and br.same_bits(before[1], want[1])
    assert (want[1] > 0).sum() > 200
    gt.synchronize()
    assert state(gt) == s0
    gt.close()
    plain.close()


def test_view_context_that_regrows(vh, torch_cuda):
    """A view context renders before its first import (a record list of one entry), then holds 50, 3000 and 20 records."""
    torch = torch_cuda
    W, H = 64, 48
    intr = (100.0, 100.0, 31.3, 23.6)
    wall = np.array([(x, y, (x + y) % 3) for y in range(-25, 25) for x in range(-30, 30)], np.int64)
    rng = np.random.RandomState(5)
    view = vh.SDFHashtable(vh.default_params(numBuckets=4093, bucketSize=8, numVoxelBlocks=1), W, H, 1)
    view.set_raycast_intrinsics(*intr)
    img = Images(torch, W, H)
    views = [bc.View(bc.pose_of(bc.rot_y(0.2), (-1.5, 0.3, -9.0)), 0.1, 20.0), bc.View(bc.pose_of(bc.rot_x(0.3), (0.4, 1.0, -2.0)), 0.1, 20.0)]
    for v in views:
        same_as_rule(view, img, v, (np.zeros((H, W), F), np.zeros((H, W), F)), "empty view context")
    for n in (50, 3000, 20):
        keys = wall if n == len(wall) else wall[np.sort(rng.permutation(len(wall))[:n])]
        model = {tuple(int(c) for c in k): (np.zeros(512, F), np.zeros(512, F)) for k in keys}
        rec = torch.from_numpy(mm.view_records(model)).cuda()
        view.import_view(rec, n)
        assert key_set(view) == set(model) and len(model) == n
        on_keys(view, img, keys, views, (W, H), intr, f"view context of {n}", 5 if n < 100 else 1000)
    view.close()


# ---- 3. arguments ------------------------------------------------------------------------------------------------------
def test_argument_errors(vh, torch_cuda, tmp_path):
    case = bc.case("negative_keys")
    gt = context_of(vh, case, tmp_path)
    img = Images(torch_cuda, case.W, case.H)
    lib, INVALID = vh.load(), 1
    pose = np.ascontiguousarray(case.views[0].pose.reshape(16))
    P = pose.ctypes.data_as(C.POINTER(C.c_float))
    front, back = C.c_void_p(img.front.data_ptr()), C.c_void_p(img.back.data_ptr())
    call = lambda ctx=gt._h, p=P, lo=0.1, hi=5.0, f=front, b=back: lib.vh_render_blocks(ctx, p, lo, hi, f, b)
    assert call(ctx=None) == INVALID and call(p=None) == INVALID and call(f=None) == INVALID and call(b=None) == INVALID
    assert call(lo=1.0, hi=1.0) == INVALID and call(lo=2.0, hi=1.0) == INVALID            # t_max <= t_min
    assert call(lo=-0.1) == INVALID and call(lo=-1e-30) == INVALID                        # t_min < 0
    nan = float("nan")
    assert call(lo=nan) == INVALID and call(hi=nan) == INVALID and call(lo=nan, hi=nan) == INVALID
    gt.synchronize()
    assert img.untouched()
    assert call() == 0                                               # and the good call is good
    got = img.host()
    want = case.expected(0)
    assert br.same_bits(got[0], want[0]) and br.same_bits(got[1], want[1])
    gt.close()
