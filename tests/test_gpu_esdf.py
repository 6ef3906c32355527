"""vh_esdf_lattice on the GPU against the specification (tests/esdf_ref.py, a brute-force minimum by definition, pinned by
tests/test_esdf_ref_cpu.py): the int32 squared distances and the float metres, both bit for bit, on models the tests choose
themselves (tests/mesh_models.py) and on tables the frame path filled.  Every case asserts, on the reference's own answer, a
condition without which it could pass vacuously."""
import ctypes as C
import itertools

import numpy as np
import pytest

import esdf_ref as er
import mesh_models as mm
import sample_ref as sr
from test_gpu_gc import frames
from test_gpu_mesh import fuse, shard_pair, table_of
from test_gpu_sample import SMALL, context_with

pytestmark = pytest.mark.gpu
F = np.float32
MODES = (er.KEEP, er.FREE, er.OCCUPIED)


def computed(gt, lo, dims, radius, unknown=er.KEEP):
    f, d = gt.esdf_lattice(lo, dims, radius, unknown, distance=True, dist2=True)
    return d.cpu().numpy(), f.cpu().numpy()


def same_as_reference(gt, field, lo, dims, radius, unknown=er.KEEP):
    """Both outputs against the specification on `field`; returns the specification's D."""
    d, f = computed(gt, lo, dims, radius, unknown)
    want = er.esdf(field, lo, dims, radius, unknown)
    assert d.dtype == np.int32 and d.shape == want.shape
    assert np.array_equal(d, want), f"dist2 differs in {np.count_nonzero(d != want)} of {d.size} voxels (lo {lo} dims {dims} R {radius} unknown {unknown})"
    assert er.same_bits(f, er.distance(want, gt.params.voxelSize)), (lo, dims, radius, unknown)
    return want


def kinds(want):
    """How many voxels are NONE, +FAR, -FAR, positive, negative."""
    finite = (want != er.NONE) & (np.abs(want.astype(np.int64)) < er.FAR)
    return [int((want == er.NONE).sum()), int((want == er.FAR).sum()), int((want == -er.FAR).sum()),
            int((finite & (want > 0)).sum()), int((finite & (want < 0)).sum())]


# ---- 1. crafted models -----------------------------------------------------------------------------------------------
CRAFTED = {                          # model -> a box across its block seams and out of it, unaligned
    "lone_block": ((37, -27, 13), (14, 13, 12)),
    "many_blocks": ((94, -3, -6), (21, 10, 9)),          # the sphere of radius 97.4 around (3.3, 2.1, -1.7) passes through it
    "holes": ((-27, 19, -12), (22, 20, 12)),
    "zeros": ((-10, -9, -5), (20, 19, 11)),
    "non_finite": ((-10, -9, -5), (20, 19, 11)),
    "weights": ((-10, -9, -5), (20, 19, 11)),
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_models(vh, torch_cuda, tmp_path, name):
    model = mm.holes(0) if name == "holes" else getattr(mm, name)()
    kw = dict(numBuckets=mm.MANY_BUCKETS, bucketSize=mm.MANY_BUCKET_SIZE, numVoxelBlocks=len(model) + 11) if name == "many_blocks" else SMALL
    gt = context_with(vh, model, tmp_path, **kw)
    field = sr.Field(model)
    lo, dims = CRAFTED[name]
    for unknown in MODES:
        want = same_as_reference(gt, field, lo, dims, 3, unknown)
        k = kinds(want)
        print(f"{name} unknown={unknown}: none={k[0]} far={k[1]} -far={k[2]} positive={k[3]} negative={k[4]}")
        assert (want != 0).all() and k[3] > 20 and k[4] > 20
        assert (k[0] > 20) if unknown == er.KEEP and name != "many_blocks" else (k[0] == 0 or unknown == er.KEEP)
    if name == "zeros":                                              # a stored +-0 is outside: its value is positive
        s, _ = field.voxels(er.grid(lo, dims))
        zero = s == 0
        assert zero.sum() > 50 and (er.esdf(field, lo, dims, 3)[zero] > 0).all()
    if name == "non_finite":                                         # -inf is inside, a NaN sdf with weight 1 is unknown
        raw = {k: v[0] for k, v in model.items()}
        g = er.grid(lo, dims)
        want = er.esdf(field, lo, dims, 3)
        hits = [0, 0]
        for p, d in zip(g.reshape(-1, 3), want.reshape(-1)):
            key = tuple(int(c) >> 3 for c in p)
            if key in raw:
                v = raw[key][((int(p[2]) & 7) << 6) | ((int(p[1]) & 7) << 3) | (int(p[0]) & 7)]
                if np.isneginf(v) and model[key][1][((int(p[2]) & 7) << 6) | ((int(p[1]) & 7) << 3) | (int(p[0]) & 7)] > 0:
                    hits[0] += 1
                    assert d < 0
                if np.isnan(v):
                    hits[1] += 1
                    assert d == er.NONE
        assert min(hits) > 3, hits
    gt.close()


# ---- 2. the exact cap ------------------------------------------------------------------------------------------------
def test_exact_cap(vh, torch_cuda, tmp_path):
    sdf = np.full(512, 1.0, F)
    sdf[0] = -1.0                                                    # one inside voxel, (0, 0, 0), in a block of outside voxels
    model = {(0, 0, 0): (sdf, np.ones(512, F))}
    gt = context_with(vh, model, tmp_path)
    lo, dims = (-2, -1, -3), (11, 10, 12)
    at = lambda d, x, y, z: int(d[z - lo[2], y - lo[1], x - lo[0]])
    d5 = same_as_reference(gt, model, lo, dims, 5)
    assert [at(d5, *p) for p in ((5, 0, 0), (3, 4, 0), (0, 3, 4))] == [25, 25, 25]
    assert [at(d5, *p) for p in ((4, 4, 0), (6, 0, 0))] == [er.FAR, er.FAR]
    assert at(d5, 0, 0, 0) == -1 and at(d5, -1, 0, 0) == er.NONE
    d7 = same_as_reference(gt, model, lo, dims, 7)
    assert at(d7, 2, 3, 6) == 49 and at(d7, 7, 1, 0) == er.FAR and at(d7, 6, 0, 0) == 36
    gt.close()


# ---- 3. boxes --------------------------------------------------------------------------------------------------------
def test_boxes(vh, torch_cuda, tmp_path):
    model = mm.holes(0)                                              # around key (-2, 3, -1): voxels x -24..-1, y 16..39, z -16..7
    corner = [o for o in itertools.product((-1, 0), (0, 1), (0, 1)) if o in mm.holes_present(0)]
    assert 0 < len(corner) < 8                                       # of the 2x2x2 blocks around voxel (-16, 32, 0) some are absent
    gt = context_with(vh, model, tmp_path)
    field = sr.Field(model)
    boxes = [((-10, 27, -3), (1, 1, 1), 4), ((-13, 25, -12), (1, 1, 19), 4), ((-12, 25, -3), (19, 1, 1), 4),
             ((-19, 21, -9), (13, 9, 20), 3), ((-3, 5, -9), (13, 9, 20), 6), ((-11, 26, -4), (2, 3, 1), 6),
             ((-20, 27, -5), (9, 9, 9), 5), ((-31, 9, -23), (17, 11, 10), 9)]
    mixed = 0
    for lo, dims, radius in boxes:
        for unknown in MODES:
            want = same_as_reference(gt, field, lo, dims, radius, unknown)
            mixed += len(set(np.sign(want.astype(np.int64)).reshape(-1).tolist())) > 1
    assert mixed >= 9
    # wholly in unallocated space, further than R from every block
    for lo, dims in (((100, 100, 100), (5, 4, 3)), ((-300, 7, 9), (1, 1, 1))):
        d, f = computed(gt, lo, dims, 7, er.KEEP)
        assert (d == er.NONE).all() and np.isnan(f).all()
        d, f = computed(gt, lo, dims, 7, er.FREE)
        assert (d == er.FAR).all() and np.isposinf(f).all()
        d, f = computed(gt, lo, dims, 7, er.OCCUPIED)
        assert (d == -er.FAR).all() and np.isneginf(f).all()
    gt.close()


# ---- 3b. boxes larger than one tile of every pass ----------------------------------------------------------------------
SEAM_LO = (3, 2, 1)
SEAM_BOXES = {                       # dims -> voxels of the other class placed at the tile seams (relative to SEAM_LO), both sides
    (262, 5, 4): ((259, 2, 2), (252, 3, 1)),                   # x pass: two 256-voxel tiles per row, many rows
    (70, 41, 9): ((66, 34, 4), (10, 29, 6), (40, 33, 2)),      # y pass: two inner tiles x two 32-output tiles x 9 + 2R slices
    (20, 9, 40): ((5, 4, 34), (15, 7, 29)),                    # z pass: three inner tiles x two 32-output tiles
    (70, 41, 36): ((60, 35, 33), (20, 30, 30)),                # y and z beyond a tile at once
}


def seam_model(inverted, seed=61):
    """34 x 6 x 5 blocks of one class with some 300 scattered voxels of the other (and 1 % unknown), so that the nearest site
    is typically six voxels away, plus the voxels of SEAM_BOXES."""
    rng = np.random.RandomState(seed)
    sea = F(-1.0) if inverted else F(1.0)
    model = {k: (np.where(rng.uniform(size=512) < 0.0006, -sea, sea).astype(F), np.where(rng.uniform(size=512) < 0.01, 0, 1).astype(F))
             for k in mm.cube_keys((0, 0, 0), (34, 6, 5))}
    for rel in (r for sites in SEAM_BOXES.values() for r in sites):
        x, y, z = (r + l for r, l in zip(rel, SEAM_LO))
        sdf, w = model[(x >> 3, y >> 3, z >> 3)]
        at = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7)
        sdf[at], w[at] = -sea, 1.0
    return model


@pytest.mark.parametrize("inverted", (False, True))
def test_boxes_beyond_one_tile(vh, torch_cuda, tmp_path, inverted):
    """Boxes with more than 256 voxels in x (the x pass's tile) and more than 32 in y and in z (the other passes' tile of
    outputs: the second tile's runs start inside the column), with more than one tile across the lanes as well.  At R = 4 and
    at R = 10, where a window reaches across a seam.  Sparse sites of the class the field measures: P with a few inside voxels
    in an outside sea, N with the signs inverted."""
    model = seam_model(inverted)
    gt = context_with(vh, model, tmp_path, numBuckets=mm.MANY_BUCKETS, bucketSize=mm.MANY_BUCKET_SIZE, numVoxelBlocks=len(model) + 11)
    field = sr.Field(model)
    for dims in SEAM_BOXES:
        for radius in (4, 10):
            want = same_as_reference(gt, field, SEAM_LO, dims, radius)
            mag = np.abs(want.astype(np.int64))
            sea = (want > 0) if not inverted else (want < 0)
            hit = sea & (mag < er.FAR) & (mag >= (16 if radius == 10 else 4))       # a distance to a site that is not next door
            if dims[0] > 256:
                assert hit[:, :, 256:].any() and hit[:, :, 250:256].any()            # on both sides of x = 256
            if dims[1] > 32:
                assert hit[:, 32:, :].any() and hit[:, 28:32, :].any()               # ... of y = 32
            if dims[2] > 32:
                assert hit[32:, :, :].any() and hit[28:32, :, :].any()               # ... of z = 32
            k = kinds(want)
            print(f"inverted={inverted} dims={dims} R={radius}: none={k[0]} far={k[1]} -far={k[2]} positive={k[3]} negative={k[4]}")
            assert k[0] > 10 and min(k[3], k[4]) >= 2
        if not inverted and dims != (70, 41, 36):
            same_as_reference(gt, field, SEAM_LO, dims, 4, er.FREE)
    gt.close()


# ---- 4. radii at the seams -------------------------------------------------------------------------------------------
RADII = (1, 7, 8, 9, 63, 64, 65, 127, 128, 255)


@pytest.mark.parametrize("radius", RADII)
def test_radii_at_the_seams(vh, torch_cuda, tmp_path, radius):
    """One site of each class and nothing else: under FREE every voxel but A is outside, so P = |g - A|^2 up to the cap; under
    OCCUPIED every voxel but B is inside, so N = |g - B|^2.  The box is put at distance R - 1, R and R + 1 from the site,
    before and behind it on each axis, as a single voxel and as 70 x 3 x 2."""
    A, B = (3, 5, 2), (1604, 6, 1)                                   # 1600 voxels apart: never within R of the same box
    sdf, w = np.full(512, 1.0, F), np.zeros(512, F)
    sa, wa = sdf.copy(), w.copy()
    sa[(A[2] << 6) | (A[1] << 3) | A[0]], wa[(A[2] << 6) | (A[1] << 3) | A[0]] = -1.0, 1.0
    wb = w.copy()
    wb[((B[2] & 7) << 6) | ((B[1] & 7) << 3) | (B[0] & 7)] = 1.0
    model = {(0, 0, 0): (sa, wa), (200, 0, 0): (sdf.copy(), wb)}
    gt = context_with(vh, model, tmp_path)
    field = sr.Field(model)
    reached = 0
    for unknown, site in ((er.FREE, A), (er.OCCUPIED, B)):
        for dims in ((1, 1, 1), (70, 3, 2)):
            for axis, side, gap in itertools.product(range(3), (-1, 1), (radius - 1, radius, radius + 1)):
                # the box's face on `axis` is `gap` voxels from the site; across the other axes the site is inside the box's span
                lo = [site[a] - dims[a] // 2 for a in range(3)]
                lo[axis] = site[axis] + gap if side > 0 else site[axis] - gap - dims[axis] + 1
                want = same_as_reference(gt, field, tuple(lo), dims, radius, unknown)
                sign = 1 if unknown == er.FREE else -1
                best = sign * want.astype(np.int64)
                if gap == 0:
                    assert (best.reshape(-1) == -1).sum() == 1       # the site itself, one voxel from the other class
                elif gap <= radius:
                    assert best.min() == gap * gap
                    reached += 1
                else:
                    assert (best == er.FAR).all()
    assert reached >= 2 * 2 * 6
    gt.close()


# ---- 5. independence from the box ------------------------------------------------------------------------------------
def test_independence_from_the_box(vh, torch_cuda, tmp_path):
    model = {k: (np.full(512, 1.0, F), np.ones(512, F)) for k in mm.cube_keys(-1, 1)}      # outside voxels, x -8 .. 7
    model[(3, 0, 0)] = (np.full(512, -1.0, F), np.ones(512, F))                            # the only inside voxels, x 24 .. 31
    gt = context_with(vh, model, tmp_path)
    field = sr.Field(model)
    R = 20
    la, da, lb, db = (-6, -7, -5), (12, 10, 9), (1, -2, -1), (7, 9, 8)      # x -6 .. 5 and 1 .. 7: the sites lie outside both
    a = same_as_reference(gt, field, la, da, R)
    b = same_as_reference(gt, field, lb, db, R)
    fa, fb = computed(gt, la, da, R)[1], computed(gt, lb, db, R)[1]
    # overlap: x 1 .. 5, y -2 .. 2, z -1 .. 3
    assert np.array_equal(a[4:9, 5:10, 7:12], b[0:5, 0:5, 0:5]) and er.same_bits(fa[4:9, 5:10, 7:12], fb[0:5, 0:5, 0:5])
    big, fbig = computed(gt, (-9, -9, -9), (20, 19, 18), R)
    assert np.array_equal(big[4:13, 2:12, 3:15], a) and er.same_bits(fbig[4:13, 2:12, 3:15], fa)
    assert int(a[5, 7, 11]) == 19 * 19 and (a[5, 7, :9] == er.FAR).all()      # voxel (5, 0, 0) sees (24, 0, 0); x <= 2 is too far
    assert ((b > 0) & (b < er.FAR)).sum() > 50
    gt.close()


# ---- 6. tables -------------------------------------------------------------------------------------------------------
def test_two_shards(vh, torch_cuda):
    shards = shard_pair(vh, torch_cuda)
    models = [mm.model_of(sh.table.hash_table(), sh.table.sdf_blocks()) for sh in shards]
    assert not set(models[0]) & set(models[1])
    # a block of shard 0 with a face neighbour in shard 1
    pairs = [(k, (k[0] + 1, k[1], k[2])) for k in sorted(models[0]) if (k[0] + 1, k[1], k[2]) in models[1]]
    assert pairs
    k0, k1 = pairs[len(pairs) // 2]
    lo, dims = tuple(int(c) * 8 - 3 for c in k0), (22, 14, 13)
    for sh, model, other in zip(shards, models, (k1, k0)):
        field = sr.Field(model)
        want = same_as_reference(sh.table, field, lo, dims, 5)
        in_other = ((er.grid(lo, dims) >> 3) == np.array(other)).all(-1)
        assert in_other.sum() >= 512 - 5 * 64 and (want[in_other] == er.NONE).all()      # the other shard's block is unknown
        assert (want != er.NONE).sum() > 50
        same_as_reference(sh.table, field, lo, dims, 5, er.FREE)
    for sh in shards:
        sh.table.close()


def test_overflow_list_chains(vh, torch_cuda):
    gt = fuse(torch_cuda, table_of(vh, 1, overflow=True, numBuckets=512, bucketSize=2, numVoxelBlocks=4096,
                                   attachedLinkedListSize=8))
    table = gt.hash_table()
    assert (table["offset"] != 0).sum() > 20                         # chains did form
    model = mm.model_of(table, gt.sdf_blocks())
    field = sr.Field(model)
    # blocks whose entry does not sit in the bucket of its key (it was reached through a chain), and a few that do
    used = np.nonzero(table["ptr"] != -1)[0]
    away = used[mm.hash_block(table["pos"][used], 512) != used // 2]
    assert len(away) > 10
    picks = [tuple(int(c) for c in table["pos"][i]) for i in list(away[:: max(1, len(away) // 4)][:4]) + list(used[:: len(used) // 3][:3])]
    total = np.zeros(5, np.int64)
    for key in picks:
        want = same_as_reference(gt, field, tuple(c * 8 - 2 for c in key), (12, 11, 10), 4)
        assert (want != er.NONE).any()                               # the block itself is found
        total += kinds(want)
    print(f"overflow: none={total[0]} far={total[1]} -far={total[2]} positive={total[3]} negative={total[4]} over {len(picks)} boxes")
    assert total[0] > 100 and total[3] + total[1] > 100 and total[4] + total[2] > 100
    gt.close()


def test_view_table(vh, torch_cuda):
    torch = torch_cuda
    model = mm.every_configuration()
    rec = torch.from_numpy(mm.view_records(model)).cuda()
    view = vh.SDFHashtable(vh.default_params(numBuckets=509, bucketSize=8, numVoxelBlocks=1), 640, 480, 1)
    view.import_view(rec, len(model))
    for unknown in MODES:
        want = same_as_reference(view, model, (-2, 5, 3), (20, 7, 9), 3, unknown)
        assert kinds(want)[3] > 100 and kinds(want)[4] > 100
    view.close()


# ---- 7. queueing, purity, guards, optional outputs -------------------------------------------------------------------
def test_sees_queued_frames_and_changes_nothing(vh, torch_cuda):
    torch = torch_cuda
    plain = fuse(torch, table_of(vh, 1))
    model = mm.model_of(plain.hash_table(), plain.sdf_blocks())
    keys = np.array(sorted(model), np.int64)
    lo, dims, R = tuple(int(c) * 8 - 9 for c in keys[len(keys) // 2]), (37, 30, 21), 6
    gt = table_of(vh, 1)
    fr = frames(6)
    keep = [torch.from_numpy(v).cuda() for _, v in fr]
    gt.set_option("pipeline", 1)
    gt.integrate_batch([q for q, _ in fr[:5]], keep[:5])
    gt.integrate(fr[5][0], keep[5])                                  # pipelined: its second half is still pending, no flush
    before = computed(gt, lo, dims, R)
    gt.flush()
    after = computed(gt, lo, dims, R)
    want = er.esdf(model, lo, dims, R)
    assert np.array_equal(before[0], want) and np.array_equal(after[0], want)
    assert er.same_bits(before[1], er.distance(want, gt.params.voxelSize)) and er.same_bits(after[1], before[1])
    k = kinds(want)
    assert k[0] > 100 and k[3] > 100 and k[4] > 100, k
    # purity, guards and each output alone
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    n, guard, need = int(np.prod(dims)), 4096, gt.esdf_workspace_bytes(dims, R)
    assert need > 0 and need % 16 == 0
    work = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    d2 = torch.full((n + 2 * guard,), -77, dtype=torch.int32, device="cuda")
    dist = torch.full((n + 2 * guard,), -7.5, dtype=torch.float32, device="cuda")
    for use_d2, use_dist in ((True, True), (True, False), (False, True)):
        d2.fill_(-77)
        dist.fill_(-7.5)
        gt.esdf_lattice_into(lo, dims, R, d2[guard:guard + n] if use_d2 else None, dist[guard:guard + n] if use_dist else None,
                             workspace=work[:need])
        h2, hd = d2.cpu().numpy(), dist.cpu().numpy()
        assert (work[need:].cpu().numpy() == 0x5A).all()
        assert (h2[:guard] == -77).all() and (h2[guard + n:] == -77).all() and (hd[:guard] == -7.5).all() and (hd[guard + n:] == -7.5).all()
        if use_d2:
            assert np.array_equal(h2[guard:guard + n], want.reshape(-1))
        else:
            assert (h2 == -77).all()
        if use_dist:
            assert er.same_bits(hd[guard:guard + n], er.distance(want, gt.params.voxelSize).reshape(-1))
        else:
            assert (hd == -7.5).all()
    gt.synchronize()
    assert state(gt) == s0
    gt.close()
    plain.close()


def test_launch_option_is_for_timing_only(vh, torch_cuda, tmp_path):
    """Option "esdf_launches" (tools/esdf_time.py): 0 and 4 are the whole call; 1..3 stop early and write no output."""
    torch = torch_cuda
    model = mm.lone_block()
    gt = context_with(vh, model, tmp_path)
    lo, dims, R = (37, -27, 13), (14, 13, 12), 4
    gt.set_option("esdf_launches", 4)
    want = same_as_reference(gt, model, lo, dims, R)
    assert kinds(want)[3] > 20 and kinds(want)[4] > 20
    out = torch.full((int(np.prod(dims)),), -77, dtype=torch.int32, device="cuda")
    for k in (1, 2, 3):
        gt.set_option("esdf_launches", k)
        gt.esdf_lattice_into(lo, dims, R, out)
    assert (out.cpu().numpy() == -77).all()
    # the host form ignores the setting (it would copy memory nobody wrote) and leaves it as it was
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    h2 = np.full(int(np.prod(dims)), -77, np.int32)
    assert vh.load().vh_esdf_lattice_host(gt._h, i3(*lo), i3(*dims), R, er.KEEP, h2.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert np.array_equal(h2, want.reshape(-1))
    gt.esdf_lattice_into(lo, dims, R, out)
    assert (out.cpu().numpy() == -77).all()
    assert vh.load().vh_set_option(gt._h, b"esdf_launches", 5) == 1 and vh.load().vh_set_option(gt._h, b"esdf_launches", -1) == 1
    gt.set_option("esdf_launches", 0)
    same_as_reference(gt, model, lo, dims, R)
    gt.close()


# ---- 8. arguments ----------------------------------------------------------------------------------------------------
def test_argument_errors(vh, torch_cuda, tmp_path):
    torch = torch_cuda
    gt = context_with(vh, mm.lone_block(), tmp_path)
    lib, h = vh.load(), gt._h
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    INVALID = 1
    dims, R = (4, 3, 2), 5
    need = gt.esdf_workspace_bytes(dims, R)
    work = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), -77, dtype=torch.int32, device="cuda")
    outf = torch.full((64,), -7.5, dtype=torch.float32, device="cuda")
    Wp, O, Of = C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(outf.data_ptr())
    assert work.data_ptr() % 16 == 0
    call = lambda lo=(40, -24, 16), d=dims, r=R, u=0, w=Wp, nb=need, a=O, b=Of, ctx=h: \
        lib.vh_esdf_lattice(ctx, i3(*lo) if lo else None, i3(*d) if d else None, r, u, w, nb, a, b)
    state = lambda t: (t.hash_table().tobytes(), t.sdf_blocks().tobytes(), t.heap().tobytes(), t.counters())
    s0 = state(gt)
    for r in (0, -1, 256, 1 << 20):
        assert call(r=r) == INVALID
    for u in (-1, 3, 7):
        assert call(u=u) == INVALID
    assert call(d=(-1, 3, 2)) == INVALID and call(d=(4, 3, -2)) == INVALID
    assert call(lo=(-2**31 + 4, 0, 0)) == INVALID                    # lo - R below int32
    assert call(lo=(0, 2**31 - 1 - 3 - 4, 0)) == INVALID             # lo + dims + R = 2^31 + 1 - ... beyond int32's last
    assert call(lo=(0, 0, 2**31 - 1 - 2 - 5)) == 0                   # lo + dims + R = int32's last exactly
    assert call(lo=(-2**31 + 5, 0, 0)) == 0                          # lo - R = int32's first exactly
    assert call(a=None, b=None) == INVALID
    assert call(w=None) == INVALID
    assert call(w=C.c_void_p(work.data_ptr() + 8), nb=need + 8) == INVALID
    assert call(nb=need - 1) == INVALID
    assert call(d=(1 << 11, 1 << 10, 1 << 10), nb=1 << 62) == INVALID                     # 2^31 voxels
    assert call(ctx=None) == INVALID and call(lo=None) == INVALID and call(d=None) == INVALID
    n = C.c_uint64(99)
    assert lib.vh_esdf_workspace_bytes(i3(4, 3, 2), 0, C.byref(n)) == INVALID and lib.vh_esdf_workspace_bytes(i3(4, -3, 2), 5, C.byref(n)) == INVALID
    assert lib.vh_esdf_workspace_bytes(i3(4, 3, 2), 5, None) == INVALID and n.value == 99
    gt.synchronize()
    # nothing but the two good calls at the ends of int32 has written: 24 voxels of unallocated space, NONE and NaN
    h_out, h_f = out.cpu().numpy(), outf.cpu().numpy()
    assert (h_out[:24] == er.NONE).all() and (h_out[24:] == -77).all() and np.isnan(h_f[:24]).all() and (h_f[24:] == -7.5).all()
    assert (work[need:].cpu().numpy() == 0x5A).all()
    # a zero dimension: VH_OK, nothing launched, no workspace needed
    out.fill_(-77)
    outf.fill_(-7.5)
    for d in ((0, 3, 2), (4, 0, 2), (4, 3, 0)):
        assert call(d=d, w=None, nb=0) == 0 and gt.esdf_workspace_bytes(d, R) == 0
    assert gt.esdf_lattice((0, 0, 0), (3, 0, 2), 4).shape == (2, 0, 3)
    gt.synchronize()
    assert (out.cpu().numpy() == -77).all() and (outf.cpu().numpy() == -7.5).all()
    assert state(gt) == s0
    # and the good call is good
    assert call() == 0
    gt.synchronize()
    assert np.array_equal(out.cpu().numpy()[:24], er.esdf(mm.lone_block(), (40, -24, 16), dims, R).reshape(-1))
    gt.close()
