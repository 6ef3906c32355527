"""One crafted model through every caller of the trilinear cell and of the nearest lookup: vh_sample_sdf, vh_sample_color,
vh_sdf_residuals, vh_sdf_color_residuals, vh_merge and vh_merge_color, each bit for bit against its rule in numpy
(tests/sample_ref.py, color_ref.py, sdf_track_ref.py, sdf_color_track_ref.py, merge_ref.py, merge_color_ref.py).

The model is 2 x 2 x 2 blocks (voxels 0..15 per axis), every voxel valid with a non-linear sdf and weight and a colour word of
count >= 1, but for two voxels in the far corner block (1, 1, 1): INVALID has weight 0 and EMPTY (a valid voxel) a word of count 0.

The points: one in a cell of each cross mask 0..7 whose eight corners are clean (CLEAN), then one of each mask again in a cell
that has no sample or no colour (DIRTY).  A cell of mask 7 crosses a block face on every axis, and in a model of 2 x 2 x 2 blocks
only the cell (7, 7, 7) does so with all eight blocks present: it is the clean one, so the second cell of mask 7 -- and that of
mask 3, which two special voxels cannot reach beside masks 1, 2, 4, 5 and 6 -- is one whose far blocks are absent.  Between
the points sit lanes without one: NaN, |u| >= 2^30 and (for the two residual calls, which read float4 pixels) z == 0.  Several
of them follow a point of block (0, 0, 0), whose key they share, so they sit in a run that asked for that block.  Two more
points sit on INVALID and on EMPTY themselves, for the nearest lookup.

The merges go into an empty model (vh_merge_color) and an empty twin (vh_merge) half a voxel away: the trilinear one samples
every cell of the model at t = 0.5, the nearest one rounds on exact ties, which the rule and the library must resolve alike."""
import numpy as np
import pytest

import color_ref as CR
import merge_color_cases as CC
import merge_color_ref as M
import merge_ref as R
import sample_ref as sr
import sdf_color_track_ref as cref
import sdf_track_ref as ref
from test_gpu_icp import close_sums
from test_gpu_sample import SMALL
from test_gpu_sdf_color_track import coloured_context, map_buffers, tracker

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
VS = 0.02
W, H = 16, 4
DIST_THRES, COLOR_WEIGHT, COLOR_THRES = 0.08, 0.1, 2.0        # |e| <= 1: a model intensity is a photometric row
INVALID, EMPTY = (8, 9, 8), (9, 8, 8)                         # both in block (1, 1, 1)
# corner 0 of the cells, by cross mask (bit a: i[a] & 7 == 7)
CLEAN = [(2, 3, 4), (7, 2, 3), (3, 7, 12), (7, 7, 2), (12, 3, 7), (7, 12, 7), (3, 7, 7), (7, 7, 7)]
DIRTY = [(8, 8, 8),        # mask 0: INVALID and EMPTY
         (7, 9, 8),        # mask 1: INVALID
         (9, 7, 8),        # mask 2: EMPTY
         (15, 15, 3),      # mask 3: the blocks (2, ., .) and (., 2, .) are absent
         (8, 9, 7),        # mask 4: INVALID
         (7, 8, 7),        # mask 5: INVALID
         (8, 7, 7),        # mask 6: EMPTY
         (7, 7, 15)]       # mask 7: the blocks (., ., 2) are absent
N_POINTS = 57              # what the point calls take: not a multiple of 64


def crafted_model():
    lin = np.arange(512)
    lx, ly, lz = lin & 7, (lin >> 3) & 7, lin >> 6
    rng = np.random.RandomState(5)
    model = {}
    for key in [(x, y, z) for z in range(2) for y in range(2) for x in range(2)]:
        x, y, z = (8 * key[0] + lx).astype(np.float64), (8 * key[1] + ly).astype(np.float64), (8 * key[2] + lz).astype(np.float64)
        sdf = (0.03 * np.sin(0.41 * x + 0.13 * y * y - 0.29 * z) * np.cos(0.23 * z * x - 0.7)).astype(F)
        weight = (1.0 + ((3 * x + 5 * y * y + 7 * z) % 11) * 0.75).astype(F)
        words = ((rng.randint(1, 256, 512).astype(U) << U(24)) | rng.randint(0, 1 << 24, 512).astype(U)).astype(U)
        model[key] = (sdf, weight, words)
    index = lambda g: ((g[2] & 7) << 6) | ((g[1] & 7) << 3) | (g[0] & 7)
    model[(1, 1, 1)][1][index(INVALID)] = 0
    model[(1, 1, 1)][2][index(EMPTY)] &= U(0xFFFFFF)
    return model


def crafted_pixels():
    """The 64 float4 pixels of the 16 x 4 image; the first N_POINTS rows' xyz are the point calls' input."""
    t = np.array([0.3125, 0.59375, 0.71875])
    cell = lambda i: list((np.asarray(i, np.float64) + t) * VS) + [1.0]
    nan, far, zero = [np.nan] * 3 + [1.0], [3.0e7, -3.0e7, 3.0e7, 1.0], [0.1, 0.1, 0.0, 1.0]
    rows, where = [], {}
    for n, gap in enumerate((nan, far, zero, nan, far, zero, nan, far)):
        where[("clean", n)] = len(rows)
        rows += [cell(CLEAN[n]), gap]
        where[("dirty", n)] = len(rows)
        rows += [cell(DIRTY[n]), cell(CLEAN[0]), gap]         # ... a second lane of block (0, 0, 0), then a lane without a point
    t = np.array([0.125, 0.1875, 0.0625])                       # the nearest voxel is corner 0: the two special voxels themselves
    where["invalid"], where["empty"] = len(rows), len(rows) + 2
    rows += [cell(INVALID), nan, cell(EMPTY), nan] + [cell(CLEAN[0]), nan] * 6 + [cell(CLEAN[7])]
    assert len(rows) == N_POINTS and N_POINTS % 64 != 0
    rows += [zero] * (W * H - len(rows))
    return np.array(rows, np.float64).astype(F).reshape(H, W, 4), where


def cells_of(points):
    """(corner 0 [n, 3] int64, cross mask [n]) of the trilinear cells; rows without a finite point read (0, 0, 0)."""
    with np.errstate(invalid="ignore"):
        i = np.nan_to_num(np.floor((np.asarray(points, F) / F(VS)).astype(F)), nan=0.0, posinf=0.0, neginf=0.0)
    i = np.where(np.abs(i) < 2.0 ** 30, i, 0).astype(np.int64)
    return i, ((i & 7) == 7) @ np.array([1, 2, 4])


def test_every_caller_of_the_cell_on_one_crafted_model(oracle, vh, torch_cuda):
    torch = torch_cuda
    model = crafted_model()
    plain = {k: (v[0], v[1]) for k, v in model.items()}
    inp, where = crafted_pixels()
    pts = np.ascontiguousarray(inp.reshape(-1, 4)[:N_POINTS, :3])
    clean, dirty = ([where[(kind, n)] for n in range(8)] for kind in ("clean", "dirty"))

    # ---- on the CPU, before anything runs on the GPU: the cells are the intended ones and the rule sees every kind -----------
    i, mask = cells_of(pts)
    for n in range(8):
        assert tuple(i[clean[n]]) == CLEAN[n] and tuple(i[dirty[n]]) == DIRTY[n]
        assert mask[clean[n]] == n and mask[dirty[n]] == n, n
    tri = sr.sample(plain, pts, VS, sr.TRILINEAR)
    near = sr.sample(plain, pts, VS, sr.NEAREST)
    col_tri, col_near = CR.sample(model, pts, VS, CR.TRILINEAR), CR.sample(model, pts, VS, CR.NEAREST)
    rgba = np.random.default_rng(77).integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(U)
    eye = np.eye(4)
    geo_px = ref.pixels(plain, inp, eye, VS, DIST_THRES)
    px = cref.pixels(model, inp, rgba, eye, VS, DIST_THRES, COLOR_WEIGHT, COLOR_THRES)
    kept, photo = px[3], px[6]
    assert np.isfinite(tri[0][clean]).all() and np.isfinite(tri[2][clean]).all() and (col_tri[clean] != 0).all()
    assert kept[clean].all() and photo[clean].all()                      # all eight masks with a sample and a photometric row
    assert not photo[dirty].any() and not (col_tri[dirty] != 0).any()
    no_sample = np.isnan(tri[0][dirty])
    assert list(no_sample) == [True, True, False, True, True, True, False, True]
    assert np.array_equal(kept[dirty], ~no_sample)                       # EMPTY's cells: a geometric row, no photometric one
    have = inp.reshape(-1, 4)[:, 2] != 0
    with np.errstate(invalid="ignore"):
        lanes_without = ~((np.abs(pts / F(VS)) < sr.DOMAIN).all(1))
    assert lanes_without.sum() >= 16 and np.isnan(tri[0][lanes_without]).all() and (~have).sum() >= 7 + 4
    assert not kept[~have].any() and np.isnan(near[0][lanes_without]).all() and np.isfinite(near[0][clean]).all()
    assert np.isnan(near[0][where["invalid"]]) and col_near[where["invalid"]] == 0
    assert np.isfinite(near[0][where["empty"]]) and col_near[where["empty"]] == 0 and (col_near[clean] != 0).all()

    # ---- the point calls ---------------------------------------------------------------------------------------------------
    gt = coloured_context(vh, model)
    d_pts = torch.from_numpy(pts).cuda()
    for mode, want, want_color in ((sr.NEAREST, near, col_near), (sr.TRILINEAR, tri, col_tri)):
        got = [t.cpu().numpy() for t in gt.sample_sdf(d_pts, mode, weight=True, gradient=True)]
        for name, g, w in zip(("sdf", "weight", "gradient"), got, want):
            assert sr.same_bits(g, w), (name, mode)
        assert np.array_equal(gt.sample_color(d_pts, mode).cpu().numpy(), want_color), mode

    # ---- the two rounds ----------------------------------------------------------------------------------------------------
    d_in, d_rgba = torch.from_numpy(inp).cuda(), torch.from_numpy(rgba).cuda()
    names = ("points", "sdf", "gradient", "color_residual", "color_gradient")
    geo = tracker(gt, W, H, cls="SdfTracking", dist_thres=DIST_THRES)
    _, views, _, _ = map_buffers(torch, W, H)
    got = geo.residuals(d_in, eye, *views[:3])
    for what, v, wm in zip(names, views[:3], ref.maps(*geo_px[:4])):
        assert sr.same_bits(v.cpu().numpy(), wm.reshape(-1)), what
    close_sums(got, ref.system(*geo_px[:4]))
    geo.close()
    joint = tracker(gt, W, H, dist_thres=DIST_THRES, color_weight=COLOR_WEIGHT, color_thres=COLOR_THRES)
    _, views, _, _ = map_buffers(torch, W, H)
    got = joint.residuals(d_in, d_rgba, eye, *views)
    for what, v, wm in zip(names, views, cref.maps(*px)):
        assert sr.same_bits(v.cpu().numpy(), wm.reshape(-1)), what
    want = cref.system(*px, COLOR_WEIGHT)
    assert want[3] == kept.sum() + photo.sum()
    close_sums(got, want)
    joint.close()

    # ---- the merges: into an empty model and an empty twin, half a voxel away ---------------------------------------------------
    T = np.eye(4, dtype=F)
    T[:3, 3] = F(0.5 * VS)
    Tinv = oracle.invert4x4(T)
    src_snap = CC.snapshot(gt)
    for mode in (sr.NEAREST, sr.TRILINEAR):
        dst, twin = (vh.SDFHashtable(vh.default_params(**SMALL), 640, 480, 1) for _ in range(2))
        stats, twin_stats = dst.merge(gt, T, mode, colors=True), twin.merge(gt, T, mode)
        CC.unchanged(src_snap, CC.snapshot(gt))
        got, got_twin = CC.model(CC.snapshot(dst)), CC.model(CC.snapshot(twin))
        assert stats == twin_stats and stats["unplaced"] == 0 and got.keys() == got_twin.keys()
        assert set(got) == R.candidates(model.keys(), T, F(VS), F(VS))[0] and len(got) > 8
        want, gstats, cstats = M.apply(CC.with_new_blocks({}, got.keys()), model, sorted(got), Tinv, F(VS), F(VS),
                                       dst.params.truncation, dst.params.integrationWeightMax, mode, 255)
        print(f"mode {mode}: {stats}; geometry {gstats}; colour {cstats}")
        assert gstats["fresh"] > 3000 and cstats["fresh"] > 3000
        if mode == sr.TRILINEAR:                     # t = 0.5 in every cell of the model: INVALID's eight cells, EMPTY's other cells
            assert gstats["fresh"] == 15 ** 3 - 8 and cstats["no_sample"] >= 4
        for k in want:
            for a, b, c in zip(got[k], got_twin[k][:2] + (None,), want[k]):
                assert np.array_equal(np.asarray(a).view(U), np.asarray(c).view(U)), (mode, k)
                assert b is None or np.array_equal(np.asarray(b).view(U), np.asarray(c).view(U)), (mode, k)
        assert not any(v[2].any() for v in got_twin.values())
        dst.close()
        twin.close()
    gt.close()
