"""Inputs shared by tests/test_merge_color_ref_cpu.py, tests/test_gpu_merge_color.py and tests/test_gpu_color_lifecycle.py: the
frames, pools and transforms of tests/merge_cases.py with a colour image per frame that differs per frame and per pixel, the
colour schedule of the two models, and the cases (transform, voxel-size ratio, mode, weight_max) the GPU tests merge.

src is fused from frames 0 and 1 and coloured twice per frame (two different images), so that its counts reach 4 and a
weight_max of 3 binds (the rest of the range, counts up to 255 on either side, is tests/color_count_cases.py's: crafted words); dst
is fused from frame 2 and coloured once.  Colour lives within 1.5 voxels of the surface, so two
coloured voxels meet only where the moved src surface lies on dst's: under merge_cases.OBLIQUE (27 degrees) the rule finds no
such voxel under REFERENCE semantics, under CLOSE -- the same axis, 3 degrees, a translation off the lattice -- some hundreds in
both (tests/test_merge_color_ref_cpu.py checks every branch for every case)."""
import numpy as np

import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as D
import merge_cases as MC

F = np.float32
U = np.uint32
W, H = MC.W, MC.H
VS = MC.VS
BAND = 1.5 * VS
NEAREST, TRILINEAR = 0, 1

# frame -> the seeds of the colour images fused with it
SRC_COLORS = {0: (0, 3), 1: (1, 4)}
DST_COLORS = {2: (2,)}

CLOSE = MC.rigid((0.3, 1.0, -0.45), 3.0, (0.013, -0.021, 0.017))          # oblique: no axis kept, a translation off the lattice
TRANSFORMS = dict(MC.TRANSFORMS, close=CLOSE)

# (id, transform, vs_d / vs_s, mode, weight_max): the merges into the fused, coloured dst
CASES = [("close-trilinear", "close", 1.0, TRILINEAR, 255),
         ("close-trilinear-cap3", "close", 1.0, TRILINEAR, 3),
         ("close-nearest-cap3", "close", 1.0, NEAREST, 3)]
# (both semantics for the first, PINHOLE for the cap cases)
SEM_CASES = [(sem,) + c for c in CASES for sem in ((0, 1) if c[4] == 255 else (1,))]


def image(seed):
    """A colour image: every pixel and every seed different; byte 3 is noise the library must ignore."""
    return np.random.default_rng(100 + seed).integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(U)


def model_of(table, vox, color):
    """{key: (sdf[512], weight[512], colour[512])} of a downloaded table, SDF volume and colour volume."""
    out = {}
    for e in table[table["ptr"] != -1]:
        p = int(e["ptr"])
        out[tuple(int(c) for c in e["pos"])] = (vox["sdf"][p:p + 512].copy(), vox["weight"][p:p + 512].copy(), color[p:p + 512].copy())
    return out


def with_new_blocks(model, keys):
    """The coloured model with a zeroed block for every key it lacks: what the allocation leaves for the update."""
    out = dict(model)
    for k in keys:
        if k not in out:
            out[k] = (np.zeros(512, F), np.zeros(512, F), np.zeros(512, U))
    return out


def oracle_model(oracle, sem, colors, **kw):
    """The coloured model of the schedule `colors` without a GPU: the oracle's TSDF, tests/color_ref.py's colour."""
    ot = DC.oracle_table(oracle, sem, **kw)
    frames = DC.frames(oracle)
    proj = DC.projection(sem)
    color = np.zeros(ot.params.numVoxelBlocks * 512, U)
    for i in sorted(colors):
        ot.integrate(frames[i][0], frames[i][2])
    tab, vox = ot.hash_table().copy(), ot.sdf_blocks().copy()
    for i in sorted(colors):
        pose, d16, _ = frames[i]
        inv = oracle.invert4x4(pose)
        entries = tab[D.visible_entries(tab, ot.params, sem, proj, pose, inv, W, H)]
        for seed in colors[i]:
            color, _ = CR.integrate(color, vox, entries, ot.params, sem, proj, inv, (d16, DC.k_inv()), image(seed), BAND, 255)
    model = model_of(tab, vox, color)
    ot.close()
    return model


# ---- the GPU side (vh and torch come from the tests' fixtures) -------------------------------------------------------------------
def table(vh, kw, sem=1, bucket_range=None, **over):
    p = dict(kw)
    p.update(over)
    gt = vh.SDFHashtable(vh.default_params(**p), W, H, sem, bucket_range=bucket_range)
    gt.set_projection(DC.projection(sem, W, H))
    return gt


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(torch, gt, oracle, colors, depth=True):
    """All the schedule's depth frames, then its colour images (the order oracle_model uses)."""
    frames = DC.frames(oracle)
    for i in sorted(colors):
        if depth:
            gt.integrate_depth(frames[i][0], dev(torch, frames[i][1]), DC.k_inv())
    for i in sorted(colors):
        for seed in colors[i]:
            gt.integrate_color(frames[i][0], dev(torch, frames[i][1]), DC.k_inv(), dev(torch, image(seed)), BAND, 255)


def snapshot(gt):
    gt.synchronize()
    words = gt.params.numVoxelBlocks * 512
    return dict(table=gt.hash_table(), heap=gt.heap(), vox=gt.sdf_blocks(), compact=gt.compact(), counters=gt.counters(),
                has_color=gt.has_color(), color=gt.color_volume() if gt.has_color() else np.zeros(words, U))


def unchanged(a, b):
    assert np.array_equal(a["table"], b["table"]) and np.array_equal(a["heap"], b["heap"])
    assert np.array_equal(a["vox"].view(U), b["vox"].view(U)) and np.array_equal(a["color"], b["color"])
    assert a["counters"] == b["counters"] and a["has_color"] == b["has_color"]


def model(snap):
    return model_of(snap["table"], snap["vox"], snap["color"])
