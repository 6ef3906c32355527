"""The specification of vh_sdf_color_build_system / vh_sdf_color_residuals / vh_sdf_color_align in numpy: tests/sdf_track_ref.py
with a photometric row beside the geometric one, over a model dictionary {block key: (sdf[512], weight[512], colour[512])} as
tests/color_ref.py defines it (a dictionary of (sdf, weight) pairs is a model without a colour volume).  It does not import the
product.

Rule (include/voxelhash.h, "tracking against the model's colour and shape"), float32 with every multiply, add and divide rounded
on its own:
  point, sample, geometric kept and row: sdf_track_ref's q, (s, g), kept, J = [g, q x g] with residual s.
  luminance  Y(w) = (float)(77 r + 150 g + 29 b) / 65280 of a word r | g << 8 | b << 16 | ...
  input      I = Y(rgba[idx]).
  model      at q there is an intensity iff color_ref.sample's TRILINEAR rule has a colour: eight valid corners, all eight words
             with count > 0.  C = sample_ref's lerp nest over the eight Y, gC = its corner-difference gradient over them / voxelSize.
  photometric row  e = C - I; kept iff geometrically kept, an intensity, |e| < color_thres and color_weight != 0;
             h = color_weight * gC, J = [h, q x h], residual color_weight * e.
  system     sdf_track_ref.system over all rows (float64 sums of the float32 products); count = rows; error = sum of residuals.
  step       sdf_track_ref.align's.
  maps       sdf_track_ref.maps', then e where the pixel has a photometric row else NaN, gC where it has one else (0, 0, 0)."""
import numpy as np

import color_ref as CR
import sample_ref as S
import sdf_track_ref as ref

F, U = np.float32, np.uint32


def luminance(word):
    r, g, b = CR.channels(word)
    return ((U(77) * r + U(150) * g + U(29) * b).astype(F) / F(65280.0)).astype(F)


class Model:
    """The two look-ups of one model: the dense distance field of sdf_track_ref and the colour words of color_ref (None
    without a colour volume)."""

    def __init__(self, model):
        values = list(model.values())
        coloured = bool(values) and len(values[0]) == 3
        self.field = ref.Field({k: (v[0], v[1]) for k, v in model.items()})
        self.color = CR.ColorField(model) if coloured else None


def as_model(model):
    return model if isinstance(model, Model) else Model(model)


def pixels(model, points4, rgba, pose, voxel_size, dist_thres, color_weight, color_thres):
    """Per pixel: sdf_track_ref.pixels' q, s, g, kept, then e [n] and gC [n, 3] (the photometric residual and luminance gradient
    wherever the pixel is geometrically kept and q has a model intensity: NaN elsewhere) and photo [n]: the pixel has a
    photometric row."""
    m = as_model(model)
    q, s, g, kept, _ = ref.pixels(m.field, points4, pose, voxel_size, dist_thres)
    n = len(q)
    e, gC, photo = np.full(n, np.nan, F), np.full((n, 3), np.nan, F), np.zeros(n, bool)
    if m.color is None or F(color_weight) == 0 or not kept.any():
        return q, s, g, kept, e, gC, photo
    vs = F(voxel_size)
    at = np.flatnonzero(kept)
    u = (q[at] / vs).astype(F)                                           # (kept: a sample, so |u| < 2^30)
    f = np.floor(u).astype(F)
    i = f.astype(np.int64)
    t = (u - f).astype(F)
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    words = [m.color.words(i + np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64)) for c in range(8)]
    has = np.all([CR.count(w) > 0 for w in words], axis=0)
    y = [luminance(w) for w in words]
    L = S.lerp
    C = L(L(L(y[0], y[1], tx), L(y[2], y[3], tx), ty), L(L(y[4], y[5], tx), L(y[6], y[7], tx), ty), tz)
    d = lambda a, b: (y[a] - y[b]).astype(F)
    grad = np.stack([(L(L(d(1, 0), d(3, 2), ty), L(d(5, 4), d(7, 6), ty), tz) / vs).astype(F),
                     (L(L(d(2, 0), d(3, 1), tx), L(d(6, 4), d(7, 5), tx), tz) / vs).astype(F),
                     (L(L(d(4, 0), d(5, 1), tx), L(d(6, 2), d(7, 3), tx), ty) / vs).astype(F)], 1)
    I = luminance(np.ascontiguousarray(rgba, U).reshape(-1)[at])
    res = (C - I).astype(F)
    e[at[has]], gC[at[has]] = res[has], grad[has]
    photo[at[has]] = np.abs(res[has]) < F(color_thres)
    return q, s, g, kept, e, gC, photo


def maps(q, s, g, kept, e, gC, photo):
    """What vh_sdf_color_residuals writes: (points, sdf, gradient, color_residual, color_gradient)."""
    return ref.maps(q, s, g, kept) + (np.where(photo, e, F(np.nan)).astype(F), np.where(photo[:, None], gC, F(0)).astype(F))


def system(q, s, g, kept, e, gC, photo, color_weight):
    """(JTJ [6, 6], JTr [6], error, count) over the geometric and the photometric rows."""
    cw = F(color_weight)
    h = (cw * gC[photo]).astype(F)
    r = (cw * e[photo]).astype(F)
    rows_q = np.concatenate([q[kept], q[photo]])
    rows_g = np.concatenate([g[kept], h])
    rows_r = np.concatenate([s[kept], r])
    return ref.system(rows_q, rows_r, rows_g, np.ones(len(rows_q), bool))


def build_system(model, points4, rgba, pose, voxel_size, dist_thres, color_weight, color_thres):
    px = pixels(model, points4, rgba, pose, voxel_size, dist_thres, color_weight, color_thres)
    return system(*px, color_weight)


def align(model, points4, rgba, start_pose, voxel_size, dist_thres, color_weight, color_thres, max_iters):
    """-> (pose [4, 4] float64, last system, rounds that took a step): sdf_track_ref.align over the joint system."""
    m = as_model(model)
    T = np.asarray(start_pose, np.float64).reshape(4, 4).copy()
    last, steps = None, 0
    for _ in range(max_iters):
        last = build_system(m, points4, rgba, T, voxel_size, dist_thres, color_weight, color_thres)
        JTJ, JTr, err, _ = last
        if err == 0:
            break
        try:
            np.linalg.cholesky(JTJ)
        except np.linalg.LinAlgError:
            break
        T = ref.se3_exp(-np.linalg.solve(JTJ, JTr)) @ T
        steps += 1
    return T, last, steps
