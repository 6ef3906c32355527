"""The specification of vh_sdf_build_system / vh_sdf_residuals / vh_sdf_align in numpy: point-to-SDF alignment (Bylow et al.,
RSS 2013) on top of tests/sample_ref.py, over a model dictionary as tests/mesh_models.py defines it.  It does not import the
product.

Rule (include/voxelhash.h, "tracking against the model itself"), float32 with every multiply and add rounded on its own:
  point   p = input[idx] (camera frame, float4); p.z == 0: no point.  q_r = ((T[r][0]*p.x + T[r][1]*p.y) + T[r][2]*p.z) + T[r][3]
          with T the float32 copy of the camera -> world pose.
  sample  (s, g) = the trilinear sdf and gradient of sample_ref.sample at q.
  kept    a point, a sample, |s| < dist_thres, g finite on every axis.
  system  J = [g, q x g], residual s: the float32 products J_a * J_b, J_a * s, summed here in float64 (the library adds them
          in float32 in a fixed order); error = sum s; count.
  step    T <- exp(-(JTJ^-1 JTr)) T in double, twist (v, w); stop when the summed residual is exactly 0 or JTJ is not positive
          definite.
  maps    points = q ((0, 0, 0) without a point), sdf = s where kept else NaN, gradient = g where kept else (0, 0, 0)."""
import numpy as np

import sample_ref as sr

F = np.float32


class Field(sr.Field):
    """sample_ref.Field with the block look-up as a dense array over the bounding box of the keys instead of a dictionary
    walk per distinct key: the same answers, fast enough for ten rounds on a whole image."""

    def __init__(self, model):
        super().__init__(model)
        keys = np.array(list(self.row), np.int64).reshape(-1, 3)
        self.lo = keys.min(0) if len(keys) else np.zeros(3, np.int64)
        self.dims = (keys.max(0) - self.lo + 1) if len(keys) else np.ones(3, np.int64)
        assert self.dims.prod() < 1 << 26, "a dense look-up is meant for one scene"
        self.rows = np.full(tuple(self.dims), len(self.row), np.int64)          # len(row): the absent block
        if len(keys):
            self.rows[tuple((keys - self.lo).T)] = np.fromiter(self.row.values(), np.int64, len(keys))

    def voxels(self, g):
        g = np.asarray(g, np.int64)
        flat = g.reshape(-1, 3)
        k = (flat >> 3) - self.lo
        inside = ((k >= 0) & (k < self.dims)).all(1)
        row = np.full(len(flat), len(self.row), np.int64)
        row[inside] = self.rows[tuple(k[inside].T)]
        index = ((flat[:, 2] & 7) << 6) | ((flat[:, 1] & 7) << 3) | (flat[:, 0] & 7)
        return self.sdf[row, index].reshape(g.shape[:-1]), self.weight[row, index].reshape(g.shape[:-1])


def move(points4, pose):
    """(q [n, 3] float32, have [n]): the input points moved by the float32 copy of `pose`; rows without a point are 0."""
    p = np.ascontiguousarray(points4, F).reshape(-1, 4)
    T = np.asarray(pose, np.float64).reshape(4, 4).astype(F)
    have = p[:, 2] != 0
    q = np.zeros((len(p), 3), F)
    x, y, z = p[have, 0], p[have, 1], p[have, 2]
    with np.errstate(all="ignore"):
        for r in range(3):
            q[have, r] = (((T[r, 0] * x).astype(F) + (T[r, 1] * y).astype(F)).astype(F) + (T[r, 2] * z).astype(F)).astype(F) + T[r, 3]
    return q, have


def pixels(model, points4, pose, voxel_size, dist_thres):
    """Per pixel: q [n, 3], s [n], g [n, 3] (the sample wherever there is a point: NaN without a sample), kept [n], and
    sampled [n]: the pixel has a point and the point a sample."""
    field = model if isinstance(model, sr.Field) else Field(model)
    q, have = move(points4, pose)
    n = len(q)
    s, w, g = np.full(n, np.nan, F), np.zeros(n, F), np.full((n, 3), np.nan, F)
    s[have], w[have], g[have] = sr.sample(field, q[have], voxel_size, sr.TRILINEAR)
    with np.errstate(invalid="ignore"):
        kept = have & (np.abs(s) < F(dist_thres)) & np.isfinite(g).all(1)
        sampled = have & (w > 0)                 # (no sample: weight exactly 0; the crafted models' valid weights are > 0)
    return q, s, g, kept, sampled


def maps(q, s, g, kept):
    """What vh_sdf_residuals writes: (points, sdf, gradient)."""
    return q, np.where(kept, s, F(np.nan)).astype(F), np.where(kept[:, None], g, F(0)).astype(F)


def system(q, s, g, kept):
    """(JTJ [6, 6], JTr [6], error, count): float64 sums of the float32 products."""
    q, s, g = q[kept], s[kept], g[kept]
    m = lambda a, b: (a * b).astype(F)
    J = np.stack([g[:, 0], g[:, 1], g[:, 2],
                  (m(q[:, 1], g[:, 2]) - m(q[:, 2], g[:, 1])).astype(F),
                  (m(q[:, 2], g[:, 0]) - m(q[:, 0], g[:, 2])).astype(F),
                  (m(q[:, 0], g[:, 1]) - m(q[:, 1], g[:, 0])).astype(F)], 1)
    JTJ = np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            JTJ[a, b] = JTJ[b, a] = m(J[:, a], J[:, b]).astype(np.float64).sum()
    JTr = np.array([m(J[:, a], s).astype(np.float64).sum() for a in range(6)])
    return JTJ, JTr, float(s.astype(np.float64).sum()), int(kept.sum())


def build_system(model, points4, pose, voxel_size, dist_thres):
    q, s, g, kept, _ = pixels(model, points4, pose, voxel_size, dist_thres)
    return system(q, s, g, kept)


def se3_exp(twist):
    """exp of the twist (v, w): R = I + A K + B K^2, t = (I + B K + C K^2) v, K = [w]x."""
    v, w = np.asarray(twist[:3], np.float64), np.asarray(twist[3:], np.float64)
    th2 = float(w @ w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th2 < 1e-8:
        A, B, Cc = 1 - th2 / 6, 0.5 - th2 / 24, 1 / 6 - th2 / 120
    else:
        th = np.sqrt(th2)
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ v
    return T


def align(model, points4, start_pose, voxel_size, dist_thres, max_iters):
    """-> (pose [4, 4] float64, last system, rounds that took a step)."""
    field = model if isinstance(model, sr.Field) else Field(model)
    T = np.asarray(start_pose, np.float64).reshape(4, 4).copy()
    last, steps = None, 0
    for _ in range(max_iters):
        last = build_system(field, points4, T, voxel_size, dist_thres)
        JTJ, JTr, err, _ = last
        if err == 0:
            break
        try:
            np.linalg.cholesky(JTJ)
        except np.linalg.LinAlgError:
            break
        T = se3_exp(-np.linalg.solve(JTJ, JTr)) @ T
        steps += 1
    return T, last, steps
