"""The specification of the DDA raycast (vh_raycast, vh_raycast_normals) in vectorised numpy, IEEE float32
throughout (every multiply and add rounded on its own), over a model dictionary as tests/mesh_models.py defines it: {block key
(x, y, z): (sdf[512], weight[512])}, voxel index ((z&7)<<6)|((y&7)<<3)|(x&7).  It does not import the product, knows nothing
of a table, a bitmap or a jump, and walks every ray voxel by voxel to its end: besides the image it states, per ray, the facts
the tests' conditions are about (ties, inactive axes, candidates, where a ray starts and ends).

Rule.  Pixel (u, v): dx = (u - cx) / fx, dy = (v - cy) / fy; per axis a of the world, with the pose T (camera -> world):
D_a = (T[a,0] * dx + T[a,1] * dy) + T[a,2], G_a = T[a,3] / voxelSize + 0.5, E_a = D_a / voxelSize; the axis is active iff
|E_a| > 1e-20, steps by s_a = +1 iff E_a > 0, else -1, with 1/E_a the rounded reciprocal.  The ray starts in voxel
floor(G + E * t_min).  The crossing out of integer coordinate c on axis a happens at t_a(c) = ((float)c - Gs_a) * (1 / E_a),
Gs_a = G_a - 1 for an axis that steps up, G_a otherwise; never for an inactive axis.  The walk takes, again and again, the
first of the three pending crossings in the order (t, priority y < z < x); a crossing with t >= t_max is not taken and ends
the ray.  A visited voxel of a block of the model with weight > 0 is a sample, placed at the camera depth of its centre,
((z0 * x + z1 * y) + z2 * z) + z3 with z0..2 = row 2 of the inverse pose times voxelSize and z3 its last element.  The hit is
the first pair of consecutive visited voxels that are both samples with sdf_prev > 0 >= sdf_cur: depth = t_prev + ((t_cur -
t_prev) * sdf_prev) / (sdf_prev - sdf_cur); no hit: 0.  The normal of a hit is the gradient at the pair's second voxel --
per axis (s+ - s-) * 0.5 where both neighbours are samples, s+ - here or here - s- where one is, no normal where neither --
divided by its length sqrt((gx*gx + gy*gy) + gz*gz) if that is > 0, rotated into the camera frame: n_i = (T[0,i] * w0 +
T[1,i] * w1) + T[2,i] * w2, w = 0; else zeros."""
import numpy as np

F = np.float32
I = np.int64
X, Y, Z = 0, 1, 2
BY_PRIORITY = (Y, Z, X)                  # a tie is won by y, then z, then x
PAIRS = ((X, Y), (X, Z), (Y, Z))
KEY_OFFSET = 1 << 20                     # block keys of |k| < 2^20 pack into 63 bits


class Field:
    """The model's voxels by global integer coordinate, through sorted packed block keys."""

    def __init__(self, model):
        keys = np.array(list(model.keys()), I).reshape(-1, 3)
        assert len(keys) and np.abs(keys).max() < KEY_OFFSET
        packed = self.pack(keys)
        order = np.argsort(packed)
        self.packed = packed[order]
        n = len(keys)
        self.sdf = np.zeros((n + 1, 512), F)                          # row n: the absent block (weight 0: no sample)
        self.weight = np.zeros((n + 1, 512), F)
        vals = list(model.values())
        for row, i in enumerate(order.tolist()):
            self.sdf[row] = np.asarray(vals[i][0], F)
            self.weight[row] = np.asarray(vals[i][1], F)

    @staticmethod
    def pack(keys):
        k = np.asarray(keys, I) + KEY_OFFSET
        return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]

    def voxels(self, c):
        """(allocated, sdf, weight) of the voxels c [N, 3] (int64)."""
        want = self.pack(c >> 3)                                      # floor division by 8
        at = np.minimum(np.searchsorted(self.packed, want), len(self.packed) - 1)
        allocated = self.packed[at] == want
        row = np.where(allocated, at, len(self.packed))
        lin = ((c[:, 2] & 7) << 6) | ((c[:, 1] & 7) << 3) | (c[:, 0] & 7)
        return allocated, self.sdf[row, lin], self.weight[row, lin]


def _crossing(c, Gs, invE, active):
    with np.errstate(over="ignore", invalid="ignore"):
        t = (c.astype(F) - Gs) * invE
    return np.where(active, t, F(np.inf)).astype(F)


def raycast(model, voxel_size, pose, inverse, fx, fy, cx, cy, W, H, t_min, t_max, max_steps=1 << 22):
    """(depth [H, W], normals [H, W, 4], record) of the view.  `inverse` is the cofactor inverse of `pose` (its row 2 places
    the samples).  The record is a dict of arrays [H, W]: found; start [.., 3] (the first voxel); hit [.., 3], first [.., 3] (the pair's two voxels); events
    (crossings taken before the hit or the ray's end); candidates (+ -> - pairs of consecutive samples over the whole ray);
    straddles; tie_xy, tie_xz, tie_yz, tie_xyz (events before the hit or the end at which that many crossings were pending at
    the same time, two-way ties by pair); inactive (axes that never step); starts_in_allocated, ends_in_allocated;
    tmax_equals_event; broken_by_weight (consecutive visited voxels of allocated blocks with sdf + -> - that are no pair
    because a weight is not > 0, before the hit or the end); normal_starved, normal_one_sided (of a hit)."""
    field = Field(model)
    T = np.asarray(pose, F).reshape(4, 4)
    inv = np.asarray(inverse, F).reshape(4, 4)
    vs, t_min, t_max = F(voxel_size), F(t_min), F(t_max)
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    zrow = (inv[2, 0] * vs, inv[2, 1] * vs, inv[2, 2] * vs, inv[2, 3])
    v, u = np.divmod(np.arange(W * H), W)
    N = W * H
    dx, dy = (u.astype(F) - cx) / fx, (v.astype(F) - cy) / fy
    D = np.stack([(T[a, 0] * dx + T[a, 1] * dy) + T[a, 2] for a in range(3)], 1).astype(F)
    G = np.array([T[a, 3] / vs + F(0.5) for a in range(3)], F)
    E = (D / vs).astype(F)
    active = np.abs(E) > F(1.0e-20)
    with np.errstate(divide="ignore"):
        invE = np.where(active, F(1) / E, F(0)).astype(F)
    s = np.where(E > 0, 1, -1).astype(I)
    Gs = np.where(E > 0, G[None, :] - F(1), G[None, :]).astype(F)
    c = np.floor(G[None, :] + E * t_min).astype(I)
    start = c.copy()
    tn = _crossing(c, Gs, invE, active)

    def centre_depth(p):
        return ((zrow[0] * p[:, 0].astype(F) + zrow[1] * p[:, 1].astype(F)) + zrow[2] * p[:, 2].astype(F)) + zrow[3]

    alive = np.ones(N, bool)
    found = np.zeros(N, bool)
    depth = np.zeros(N, F)
    hit, first = np.zeros((N, 3), I), np.zeros((N, 3), I)
    prev_sample, prev_alloc = np.zeros(N, bool), np.zeros(N, bool)
    prev_sdf, prev_t, prev_c = np.zeros(N, F), np.zeros(N, F), np.zeros((N, 3), I)
    last_sdf = np.zeros(N, F)                                         # of the voxel visited before, a sample or not
    count = {k: np.zeros(N, I) for k in ("events", "candidates", "tie_xy", "tie_xz", "tie_yz", "tie_xyz", "broken_by_weight")}
    starts = ends = tmax_event = None
    for step in range(max_steps):
        alloc, sdf, weight = field.voxels(c)
        if starts is None:
            starts, ends, tmax_event = alloc.copy(), np.zeros(N, bool), np.zeros(N, bool)
        with np.errstate(invalid="ignore"):
            sample = alloc & (weight > 0)
            falls = (prev_sdf > 0) & (sdf <= 0)
            broken = alloc & prev_alloc & (last_sdf > 0) & (sdf <= 0) & ~(sample & prev_sample)
        pair = alive & sample & prev_sample & falls
        count["broken_by_weight"] += alive & ~found & broken
        count["candidates"] += pair
        new = pair & ~found
        if new.any():
            t_cur = centre_depth(c)
            with np.errstate(all="ignore"):
                d = prev_t + ((t_cur - prev_t) * prev_sdf) / (prev_sdf - sdf)
            depth[new] = d[new]
            hit[new], first[new] = c[new], prev_c[new]
            found |= new
        upd = alive & sample
        if upd.any():
            prev_t = np.where(upd, centre_depth(c), prev_t).astype(F)
        prev_sdf = np.where(upd, sdf, prev_sdf)
        prev_c = np.where(upd[:, None], c, prev_c)
        prev_sample, prev_alloc, last_sdf = sample, alloc, sdf
        # the first pending crossing in the order (t, priority)
        a = np.full(N, BY_PRIORITY[0], I)
        best = tn[:, BY_PRIORITY[0]]
        for b in BY_PRIORITY[1:]:
            sooner = tn[:, b] < best
            a = np.where(sooner, b, a)
            best = np.where(sooner, tn[:, b], best)
        stops = alive & ~(best < t_max)
        ends |= stops & alloc
        tmax_event |= stops & (best == t_max)
        alive &= ~stops
        if not alive.any():
            break
        counting = alive & ~found
        same = {p: (tn[:, p[0]] == tn[:, p[1]]) & (tn[:, p[0]] == best) for p in PAIRS}
        three = same[(X, Y)] & same[(X, Z)]
        count["tie_xyz"] += counting & three
        for p, name in zip(PAIRS, ("tie_xy", "tie_xz", "tie_yz")):
            count[name] += counting & same[p] & ~three
        count["events"] += counting
        rows = np.nonzero(alive)[0]
        ar = a[rows]
        c[rows, ar] += s[rows, ar]
        tn[rows, ar] = _crossing(c[rows, ar], Gs[rows, ar], invE[rows, ar], active[rows, ar])
    else:
        raise AssertionError("a ray took more steps than the rule allows")

    # normals of the hits
    normals = np.zeros((N, 4), F)
    starved, one_sided = np.zeros(N, bool), np.zeros(N, bool)
    rows = np.nonzero(found)[0]
    if len(rows):
        h = hit[rows]
        _, here, _ = field.voxels(h)
        g = np.zeros((len(rows), 3), F)
        ok = np.ones(len(rows), bool)
        some_one_sided = np.zeros(len(rows), bool)
        with np.errstate(all="ignore"):
            for ax in range(3):
                step = np.zeros(3, I)
                step[ax] = 1
                ap, sp, wp = field.voxels(h + step)
                am, sm, wm = field.voxels(h - step)
                hp, hm = ap & (wp > 0), am & (wm > 0)
                g[:, ax] = np.where(hp & hm, (sp - sm) * F(0.5), np.where(hp, sp - here, np.where(hm, here - sm, F(0))))
                ok &= hp | hm
                some_one_sided |= hp != hm
            length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
            ok_len = ok & (length > 0)
            w = (g / length[:, None]).astype(F)
            for i in range(3):
                n_i = (T[0, i] * w[:, 0] + T[1, i] * w[:, 1]) + T[2, i] * w[:, 2]
                normals[rows, i] = np.where(ok_len, n_i, F(0))
        starved[rows] = ~ok
        one_sided[rows] = ok & some_one_sided

    shape = lambda x: x.reshape((H, W) + x.shape[1:])
    record = {k: shape(val) for k, val in count.items()}
    record.update(found=shape(found), start=shape(start), hit=shape(hit), first=shape(first), straddles=shape(found & ((hit >> 3) != (first >> 3)).any(1)),
                  inactive=shape((~active).sum(1)), starts_in_allocated=shape(starts), ends_in_allocated=shape(ends),
                  tmax_equals_event=shape(tmax_event), normal_starved=shape(starved), normal_one_sided=shape(one_sided))
    return shape(depth), shape(normals), record
