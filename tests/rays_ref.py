"""The specification of vh_cast_rays (include/voxelhash.h "the model met by rays") in vectorised numpy: the DDA
of tests/raycast_ref.py with the camera taken out, IEEE float32 throughout (every multiply and add rounded on its own), over a
model dictionary as tests/mesh_models.py defines it.  It does not import the product, knows nothing of a table, a bitmap or a
jump, and walks every ray voxel by voxel to its end.

Rule.  A ray is eight floats: origin O, t_min, direction D (any length), t_max.  Per axis a: G_a = O_a / voxelSize + 0.5,
E_a = D_a / voxelSize; the axis is active iff |E_a| > 1e-20, steps by s_a = +1 iff E_a > 0, else -1, with 1/E_a the rounded
reciprocal.  The ray starts in voxel floor(G + E * t_min).  The crossing out of integer coordinate c on axis a happens at
t_a(c) = ((float)c - Gs_a) * (1 / E_a), Gs_a = G_a - 1 for an axis that steps up, G_a otherwise; never for an inactive axis.
The walk takes, again and again, the first of the three pending crossings in the order (t, priority y < z < x); a crossing
with t >= t_max is not taken and ends the ray.  A visited voxel c of a block of the model with weight > 0 is a sample at
parameter ((w0 * cx + w1 * cy) + w2 * cz) + w3: with a shared plane P, w = (P0 * vs, P1 * vs, P2 * vs, P3); without one,
dd = (Dx * Dx + Dy * Dy) + Dz * Dz, k = 1 / dd, w_a = (D_a * k) * vs, w3 = -(((Ox * Dx + Oy * Dy) + Oz * Dz) * k): the
projection of the voxel's centre onto its own ray.  The hit is the first pair of consecutive visited voxels that are both
samples with sdf_prev > 0 >= sdf_cur: t = t_prev + ((t_cur - t_prev) * sdf_prev) / (sdf_prev - sdf_cur), status 1, the voxel
the pair's second; no hit: t NaN, status 0, voxel zeros.  The normal of a hit is the gradient at that voxel -- per axis
(s+ - s-) * 0.5 where both neighbours are samples, s+ - here or here - s- where one is, none where neither -- divided by its
length sqrt((gx*gx + gy*gy) + gz*gz) if that is > 0, in the world frame; else zeros.

Refused (status -1, t NaN, voxel and normal zeros, no walk), evaluated in float64: a float that is not finite; not
t_max > t_min; dd == 0; 16 + sum_a (1.01 * (t_max - t_min) * |D_a| / vs + 2) not < 2^22; |G_a| + (|t_max| + |t_min|) * |D_a| / vs
not < 2^23 on some axis."""
import numpy as np

from raycast_ref import BY_PRIORITY, PAIRS, Field, F, I, X, Y, Z, _crossing

HIT, MISS, REFUSED = 1, 0, -1
MAX_STEPS = 1 << 22


def accepted(rays, voxel_size):
    """Which rays are walked (the others are refused), and each ray's step bound."""
    r = np.asarray(rays, F).reshape(-1, 8)
    vs = F(voxel_size)
    with np.errstate(all="ignore"):
        O, D, t0, t1 = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
        dd = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
        G = (O / vs + F(0.5)).astype(np.float64)
        e = np.abs(D.astype(np.float64)) / np.float64(vs)
        span = (t1.astype(np.float64) - t0.astype(np.float64))[:, None]
        steps = 16.0 + (1.01 * span * e + 2.0).sum(1)
        reach = np.abs(G) + (np.abs(t1.astype(np.float64)) + np.abs(t0.astype(np.float64)))[:, None] * e
        ok = np.isfinite(r).all(1) & (t1 > t0) & (dd != 0) & (steps < 2.0 ** 22) & (reach < 2.0 ** 23).all(1)
    return ok, steps


def cast(model, voxel_size, rays, depth_plane=None, max_steps=MAX_STEPS):
    """(t [n], status [n], voxel [n, 3], normal [n, 3], record) of the rays [n, 8].  `model` is a dictionary or a Field.  The
    record is a dict of arrays [n]: found; refused; start [n, 3] (the first voxel); hit, first [n, 3] (the pair's two voxels);
    events (crossings taken before the hit or the ray's end); candidates (+ -> - pairs of consecutive samples over the whole
    ray); tie_xy, tie_xz, tie_yz, tie_xyz (events before the hit or the end at which that many crossings were pending at the
    same time); inactive (axes that never step); starts_in_allocated, ends_in_allocated; tmax_equals_event."""
    field = model if isinstance(model, Field) else Field(model)
    rays = np.ascontiguousarray(np.asarray(rays, F).reshape(-1, 8))
    total = len(rays)
    vs = F(voxel_size)
    ok, _ = accepted(rays, vs)
    sel = np.nonzero(ok)[0]
    r = rays[sel]
    N = len(r)
    O, D, t_min, t_max = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
    with np.errstate(all="ignore"):
        G = (O / vs + F(0.5)).astype(F)
        E = (D / vs).astype(F)
        active = np.abs(E) > F(1.0e-20)
        invE = np.where(active, F(1) / E, F(0)).astype(F)
        s = np.where(E > 0, 1, -1).astype(I)
        Gs = np.where(E > 0, G - F(1), G).astype(F)
        c = np.floor(G + E * t_min[:, None]).astype(I)
        if depth_plane is not None:
            P = np.asarray(depth_plane, F).reshape(4)
            w = np.broadcast_to(np.array([P[0] * vs, P[1] * vs, P[2] * vs, P[3]], F), (N, 4))
        else:
            dd = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
            k = F(1) / dd
            w3 = -(((O[:, 0] * D[:, 0] + O[:, 1] * D[:, 1]) + O[:, 2] * D[:, 2]) * k)
            w = np.stack([(D[:, 0] * k) * vs, (D[:, 1] * k) * vs, (D[:, 2] * k) * vs, w3], 1).astype(F)
    start = c.copy()
    tn = _crossing(c, Gs, invE, active)

    def parameter(p):
        with np.errstate(all="ignore"):
            return ((w[:, 0] * p[:, 0].astype(F) + w[:, 1] * p[:, 1].astype(F)) + w[:, 2] * p[:, 2].astype(F)) + w[:, 3]

    alive = np.ones(N, bool)
    found = np.zeros(N, bool)
    t = np.full(N, np.nan, F)
    hit, first = np.zeros((N, 3), I), np.zeros((N, 3), I)
    prev_sample = np.zeros(N, bool)
    prev_sdf, prev_t, prev_c = np.zeros(N, F), np.zeros(N, F), np.zeros((N, 3), I)
    count = {k: np.zeros(N, I) for k in ("events", "candidates", "tie_xy", "tie_xz", "tie_yz", "tie_xyz")}
    starts, ends, tmax_event = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    for step in range(max_steps if N else 0):
        alloc, sdf, weight = field.voxels(c)
        if step == 0:
            starts = alloc.copy()
        with np.errstate(invalid="ignore"):
            sample = alloc & (weight > 0)
            falls = (prev_sdf > 0) & (sdf <= 0)
        pair = alive & sample & prev_sample & falls
        count["candidates"] += pair
        new = pair & ~found
        here = parameter(c) if (new.any() or (alive & sample).any()) else prev_t
        if new.any():
            with np.errstate(all="ignore"):
                d = prev_t + ((here - prev_t) * prev_sdf) / (prev_sdf - sdf)
            t[new] = d[new]
            hit[new], first[new] = c[new], prev_c[new]
            found |= new
        upd = alive & sample
        prev_t = np.where(upd, here, prev_t).astype(F)
        prev_sdf = np.where(upd, sdf, prev_sdf)
        prev_c = np.where(upd[:, None], c, prev_c)
        prev_sample = sample
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
        assert N == 0, "a ray took more steps than the rule allows"

    # normals of the hits: the gradient in the world frame
    normal = np.zeros((N, 3), F)
    rows = np.nonzero(found)[0]
    if len(rows):
        h = hit[rows]
        _, here, _ = field.voxels(h)
        g = np.zeros((len(rows), 3), F)
        has = np.ones(len(rows), bool)
        with np.errstate(all="ignore"):
            for ax in range(3):
                one = np.zeros(3, I)
                one[ax] = 1
                ap, sp, wp = field.voxels(h + one)
                am, sm, wm = field.voxels(h - one)
                hp, hm = ap & (wp > 0), am & (wm > 0)
                g[:, ax] = np.where(hp & hm, (sp - sm) * F(0.5), np.where(hp, sp - here, np.where(hm, here - sm, F(0))))
                has &= hp | hm
            length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
            has &= length > 0
            normal[rows] = np.where(has[:, None], (g / length[:, None]).astype(F), F(0))

    def spread(x, fill=0):
        out = np.full((total,) + x.shape[1:], fill, x.dtype)
        out[sel] = x
        return out

    status = np.full(total, REFUSED, np.int32)
    status[sel] = np.where(found, HIT, MISS)
    record = {k: spread(v) for k, v in count.items()}
    record.update(found=spread(found), refused=~ok, start=spread(start), hit=spread(hit), first=spread(first),
                  inactive=spread((~active).sum(1)), starts_in_allocated=spread(starts), ends_in_allocated=spread(ends),
                  tmax_equals_event=spread(tmax_event))
    return spread(t, np.nan), status, spread(np.where(found[:, None], hit, 0)), spread(normal), record


def same_bits(got, want):
    """Bit-equal, two NaNs counting as equal (the payload of a made-up NaN is nobody's rule)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
