"""Band allocation restated from its specification (include/voxelhash.h, "band_mode"; the comment above BandWalk in
csrc/vh_alloc.hip), independent of the kernel's and the oracle's block DDA.

The two END POINTS of a pixel's segment are fp32 values the specification states operation by operation, so they are computed
here in numpy float32, one rounding per operation.  The WALK between them is a geometric rule -- which 8^3 blocks a segment
crosses, in which order, with which tie order -- and is evaluated in exact rational arithmetic (fractions.Fraction): every
crossing parameter is the exact quotient (boundary - A) / (B - A), none is accumulated.

Block k covers [(8k - 0.5) * vs, (8k + 7.5) * vs) on an axis: world2Block rounds coordinate / vs to the nearest voxel (half away
from zero) and floors the voxel index by 8.

The tolerance of must_may()
---------------------------
For end points that are not exactly representable walks, fp32 moves every crossing a little.  With u = 2^-24 (half an ulp,
relative), C = the largest |coordinate| / vs of the case and L = the largest |B - A| component / vs (both in voxels):
  * the end points themselves: T * v is 7 operations per row, band * (R n) 5 more, the sum / difference 1, the ray band's
    s / z and its product 2 -- at most 13 roundings of values no larger than C, each <= C u voxels;
  * world2voxel's quotient coordinate / vs (start and end block): 1 rounding, <= C u;
  * the first boundary (8k - 0.5) * vs, its distance to the start and the quotient by the direction: 3 roundings, <= C u + 2 L u;
  * tdelta = 8 vs / |dir|: the direction's rounding and the quotient's, 2 L u, and it enters tmax up to 62 times; each of the 62
    additions rounds once more, <= L u each: (62 + 62 + 62) L u at most, counted as 3 * 62 L u.
A crossing of axis a misjudged by dt moves the point on axis a by |dir_a| dt, which is what the sum above bounds, in voxels:
(13 + 1 + 1) C u + (2 + 186) L u.  With the factor of 4 the issue asks for:

    eps = 4 * 2^-24 * (15 C + 188 L)   voxels.

The visited set of a DDA with perturbed crossing times is: the blocks whose three (perturbed) per-axis parameter intervals
intersect.  Each perturbed interval lies inside the exact interval of the box grown by eps and contains that of the box shrunk
by eps, hence MUST <= visited <= MAY."""
from fractions import Fraction

import numpy as np

F = np.float32
MAX_STEPS = 62
HALF = Fraction(1, 2)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


# ---------------------------------------------------------------------------
# fp32, operation by operation
# ---------------------------------------------------------------------------
def mat4_f32(T, x, y, z, w):
    """Rows of T * (x, y, z, w) summed left to right, every product and sum rounded to fp32."""
    T = np.asarray(T, F).reshape(4, 4)
    x, y, z, w = F(x), F(y), F(z), F(w)
    with np.errstate(all="ignore"):
        return [F(F(F(F(T[r, 0] * x) + F(T[r, 1] * y)) + F(T[r, 2] * z)) + F(T[r, 3] * w)) for r in range(3)]


def normal_is_absent(n):
    n = [F(c) for c in n[:3]]
    return all(c == 0 for c in n) or any(c != c for c in n)


def ends_normal(v, n, T, band):
    """(surface point g, start, end) of VH_BAND_NORMAL_DDA; start = end = None where the pixel has no normal."""
    T = np.asarray(T, F).reshape(4, 4)
    g = mat4_f32(T, *v)
    if normal_is_absent(n):
        return g, None, None
    b, nx, ny, nz = F(band), F(n[0]), F(n[1]), F(n[2])
    start, end = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            nw = F(F(F(T[a, 0] * nx) + F(T[a, 1] * ny)) + F(T[a, 2] * nz))
            start.append(F(g[a] - F(b * nw)))
            end.append(F(g[a] + F(b * nw)))
    return g, start, end


def ends_ray(v, T, band):
    """(start, end) of VH_BAND_RAY_DDA: the vertex scaled to camera depths z - b (z, if that is not positive) and z + b."""
    x, y, z, w = [F(c) for c in v]
    b = F(band)
    with np.errstate(all="ignore"):
        s0 = F(z - b)
        if not s0 > 0:
            s0 = z
        s1 = F(z + b)
        c0, c1 = F(s0 / z), F(s1 / z)
        return mat4_f32(T, F(x * c0), F(y * c0), s0, w), mat4_f32(T, F(x * c1), F(y * c1), s1, w)


def f2i_rz(x):
    """float -> int32: truncate, saturate, NaN -> 0."""
    x = float(x)
    if x != x:
        return 0
    if x >= 2147483648.0:
        return INT_MAX
    if x <= -2147483648.0:
        return INT_MIN
    return int(x)


def voxel2block1(v):
    """Floor division by 8 the way voxel2Block writes it (v - 7 wraps in 32 bits, the division truncates)."""
    if v < 0:
        v = ((v & 0xffffffff) - 7) & 0xffffffff
        if v >= 1 << 31:
            v -= 1 << 32
    return v // 8 if v >= 0 else -((-v) // 8)


def world2block_f32(p, vs):
    """world2Block in fp32: correctly rounded quotient, + copysign(0.5), truncation, floor by 8."""
    out = []
    with np.errstate(all="ignore"):
        for c in p[:3]:
            q = F(F(c) / F(vs))
            out.append(voxel2block1(f2i_rz(F(q + np.copysign(F(0.5), q)))))
    return tuple(out)


# ---------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------
def _frac(x):
    return Fraction(float(x))


def block_of_exact(q):
    """Block of the exact voxel coordinate q (a Fraction): nearest voxel, half away from zero, floored by 8."""
    v = (abs(q) + HALF).__floor__()
    return (v if q >= 0 else -v) // 8


def walk_exact(A, B, vs, max_steps=MAX_STEPS, info=None):
    """The ordered keys of the 6-connected walk from A's block along the segment A -> B.

    Axis a is crossed for the i-th time at t = (boundary - A_a) / (B_a - A_a), boundary = (8 (c_a + i + 1) - 0.5) vs going up and
    (8 (c_a - i) - 0.5) vs going down, c_a = A's block.  The next step takes x when its crossing is strictly the smallest, else z
    when z's is smaller than y's, else y.  The walk ends at B's block, after max_steps steps, or when the next crossing lies
    beyond the segment (t > 1).  info (a dict) receives 'ties' (steps decided by the tie order) and 'capped'."""
    vsq = _frac(vs)
    a0 = [_frac(c) / vsq for c in A]
    d = [_frac(B[a]) / vsq - a0[a] for a in range(3)]
    cur = [block_of_exact(q) for q in a0]
    end = [block_of_exact(_frac(c) / vsq) for c in B]
    sgn = [(x > 0) - (x < 0) for x in d]

    def crossing(a):
        if sgn[a] == 0:
            return None                                     # never
        return (8 * (cur[a] + (1 if sgn[a] > 0 else 0)) - HALF - a0[a]) / d[a]

    keys, ties, capped = [tuple(cur)], 0, False
    while cur != end:
        if len(keys) - 1 == max_steps:
            capped = True
            break
        t = [crossing(a) for a in range(3)]

        def less(p, q):                                     # p < q with None = +infinity
            return p is not None and (q is None or p < q)
        if less(t[0], t[1]) and less(t[0], t[2]):
            a = 0
        elif less(t[2], t[1]):
            a = 2
        else:
            a = 1
        if t[a] is None or t[a] > 1:
            break
        ties += sum(1 for o in range(3) if o != a and t[o] is not None and t[o] == t[a])
        cur[a] += sgn[a]
        keys.append(tuple(cur))
    if info is not None:
        info["ties"], info["capped"] = ties, capped
    return keys


def eps_voxels(A, B, vs, extra=()):
    """The tolerance of must_may in voxels (module docstring); extra: further coordinates the end points were made from."""
    vsf = float(vs)
    C = max(abs(float(c)) for c in list(A) + list(B) + list(extra)) / vsf
    L = max(abs(float(B[a]) - float(A[a])) for a in range(3)) / vsf
    return Fraction(4 * (15 * C + 188 * L) / 2.0 ** 24)


def _interval(a0, d, lo, hi):
    """[t0, t1] within [0, 1] where a0 + t d lies in [lo, hi]; None if empty."""
    if lo > hi:
        return None
    if d == 0:
        return (Fraction(0), Fraction(1)) if lo <= a0 <= hi else None
    t0, t1 = (lo - a0) / d, (hi - a0) / d
    if t0 > t1:
        t0, t1 = t1, t0
    t0, t1 = max(t0, Fraction(0)), min(t1, Fraction(1))
    return (t0, t1) if t0 <= t1 else None


def must_may(A, B, vs, eps):
    """(MUST, MAY): MAY = blocks whose closed box grown by eps voxels per side meets the segment A -> B; MUST = blocks whose box
    shrunk by eps meets it in positive length, and the block whose shrunk box holds A itself (the start block is always demanded)."""
    vsq = _frac(vs)
    eps = Fraction(eps)
    a0 = [_frac(c) / vsq for c in A]
    d = [_frac(B[a]) / vsq - a0[a] for a in range(3)]
    per_axis = []
    for a in range(3):
        lo_c, hi_c = min(a0[a], a0[a] + d[a]), max(a0[a], a0[a] + d[a])
        k0, k1 = ((lo_c - eps + HALF) // 8).__floor__() - 1, ((hi_c + eps + HALF) // 8).__floor__() + 1
        rows = []
        for k in range(k0, k1 + 1):
            lo, hi = 8 * k - HALF, 8 * k + 8 - HALF
            may = _interval(a0[a], d[a], lo - eps, hi + eps)
            if may is None:
                continue
            must = _interval(a0[a], d[a], lo + eps, hi - eps)
            holds_a = lo + eps <= a0[a] <= hi - eps
            rows.append((k, may, must, holds_a))
        per_axis.append(rows)
    MUST, MAY = set(), set()
    for kx, mx, ux, hx in per_axis[0]:
        for ky, my, uy, hy in per_axis[1]:
            t0, t1 = max(mx[0], my[0]), min(mx[1], my[1])
            if t0 > t1:
                continue
            for kz, mz, uz, hz in per_axis[2]:
                if max(t0, mz[0]) > min(t1, mz[1]):
                    continue
                MAY.add((kx, ky, kz))
                if hx and hy and hz:
                    MUST.add((kx, ky, kz))
                elif ux and uy and uz and max(ux[0], uy[0], uz[0]) < min(ux[1], uy[1], uz[1]):
                    MUST.add((kx, ky, kz))
    return MUST, MAY


# ---------------------------------------------------------------------------
# VH_BAND_RAY
# ---------------------------------------------------------------------------
def ray_half(vs, band):
    """Samples on each side of the surface sample: min(ceil(band / (4 vs)), 31); 0 without a band."""
    if not F(band) > 0:
        return 0
    return min(int(np.ceil(F(band) / F(F(4) * F(vs)))), 31)


def ray_samples(v, vs, band, T):
    """[(k, key)] of one pixel under VH_BAND_RAY: sample k at camera depth z + (k - half) * 4 vs, skipped when that is <= 0 unless
    k = half (the vertex itself, bit for bit); key = world2Block of the fp32 point, the divisions correctly rounded."""
    x, y, z, w = [F(c) for c in v]
    step = F(F(4) * F(vs))
    half = ray_half(vs, band)
    out = []
    with np.errstate(all="ignore"):
        for k in range(2 * half + 1):
            if k == half:
                p = mat4_f32(T, x, y, z, w)
            else:
                s = F(z + F(F(F(k) - F(half)) * step))
                if not s > 0:
                    continue
                scale = F(s / z)
                p = mat4_f32(T, F(x * scale), F(y * scale), s, w)
            out.append((k, world2block_f32(p, vs)))
    return out
