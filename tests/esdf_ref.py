"""The specification of vh_esdf_lattice in numpy, by definition: the site voxels of the box grown by the radius are gathered
into lists and every output voxel takes a brute-force minimum of |g - s|^2 over them, in chunks.  Nothing here is separable,
packed into bits or windowed: it shares no step with the kernels.  Over a model dictionary as tests/mesh_models.py defines it;
voxel validity is tests/sample_ref.py's (the rule of vh_sample_lattice).  It does not import the product.

Rule (include/voxelhash.h, "the model as a distance field"): a valid voxel is inside iff sdf < 0, else outside; every other
voxel is unknown, and `unknown` (KEEP, FREE, OCCUPIED) remaps the unknown ones first.  With R = radius, P(g) = min |g - s|^2
over inside s with |g - s|^2 <= R^2, N(g) the same over outside s.  D(g) = P or FAR for an outside voxel, -N or -FAR for an
inside voxel, NONE for an unknown one.  In metres: sign * (sqrt(float32(|D|)) * float32(voxelSize)), +-inf, NaN."""
import numpy as np

import sample_ref as sr

F = np.float32
KEEP, FREE, OCCUPIED = 0, 1, 2
FAR, NONE = 2 ** 31 - 1, -2 ** 31
MAX_RADIUS = 255
PAIRS = 1 << 22                      # |chunk| * |sites| per brute-force step


def classify(field, g, unknown=KEEP):
    """(inside, outside) of the voxels g [..., 3]."""
    sdf, _ = field.voxels(g)
    with np.errstate(invalid="ignore"):
        valid = sdf == sdf
        inside = valid & (sdf < 0)
    outside = valid & ~inside
    if unknown == FREE:
        outside = ~inside
    elif unknown == OCCUPIED:
        inside = ~outside
    else:
        assert unknown == KEEP
    return inside, outside


def grid(lo, dims):
    """The voxels of a box as [dims[2], dims[1], dims[0], 3] int64."""
    k, j, i = np.meshgrid(*(np.arange(int(d), dtype=np.int64) for d in (dims[2], dims[1], dims[0])), indexing="ij")
    return np.stack([i, j, k], -1) + np.asarray(lo, np.int64)


def sites(field, lo, dims, unknown, inside):
    """The sites of one class (inside or outside) among the voxels of the box lo <= g < lo + dims, [N, 3].  A class that no
    unknown voxel joins has its sites in the model's own blocks, so only the blocks that meet the box are looked at (the box may
    be large and almost empty); a class the unknown voxels join is classified voxel by voxel."""
    lo, dims = np.asarray(lo, np.int64), np.asarray(dims, np.int64)
    if (unknown == FREE and not inside) or (unknown == OCCUPIED and inside):
        assert dims.prod() < 1 << 24, "a dense classification is meant for small radii"
        g = grid(lo, dims).reshape(-1, 3)
    else:
        keys = np.array(list(field.row), np.int64).reshape(-1, 3)
        keys = keys[((keys * 8 + 7 >= lo) & (keys * 8 < lo + dims)).all(1)]
        i = np.arange(512)
        local = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
        g = (keys[:, None, :] * 8 + local[None, :, :]).reshape(-1, 3)
        g = g[((g >= lo) & (g < lo + dims)).all(1)]
    if len(g) == 0:
        return np.zeros((0, 3), np.int64)
    return g[classify(field, g, unknown)[0 if inside else 1]]


def nearest(g, s, radius):
    """min over the sites s [N, 3] of |g - s|^2 for each g [M, 3], -1 where no site has |g - s|^2 <= radius^2."""
    out = np.full(len(g), -1, np.int64)
    if len(s) == 0 or len(g) == 0:
        return out
    step = max(1, PAIRS // max(1, min(len(s), 1 << 16)))
    for a in range(0, len(g), step):
        c = g[a:a + step]
        near = s[((s >= c.min(0) - radius) & (s <= c.max(0) + radius)).all(1)]      # (a shortcut that changes no minimum)
        if len(near) == 0:
            continue
        sub = max(1, PAIRS // len(near))
        for b in range(0, len(c), sub):
            d = c[b:b + sub, None, :] - near[None, :, :]
            d2 = (d * d).sum(-1)
            d2[d2 > radius * radius] = np.iinfo(np.int64).max
            m = d2.min(1)
            out[a + b:a + b + len(m)] = np.where(m == np.iinfo(np.int64).max, -1, m)
    return out


def esdf(model, lo, dims, radius, unknown=KEEP):
    """D [dims[2], dims[1], dims[0]] int32."""
    field = model if isinstance(model, sr.Field) else sr.Field(model)
    radius = int(radius)
    assert 1 <= radius <= MAX_RADIUS
    shape = (int(dims[2]), int(dims[1]), int(dims[0]))
    if 0 in shape:
        return np.zeros(shape, np.int32)
    lo, dims = np.asarray(lo, np.int64), np.asarray(dims, np.int64)
    g = grid(lo, dims).reshape(-1, 3)
    inside, outside = classify(field, g, unknown)
    out = np.full(len(g), NONE, np.int64)
    if outside.any():
        p = nearest(g[outside], sites(field, lo - radius, dims + 2 * radius, unknown, True), radius)
        out[outside] = np.where(p < 0, FAR, p)
    if inside.any():
        n = nearest(g[inside], sites(field, lo - radius, dims + 2 * radius, unknown, False), radius)
        out[inside] = np.where(n < 0, -FAR, -n)
    return out.astype(np.int32).reshape(shape)


def distance(d, voxel_size):
    """The float form of D, float32 throughout."""
    d = np.asarray(d, np.int64)
    mag = (np.sqrt(np.abs(d).astype(F)).astype(F) * F(voxel_size)).astype(F)
    out = np.where(d < 0, -mag, mag).astype(F)
    out[d == FAR] = F(np.inf)
    out[d == -FAR] = F(-np.inf)
    out[d == NONE] = F(np.nan)
    return out


def same_bits(a, b):
    """Bit for bit (two NaNs count as equal), for either output."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(a, b)) if a.dtype != F else sr.same_bits(a, b)
