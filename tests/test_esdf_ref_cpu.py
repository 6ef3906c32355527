"""tests/esdf_ref.py (the specification of vh_esdf_lattice) pinned to facts computed without it: nested loops over every
offset of the radius' cube on random models, the sign and +-0 rule, FAR and NONE, independence from the box, and the float
form.  Boxes of at most 14^3 voxels, radii 1 .. 9, all three treatments of unknown voxels.  No GPU."""
import itertools

import numpy as np
import pytest

import esdf_ref as er

F = np.float32
MODES = (er.KEEP, er.FREE, er.OCCUPIED)


def random_model(seed, keys=None, dead=0.3):
    """Blocks of noise with zeros of both signs, +-inf, NaN and weight 0 sprinkled in; a random half of a 3x3x3 cluster."""
    rng = np.random.RandomState(seed)
    if keys is None:
        keys = [k for k in itertools.product((-1, 0, 1), repeat=3) if rng.uniform() < 0.5] or [(0, 0, 0)]
    model = {}
    for k in keys:
        sdf = rng.uniform(-1, 1, 512).astype(F)
        u = rng.uniform(size=512)
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F)
        sdf = np.where(u < 0.15, special[rng.randint(0, 5, 512)], sdf).astype(F)
        weight = np.where(rng.uniform(size=512) < dead, 0, 1).astype(F)
        model[k] = (sdf, weight)
    return model


def class_of(model, g, unknown):
    """'i', 'o' or 'u' for one voxel, from the dictionary alone."""
    key = tuple(int(c) >> 3 for c in g)
    c = "u"
    if key in model:
        at = ((int(g[2]) & 7) << 6) | ((int(g[1]) & 7) << 3) | (int(g[0]) & 7)
        s, w = float(model[key][0][at]), float(model[key][1][at])
        if w > 0 and s == s:
            c = "i" if s < 0 else "o"
    if c == "u" and unknown != er.KEEP:
        c = "o" if unknown == er.FREE else "i"
    return c


def by_loops(model, lo, dims, radius, unknown):
    out = np.zeros((dims[2], dims[1], dims[0]), np.int64)
    span = range(-radius, radius + 1)
    cache = {}

    def cls(g):
        if g not in cache:
            cache[g] = class_of(model, g, unknown)
        return cache[g]
    for k in range(dims[2]):
        for j in range(dims[1]):
            for i in range(dims[0]):
                g = (lo[0] + i, lo[1] + j, lo[2] + k)
                mine = cls(g)
                if mine == "u":
                    out[k, j, i] = er.NONE
                    continue
                other = "i" if mine == "o" else "o"
                best = None
                for dz in span:
                    for dy in span:
                        for dx in span:
                            d2 = dx * dx + dy * dy + dz * dz
                            if d2 <= radius * radius and (best is None or d2 < best) and cls((g[0] + dx, g[1] + dy, g[2] + dz)) == other:
                                best = d2
                sign = 1 if mine == "o" else -1
                out[k, j, i] = sign * (er.FAR if best is None else best)
    return out.astype(np.int32)


@pytest.mark.parametrize("unknown", MODES)
@pytest.mark.parametrize("radius", range(1, 10))
def test_against_nested_loops(radius, unknown):
    model = random_model(100 + radius)
    dims = (6, 5, 4) if radius <= 3 else (4, 3, 2) if radius <= 6 else (3, 2, 2)
    rng = np.random.RandomState(radius * 3 + unknown)
    lo = tuple(int(v) for v in rng.randint(-9, 10, 3))
    want = by_loops(model, lo, dims, radius, unknown)
    got = er.esdf(model, lo, dims, radius, unknown)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if unknown == er.KEEP:
        assert (want == er.NONE).any() or radius > 6
    else:
        assert not (want == er.NONE).any()


def test_a_14_cube_has_every_kind_of_value():
    model = random_model(7, keys=[(0, 1, 1)], dead=0.5)
    model[(0, 0, 0)] = (np.full(512, -1.0, F), np.ones(512, F))      # its middle: no outside voxel within 2
    model[(1, 0, 0)] = (np.full(512, 1.0, F), np.ones(512, F))       # ... and no inside voxel
    d = er.esdf(model, (-2, -1, -3), (14, 14, 14), 2)
    kinds = [(d == er.NONE).sum(), (d == er.FAR).sum(), (d == -er.FAR).sum(), ((d > 0) & (d < er.FAR)).sum(),
             ((d < 0) & (d > -er.FAR)).sum()]
    assert min(kinds) > 0 and (d != 0).all() and (np.abs(d[(d > -er.FAR) & (d < er.FAR) & (d != er.NONE)]) <= 4).all(), kinds


def one_block(values, weights=None):
    sdf = np.full(512, 1.0, F)
    w = np.ones(512, F) if weights is None else np.asarray(weights, F)
    for (x, y, z), v in values.items():
        sdf[(z << 6) | (y << 3) | x] = v
    return {(0, 0, 0): (sdf, w)}


def test_sign_and_zero_rule():
    # along x at y = z = 0: +1, -0.0, +0.0, -inf, -1e-45 (subnormal), NaN, +inf, +1; every other voxel of the block +1.
    # inside = {3, 4} (the zeros of either sign are outside); the nearest outside voxel of 4 is (4, 1, 0)
    model = one_block({(1, 0, 0): -0.0, (2, 0, 0): 0.0, (3, 0, 0): -np.inf, (4, 0, 0): -1e-45, (5, 0, 0): np.nan, (6, 0, 0): np.inf})
    want = [9, 4, 1, -1, -1, er.NONE, 4, 9]
    assert er.esdf(model, (0, 0, 0), (8, 1, 1), 3)[0, 0].tolist() == want
    assert by_loops(model, (0, 0, 0), (8, 1, 1), 3, er.KEEP)[0, 0].tolist() == want


def test_far_and_none_and_the_exact_cap():
    w = np.zeros(512, F)
    w[0] = 1                                  # (0,0,0): inside
    for x, y, z in ((5, 0, 0), (3, 4, 0), (0, 3, 4), (4, 4, 0), (6, 0, 0), (2, 3, 6), (7, 1, 0)):
        w[(z << 6) | (y << 3) | x] = 1
    model = one_block({(0, 0, 0): -1.0}, w)
    at = lambda d, x, y, z: int(d[z, y, x])
    d5 = er.esdf(model, (0, 0, 0), (8, 8, 8), 5)
    assert [at(d5, *p) for p in ((5, 0, 0), (3, 4, 0), (0, 3, 4))] == [25, 25, 25]
    assert [at(d5, *p) for p in ((4, 4, 0), (6, 0, 0))] == [er.FAR, er.FAR]
    assert at(d5, 0, 0, 0) == -25 and at(d5, 1, 0, 0) == er.NONE
    d7 = er.esdf(model, (0, 0, 0), (8, 8, 8), 7)
    assert at(d7, 2, 3, 6) == 49 and at(d7, 7, 1, 0) == er.FAR and at(d7, 6, 0, 0) == 36
    # FREE: the unknown voxels are outside and sites; OCCUPIED: inside and sites
    free = er.esdf(model, (0, 0, 0), (8, 8, 8), 5, er.FREE)
    assert at(free, 0, 0, 0) == -1 and at(free, 1, 0, 0) == 1 and at(free, 6, 0, 0) == er.FAR and not (free == er.NONE).any()
    occ = er.esdf(model, (0, 0, 0), (8, 8, 8), 5, er.OCCUPIED)
    assert at(occ, 5, 0, 0) == 1 and at(occ, 1, 0, 0) == -16 and at(occ, 0, 0, 0) == -25


@pytest.mark.parametrize("unknown", MODES)
def test_independence_from_the_box(unknown):
    model = random_model(31)
    model[(2, 0, 0)] = (np.full(512, -1.0, F), np.ones(512, F))      # a slab of sites outside both boxes, within R of them
    model[(1, 0, 0)] = (np.full(512, 1.0, F), np.ones(512, F))       # ... and outside voxels that see it
    a = er.esdf(model, (3, -2, 0), (9, 7, 5), 9, unknown)
    b = er.esdf(model, (7, 1, 2), (8, 9, 6), 9, unknown)
    # overlap: x 7..11, y 1..4, z 2..4
    assert np.array_equal(a[2:5, 3:7, 4:9], b[0:3, 0:4, 0:5])
    big = er.esdf(model, (0, -4, -2), (14, 14, 10), 9, unknown)
    assert np.array_equal(big[2:7, 2:9, 3:12], a)
    near = a[:, :, -1]                                               # x = 11: five voxels from the slab at x = 16
    assert ((near > 0) & (near <= 25)).any()


def test_float_form():
    d = np.array([1, 2, 3, 49, 65025, -1, -2, -65025, er.FAR, -er.FAR, er.NONE], np.int32)
    f = er.distance(d, 0.02)
    assert f.dtype == F
    vs = F(0.02)
    want = [F(1) * vs, np.sqrt(F(2)) * vs, np.sqrt(F(3)) * vs, F(7) * vs, F(255) * vs, -(F(1) * vs), -(np.sqrt(F(2)) * vs),
            -(F(255) * vs)]
    assert f[:8].view(np.uint32).tolist() == np.array(want, F).view(np.uint32).tolist()
    assert f[8] == np.inf and f[9] == -np.inf and np.isnan(f[10])
    assert er.same_bits(f, f.copy()) and not er.same_bits(f, -f)
