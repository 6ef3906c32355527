"""tests/sample_ref.py (the specification of vh_sample_sdf / vh_sample_lattice) pinned to facts computed without it, so that
the reference cannot be wrong in the same way as the kernel: stored voxels, world2Voxel's rounding, exact affine fields, the
mesh's gradient rule as tests/mesh_ref.py applies it, floor against truncation, and the domain.  No GPU."""
import numpy as np

import mesh_models as mm
import mesh_ref
import sample_ref as sr

F = np.float32
U = np.uint32
VS = F(0.02)


def stored(model, g):
    """The voxel g of the model, straight from the dictionary: (sdf, weight) or None when the block is absent."""
    key = tuple(int(c) >> 3 for c in g)
    if key not in model:
        return None
    index = ((int(g[2]) & 7) << 6) | ((int(g[1]) & 7) << 3) | (int(g[0]) & 7)
    return model[key][0][index], model[key][1][index]


def affine_model(keys, a, b):
    """sdf = a . g + b at every voxel of the blocks, weight 1: small integers, exact in float32."""
    i = np.arange(512)
    local = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    return {k: ((((np.array(k) * 8 + local) * np.array(a)).sum(1) + b).astype(F), np.ones(512, F)) for k in keys}


def test_nearest_on_the_lattice_returns_the_stored_voxel():
    model = mm.uniform_model(mm.cube_keys(-8, 8), seed=41, dead=0.05)
    rng = np.random.RandomState(1)
    g = rng.randint(-64, 65, (4000, 3))
    g[:8] = [[-64, -64, -64], [64, 64, 64], [0, 0, 0], [-1, -1, -1], [-8, 7, 8], [63, -64, 0], [64, 0, -64], [-9, 8, -8]]
    sdf, weight, _ = sr.sample(model, (g.astype(F) * VS).astype(F), VS, sr.NEAREST)
    seen_dead = seen_absent = 0
    for row, s, w in zip(g, sdf, weight):
        v = stored(model, row)
        if v is None:                                   # |g| = 64 lies in key 8, which the model does not hold
            assert np.isnan(s) and w == 0
            seen_absent += 1
        elif v[1] > 0:
            assert s.view(U) == v[0].view(U) and w == v[1]
        else:
            assert np.isnan(s) and w == 0
            seen_dead += 1
    assert seen_dead > 50 and seen_absent > 10


def test_rounding_follows_world2voxel():
    """(int)(u + copysign(0.5, u)), truncating: halves go away from zero, -0.0 to voxel 0."""
    model = {(0, 0, 0): (np.arange(512, dtype=F), np.ones(512, F)), (-1, 0, 0): (-np.arange(512, dtype=F) - 1, np.ones(512, F))}
    # one axis varies; voxelSize 1 makes u the coordinate itself
    # 0.5 - 2^-24 stays in voxel 0; 0.5 - 2^-25, the float below 0.5, does not: its sum with 0.5 rounds to 1.0 (ties to even)
    cases = {0.5: 1, -0.5: -1, 1.5: 2, -1.5: -2, 2.5: 3, -0.0: 0, 0.49999994: 0, -0.49999994: 0, 0.49999997: 1, -0.49999997: -1}
    for u, want in cases.items():
        sdf, _, _ = sr.sample(model, np.array([[u, 0, 0]], F), 1.0, sr.NEAREST)
        v = stored(model, (want, 0, 0))
        assert sdf[0] == v[0], (u, want, sdf[0])


def test_trilinear_on_a_lattice_point_is_corner_zero():
    model = mm.uniform_model(mm.cube_keys(0, 2), seed=43, dead=0.0)
    rng = np.random.RandomState(2)
    g = rng.randint(0, 15, (500, 3))
    sdf, weight, _ = sr.sample(model, (g.astype(F) * F(0.5)).astype(F), 0.5, sr.TRILINEAR)      # g * 0.5 / 0.5 = g exactly
    want = np.array([stored(model, row)[0] for row in g], F)
    assert np.array_equal(sdf.view(U), (want + F(0.0)).view(U))
    assert (weight == 1).all()


def test_affine_field_is_exact():
    a, b = (3, -2, 5), 7
    model = affine_model(mm.cube_keys(-2, 2), a, b)
    rng = np.random.RandomState(3)
    half = rng.randint(-16, 15, (2000, 3)) + 0.5                                  # half-lattice points, cells inside the blocks
    for vs in (0.5, 0.25):                                                        # powers of two: p / vs is exact
        p = (half * vs).astype(F)
        for mode in (sr.TRILINEAR,):
            sdf, weight, grad = sr.sample(model, p, vs, mode)
            assert np.array_equal(sdf, (half @ np.array(a) + b).astype(F))
            assert np.array_equal(grad, np.broadcast_to((np.array(a) / vs).astype(F), grad.shape))
            assert (weight == 1).all()
    # nearest: central differences of an affine field are exact too
    g = rng.randint(-15, 15, (500, 3))
    sdf, _, grad = sr.sample(model, (g * 0.5).astype(F), 0.5, sr.NEAREST)
    assert np.array_equal(sdf, (g @ np.array(a) + b).astype(F))
    assert np.array_equal(grad, np.broadcast_to((np.array(a) / 0.5).astype(F), grad.shape))


def test_nearest_gradient_is_the_mesh_gradient():
    """At the end voxels of every vertex of every_configuration(): what mesh_ref._gradient gives before the normalisation,
    divided by voxelSize; NaN where it reports no gradient."""
    model = mm.every_configuration()
    dense = mm.Dense(model)
    table, _, _, voxels = mm.place(model, 509, 8, len(model) + 3, seed=1)
    listed = np.nonzero(table["ptr"] != -1)[0]
    A, pos = mesh_ref._aprons(table, voxels, listed)
    block_row = {tuple(p): n for n, p in enumerate(pos.tolist())}
    v = dense.vertices()
    ends = np.unique(np.concatenate([v["a"], v["b"]]), axis=0)                     # dense (z, y, x)
    g = ends[:, ::-1] - 1 + dense.origin                                          # global (x, y, z)
    n = np.array([block_row[tuple(k)] for k in (g >> 3).tolist()])
    here = dense.sdf[tuple(ends.T)]
    want, ok = mesh_ref._gradient(A, n, g[:, 0] & 7, g[:, 1] & 7, g[:, 2] & 7, here)
    sdf, _, grad = sr.sample(model, (g.astype(F) * VS).astype(F), VS, sr.NEAREST)
    assert np.array_equal(sdf.view(U), here.view(U))
    assert np.array_equal(np.isnan(grad).any(1), ~ok)
    assert np.array_equal(grad[ok].view(U), (want[ok] / VS).astype(F).view(U))
    one_sided = dense.one_sided(ends)
    print(f"end voxels={len(g)} one-sided={one_sided.sum()} without a gradient={(~ok).sum()}")
    assert len(g) > 5000 and one_sided.sum() > 500


def test_floor_not_truncation_below_zero():
    model = mm.uniform_model(mm.cube_keys(-1, 1), seed=47, dead=0.0)
    rng = np.random.RandomState(4)
    u = rng.uniform(-0.999, -0.001, (200, 3)).astype(F)                            # corner 0 is voxel (-1, -1, -1), key (-1, -1, -1)
    sdf, _, _ = sr.sample(model, u, 1.0, sr.TRILINEAR)
    t = (u - F(-1)).astype(F)
    s = [stored(model, (-1 + (c & 1), -1 + ((c >> 1) & 1), -1 + (c >> 2)))[0] for c in range(8)]
    L = sr.lerp
    want = L(L(L(s[0], s[1], t[:, 0]), L(s[2], s[3], t[:, 0]), t[:, 1]), L(L(s[4], s[5], t[:, 0]), L(s[6], s[7], t[:, 0]), t[:, 1]), t[:, 2])
    assert np.array_equal(sdf.view(U), want.view(U)) and not np.isnan(sdf).any()
    only = {k: v for k, v in model.items() if k != (-1, -1, -1)}                   # without that block: nothing
    assert np.isnan(sr.sample(only, u, 1.0, sr.TRILINEAR)[0]).all()


def test_domain():
    model = mm.uniform_model(mm.cube_keys(-1, 1), seed=49, dead=0.0)
    edge = F(2.0 ** 30)
    below = np.nextafter(edge, F(0))
    for mode in (sr.NEAREST, sr.TRILINEAR):
        for bad in (np.nan, np.inf, -np.inf, edge, -edge):
            for axis in range(3):
                p = np.full((1, 3), 0.25, F)
                p[0, axis] = bad
                sdf, weight, grad = sr.sample(model, p, 1.0, mode)
                assert np.isnan(sdf[0]) and weight[0] == 0 and np.isnan(grad).all()
        for far in (below, -below):
            p = np.array([[far, 0.25, 0.25]], F)
            sdf, weight, grad = sr.sample(model, p, 1.0, mode)                     # looked up: the block is absent
            assert np.isnan(sdf[0]) and weight[0] == 0 and np.isnan(grad).all()
        # in metres: the same limits through the division
        p = np.array([[float(below) * 0.02, 0, 0], [3e7, 0, 0], [0.05, 0.05, 0.05]], F)
        sdf, _, _ = sr.sample(model, p, 0.02, mode)
        assert np.isnan(sdf[0]) and np.isnan(sdf[1]) and not np.isnan(sdf[2])


def test_lattice_is_the_stored_voxels():
    model = mm.holes(3)
    lo, dims = (-3 - 16, 5 + 24, -9 - 8), (13, 9, 20)
    sdf, weight = sr.lattice(model, lo, dims)
    assert sdf.shape == (20, 9, 13)
    seen = 0
    for k in range(dims[2]):
        for j in range(dims[1]):
            for i in range(0, dims[0], 3):
                v = stored(model, (lo[0] + i, lo[1] + j, lo[2] + k))
                if v is None or not v[1] > 0:
                    assert np.isnan(sdf[k, j, i]) and weight[k, j, i] == 0
                else:
                    assert sdf[k, j, i] == v[0] and weight[k, j, i] == v[1]
                    seen += 1
    assert seen > 100


def test_bulk_shares():
    """The shares the GPU bulk test asserts, from the model alone: (23/26)^3 * 0.98^8 and (24/26)^3 * 0.98."""
    model = mm.every_configuration()
    u = np.random.RandomState(7).uniform(-1, 25, (4096, 3))
    p = (u * 0.02).astype(F)
    tri = (~np.isnan(sr.sample(model, p, 0.02, sr.TRILINEAR)[0])).mean()
    near = (~np.isnan(sr.sample(model, p, 0.02, sr.NEAREST)[0])).mean()
    print(f"with a sample: trilinear {tri:.3f} nearest {near:.3f}")
    assert abs(tri - (23 / 26) ** 3 * 0.98 ** 8) < 0.04 and abs(near - (24 / 26) ** 3 * 0.98) < 0.04
