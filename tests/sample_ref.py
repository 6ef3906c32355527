"""The specification of vh_sample_sdf and vh_sample_lattice in vectorised numpy, float32 throughout (unfused multiply and add,
as the library is built), over a model dictionary as tests/mesh_models.py defines it: {block key (x, y, z): (sdf[512],
weight[512])}, voxel index ((z&7)<<6)|((y&7)<<3)|(x&7).  It does not import the product and knows nothing of a table.

Rule (include/voxelhash.h, "the model as a distance field"): voxel g sits at g * voxelSize; valid iff its block is in the
model, weight > 0 and sdf == sdf.  A point has u = p / voxelSize per axis and a sample only if |u| < 2^30 on every axis.  No
sample: sdf NaN, weight 0, gradient NaN.
  nearest: voxel (int)(u + copysign(0.5, u)), truncating; gradient per axis (s+ - s-) * 0.5, s+ - here or here - s- by which
    neighbours are valid, / voxelSize; an axis with neither: the whole gradient NaN.
  trilinear: f = floor(u), i = (int)f, t = u - f, corner c = voxel i + (c&1, c>>1&1, c>>2); a sample iff all eight are valid;
    lerp(a, b, t) = a + t * (b - a), x innermost, then y, then z; the gradient from the corner differences / voxelSize."""
import numpy as np

F = np.float32
NEAREST, TRILINEAR = 0, 1
DOMAIN = F(2.0 ** 30)


class Field:
    """The model's voxels by global integer coordinate."""

    def __init__(self, model):
        self.row = {tuple(int(c) for c in k): i for i, k in enumerate(model)}
        n = len(self.row)
        self.sdf = np.full((n + 1, 512), np.nan, F)                    # row n: the absent block
        self.weight = np.zeros((n + 1, 512), F)
        for i, (s, w) in enumerate(model.values()):
            self.sdf[i] = np.asarray(s, F)
            self.weight[i] = np.asarray(w, F)
        with np.errstate(invalid="ignore"):
            valid = (self.weight > 0) & (self.sdf == self.sdf)
        self.sdf = np.where(valid, self.sdf, F(np.nan)).astype(F)
        self.weight = np.where(valid, self.weight, F(0)).astype(F)

    def voxels(self, g):
        """(sdf, weight) of the voxels g [..., 3] (int64): NaN / 0 where a voxel is not valid."""
        g = np.asarray(g, np.int64)
        flat = g.reshape(-1, 3)
        keys, inverse = np.unique(flat >> 3, axis=0, return_inverse=True)        # floor division by 8
        rows = np.array([self.row.get(tuple(k), len(self.row)) for k in keys.tolist()], np.int64).reshape(-1)
        row = rows[inverse.reshape(-1)]
        index = ((flat[:, 2] & 7) << 6) | ((flat[:, 1] & 7) << 3) | (flat[:, 0] & 7)
        return self.sdf[row, index].reshape(g.shape[:-1]), self.weight[row, index].reshape(g.shape[:-1])


def lerp(a, b, t):
    return (a + (t * (b - a).astype(F)).astype(F)).astype(F)


def sample(model, points, voxel_size, mode=TRILINEAR):
    """points [n, 3] float32 world metres -> (sdf [n], weight [n], gradient [n, 3]), float32."""
    field = model if isinstance(model, Field) else Field(model)
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    vs = F(voxel_size)
    n = len(p)
    sdf, weight, grad = np.full(n, np.nan, F), np.zeros(n, F), np.full((n, 3), np.nan, F)
    with np.errstate(all="ignore"):
        u = (p / vs).astype(F)
        inside = (np.abs(u) < DOMAIN).all(1)                                     # False for NaN
        u = u[inside]
        if mode == NEAREST:
            r = np.trunc((u + np.copysign(F(0.5), u)).astype(F)).astype(np.int64)
            here, w = field.voxels(r)
            valid = here == here
            g = np.zeros((len(u), 3), F)
            ok = valid.copy()
            for a in range(3):
                d = np.zeros(3, np.int64)
                d[a] = 1
                sp, _ = field.voxels(r + d)
                sm, _ = field.voxels(r - d)
                hp, hm = sp == sp, sm == sm
                diff = np.where(hp & hm, ((sp - sm).astype(F) * F(0.5)).astype(F),
                                np.where(hp, (sp - here).astype(F), np.where(hm, (here - sm).astype(F), F(0)))).astype(F)
                g[:, a] = (diff / vs).astype(F)
                ok &= hp | hm
            g[~ok] = np.nan
            sdf[inside], weight[inside], grad[inside] = here, w, g
            return sdf, weight, grad
        assert mode == TRILINEAR
        f = np.floor(u).astype(F)
        i = f.astype(np.int64)
        t = (u - f).astype(F)
        tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
        s, w = [], []
        for c in range(8):
            sc, wc = field.voxels(i + np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64))
            s.append(sc)
            w.append(wc)
        all8 = np.all([sc == sc for sc in s], axis=0)

        def tri(v):
            return lerp(lerp(lerp(v[0], v[1], tx), lerp(v[2], v[3], tx), ty), lerp(lerp(v[4], v[5], tx), lerp(v[6], v[7], tx), ty), tz)
        d = lambda a, b: (s[a] - s[b]).astype(F)
        gx = (lerp(lerp(d(1, 0), d(3, 2), ty), lerp(d(5, 4), d(7, 6), ty), tz) / vs).astype(F)
        gy = (lerp(lerp(d(2, 0), d(3, 1), tx), lerp(d(6, 4), d(7, 5), tx), tz) / vs).astype(F)
        gz = (lerp(lerp(d(4, 0), d(5, 1), tx), lerp(d(6, 2), d(7, 3), tx), ty) / vs).astype(F)
        nan = F(np.nan)
        sdf[inside] = np.where(all8, tri(s), nan)
        weight[inside] = np.where(all8, tri(w), F(0))
        grad[inside] = np.where(all8[:, None], np.stack([gx, gy, gz], 1), nan)
    return sdf, weight, grad


def lattice(model, lo, dims):
    """(sdf, weight) [dims[2], dims[1], dims[0]]: voxel lo + (i, j, k) at [k, j, i]; NaN / 0 where not valid."""
    field = model if isinstance(model, Field) else Field(model)
    lo = np.asarray(lo, np.int64)
    k, j, i = np.meshgrid(*(np.arange(int(d), dtype=np.int64) for d in (dims[2], dims[1], dims[0])), indexing="ij")
    g = np.stack([i, j, k], -1) + lo
    if g.size == 0:
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        return np.zeros(shape, F), np.zeros(shape, F)
    return field.voxels(g)


def same_bits(a, b):
    """Bit for bit, two NaNs counting as equal."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
