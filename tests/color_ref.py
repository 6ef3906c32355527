"""The rule of the colour calls (include/voxelhash.h, "the model in colour") in executable form: numpy, float32 with every
operation rounded on its own, in the order the header writes them.  It does not import the product.

Fusing: integrate() applies one frame's colour image to a colour volume (uint32 per voxel, r | g << 8 | b << 16 | w << 24, the
word 0 = no colour) over the blocks `entries`, the compact set of the pose (deintegrate_ref.visible_entries).  The camera
point, projection, bounds test and depth read are the TSDF update's, taken from tests/deintegrate_ref.py.
Reading: sample() / sample_map() over a model dictionary {block key: (sdf[512], weight[512], colour[512])}, with the domain,
voxel choice and validity of tests/sample_ref.py."""
import numpy as np

import deintegrate_ref as D
import sample_ref as S

F = np.float32
U = np.uint32
NEAREST, TRILINEAR = S.NEAREST, S.TRILINEAR


def pack(r, g, b, w=255):
    return (np.asarray(r, U) | (np.asarray(g, U) << U(8)) | (np.asarray(b, U) << U(16)) | (np.asarray(w, U) << U(24))).astype(U)


def channels(word):
    word = np.asarray(word, U)
    return [(word >> U(k)) & U(255) for k in (0, 8, 16)]


def count(word):
    return np.asarray(word, U) >> U(24)


def surface_samples(entries, params, semantics, proj, pose_inv, depth_source):
    """(ok [n, 512] bool, s [n, 512], sx, sy) for the blocks `entries`, voxels in the block's linear order: s = depth - cz
    where the voxel projects into the image onto a pixel with depth > 0 (the update's steps up to its line :813)."""
    plane = depth_source[0] if isinstance(depth_source, tuple) else depth_source
    height, width = np.asarray(plane).shape[:2]
    n = len(entries)
    lin = np.arange(512)
    tx, ty, tz = lin & 7, (lin >> 3) & 7, lin >> 6
    base = D._wrap_i32(entries["pos"].astype(np.int64) * 8).reshape(n, 3)
    vx = D._wrap_i32(base[:, 0:1].astype(np.int64) + tx[None, :])
    vy = D._wrap_i32(base[:, 1:2].astype(np.int64) + ty[None, :])
    vz = D._wrap_i32(base[:, 2:3].astype(np.int64) + tz[None, :])
    vs = F(params.voxelSize)
    if semantics == D.SEM_REFERENCE:
        r = D._mat4_rows(pose_inv, vx.astype(F), vy.astype(F), vz.astype(F))
        cx, cy, cz = [D.f2i_rz(c).astype(F) * vs for c in r]
    else:
        cx, cy, cz = D._mat4_rows(pose_inv, vx.astype(F) * vs, vy.astype(F) * vs, vz.astype(F) * vs)
    sx, sy = D._project(proj, cx, cy, cz)
    ok = (sx >= 0) & (sx < width) & (sy >= 0) & (sy < height)
    sx, sy = np.where(ok, sx, 0), np.where(ok, sy, 0)
    depth = D._depth_at(depth_source, sx, sy)
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= ~(depth <= F(0.0))
        s = (depth - cz).astype(F)
    return ok, s, sx, sy


def blend(word, pixel, weight_max):
    """Steps 6 and 7: the words `word` after one sample `pixel` each (weight_max >= 1)."""
    word, pixel = np.asarray(word, U), np.asarray(pixel, U)
    w = count(word)
    fw, den = w.astype(F), (w + U(1)).astype(F)
    out = np.minimum(w + U(1), U(weight_max)) << U(24)
    for k, old, new in zip((0, 8, 16), channels(word), channels(pixel)):
        f = ((old.astype(F) * fw).astype(F) + new.astype(F)).astype(F) / den
        out = out | ((f.astype(F) + F(0.5)).astype(F).astype(U) << U(k))
    return out.astype(U)


def integrate(color, voxels, entries, params, semantics, proj, pose_inv, depth_source, rgba, band, weight_max):
    """A copy of the colour volume `color` after vh_integrate_color over the blocks `entries` (VoxelEntry records with their
    ptr); `voxels` is the TSDF volume as it is at the call.  rgba: uint32 [H, W].  Returns (color, stats)."""
    out = np.array(color, U, copy=True)
    n = len(entries)
    stats = dict(swept=0, rejected=0, sampled=0)
    if n == 0:
        return out, stats
    at = entries["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
    holds = voxels["weight"][at] > F(0.0)
    ok, s, sx, sy = surface_samples(entries, params, semantics, proj, pose_inv, depth_source)
    with np.errstate(invalid="ignore"):
        near = ok & (np.abs(s) <= F(band))
    take = holds & near & (weight_max != 0)
    word = out[at]
    new = word.copy()
    new[~holds] = 0
    if take.any():
        new[take] = blend(word[take], np.asarray(rgba, U)[sy[take], sx[take]], weight_max)
    out[at] = new
    stats.update(swept=int(((word != 0) & ~holds).sum()), rejected=int((holds & ~near).sum()), sampled=int(take.sum()))
    return out, stats


class ColorField(S.Field):
    """The model's voxels and colour words by global integer coordinate: model = {key: (sdf[512], weight[512], colour[512])}."""

    def __init__(self, model):
        super().__init__({k: (v[0], v[1]) for k, v in model.items()})
        self.color = np.zeros((len(self.row) + 1, 512), U)                  # row n: the absent block
        for i, v in enumerate(model.values()):
            self.color[i] = np.asarray(v[2], U)
        self.color[~(self.sdf == self.sdf)] = 0                             # a voxel that is not valid shows no colour

    def words(self, g):
        g = np.asarray(g, np.int64)
        flat = g.reshape(-1, 3)
        keys, inverse = np.unique(flat >> 3, axis=0, return_inverse=True)
        rows = np.array([self.row.get(tuple(k), len(self.row)) for k in keys.tolist()], np.int64).reshape(-1)
        row = rows[inverse.reshape(-1)]
        index = ((flat[:, 2] & 7) << 6) | ((flat[:, 1] & 7) << 3) | (flat[:, 0] & 7)
        return self.color[row, index].reshape(g.shape[:-1])


def sample(model, points, voxel_size, mode=TRILINEAR):
    """points [n, 3] float32 world metres -> uint32 [n]: r | g << 8 | b << 16 | 0xFF << 24, or 0 where there is no colour."""
    field = model if isinstance(model, ColorField) else ColorField(model)
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    vs = F(voxel_size)
    out = np.zeros(len(p), U)
    with np.errstate(all="ignore"):
        u = (p / vs).astype(F)
        inside = (np.abs(u) < S.DOMAIN).all(1)                              # False for NaN
        u = u[inside]
        if mode == NEAREST:
            r = np.trunc((u + np.copysign(F(0.5), u)).astype(F)).astype(np.int64)
            word = field.words(r)
            out[inside] = np.where(count(word) > 0, (word & U(0xFFFFFF)) | U(0xFF000000), U(0))
            return out
        assert mode == TRILINEAR
        f = np.floor(u).astype(F)
        i = f.astype(np.int64)
        t = (u - f).astype(F)
        tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
        words = [field.words(i + np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64)) for c in range(8)]
        all8 = np.all([count(wc) > 0 for wc in words], axis=0)             # (an invalid voxel's word is 0 here)
        rgb = np.full(len(u), 0xFF000000, U)
        for k in (0, 8, 16):
            v = [((wc >> U(k)) & U(255)).astype(F) for wc in words]
            fk = S.lerp(S.lerp(S.lerp(v[0], v[1], tx), S.lerp(v[2], v[3], tx), ty),
                        S.lerp(S.lerp(v[4], v[5], tx), S.lerp(v[6], v[7], tx), ty), tz)
            rgb |= (fk + F(0.5)).astype(F).astype(U) << U(k)
        out[inside] = np.where(all8, rgb, U(0))
    return out


def to_world(pose, points4):
    """Camera-frame float4 points -> (q [n, 3] float32, has [n]): q_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3];
    a point with .z == 0 has none (its q is NaN here, which no sample accepts)."""
    T = np.asarray(pose, F).reshape(4, 4)
    p = np.ascontiguousarray(points4, F).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        q = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(F)
    has = z != F(0.0)
    q[~has] = np.nan
    return q, has


def sample_map(model, pose, points4, voxel_size, mode=TRILINEAR):
    q, _ = to_world(pose, points4)
    return sample(model, q, voxel_size, mode)
