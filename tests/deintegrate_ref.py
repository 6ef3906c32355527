"""The rule of vh_deintegrate (include/voxelhash.h, "taking a frame back out") in executable form: numpy float32, every
multiply and add rounded on its own, in the order the header writes them.

apply_frame(..., sign=+1) is the TSDF update of integrateDepthMap restated (tests/test_deintegrate_ref_cpu.py pins it to the
oracle bit for bit on the golden scenes, tests/test_tsdf_cases_cpu.py on crafted depth and stored voxels, non-finite ones
included); sign=-1 takes the same frame's samples out again.  visible_entries() is the block set: the allocated
entries that pass blockInFrustum, in table order -- vh_set_pose + vh_flatten.
"""
import numpy as np

F = np.float32
SEM_REFERENCE, SEM_PINHOLE = 0, 1
FLAG_DEPTH_TRUNCATION, FLAG_WEIGHT_SAMPLE = 1, 2          # the oracle's integrate flags
DEPTH_UNIT = F(5000.0)                                     # uint16 sensor units per metre


def f2i_rz(x):
    """float32 -> int32 as v_cvt_i32_f32: truncate towards zero, saturate, NaN -> 0."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x.astype(np.float64))
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, -2147483648.0, 2147483647.0).astype(np.int64).astype(np.int32)


def _mat4_rows(m, x, y, z):
    """Rows 0..2 of float4x4 * (x, y, z, 1), summed left to right."""
    m = np.asarray(m, F).reshape(16)
    one = F(1.0)
    return [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] * one for r in range(3)]


def _project(proj, cx, cy, cz):
    p = np.asarray(proj, F).reshape(9)
    qx = (p[0] * cx + p[1] * cy) + p[2] * cz
    qy = (p[3] * cx + p[4] * cy) + p[5] * cz
    qz = (p[6] * cx + p[7] * cy) + p[8] * cz
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return f2i_rz(qx / qz), f2i_rz(qy / qz)


def _wrap_i32(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def visible_entries(table, params, semantics, proj, pose, pose_inv, width, height):
    """Indices into `table` (a VoxelEntry array) of the allocated entries that pass blockInFrustum, in table order."""
    idx = np.nonzero(table["ptr"] != -1)[0]
    pos = table["pos"][idx]
    vs = F(params.voxelSize)
    w = [_wrap_i32(pos[:, a].astype(np.int64) * 8).astype(F) * vs for a in range(3)]        # block2World
    if semantics == SEM_REFERENCE:
        cx, cy, cz = _mat4_rows(pose, *w)
        front = np.ones(len(idx), bool)
    else:
        cx, cy, cz = _mat4_rows(pose_inv, *w)
        front = cz > F(0.0)
    sx, sy = _project(proj, cx, cy, cz)
    ok = front & (sx < width) & (sx >= 0) & (sy < height) & (sy >= 0)
    return idx[ok]


def _depth_at(depth_source, sx, sy):
    """Camera z of pixels (sx, sy), all inside the image: a float32 plane [H, W] (the .z of a vertex map), or
    (uint16 image [H, W], k_inv) with the sensor arithmetic z = (k6 * x + k7 * y + k8 * 1) * (d / 5000)."""
    if isinstance(depth_source, tuple):
        image, k_inv = depth_source
        k = np.asarray(k_inv, F).reshape(9)
        d = np.asarray(image, np.uint16)[sy, sx].astype(F) / DEPTH_UNIT
        pz = (k[6] * sx.astype(F) + k[7] * sy.astype(F)) + k[8] * F(1.0)
        return pz * d
    return np.asarray(depth_source, F)[sy, sx]


def frame_samples(entries, params, semantics, proj, pose_inv, depth_source, flags):
    """(valid [n, 512] bool, s [n, 512], cw [n, 512]) for the blocks `entries`, voxels in the block's linear order
    z * 64 + y * 8 + x: what the TSDF update would combine into each voxel, valid where it would not return early."""
    plane = depth_source[0] if isinstance(depth_source, tuple) else depth_source
    height, width = np.asarray(plane).shape[:2]
    n = len(entries)
    lin = np.arange(512)
    tx, ty, tz = lin & 7, (lin >> 3) & 7, lin >> 6
    base = _wrap_i32(entries["pos"].astype(np.int64) * 8).reshape(n, 3)
    vx = _wrap_i32(base[:, 0:1].astype(np.int64) + tx[None, :])
    vy = _wrap_i32(base[:, 1:2].astype(np.int64) + ty[None, :])
    vz = _wrap_i32(base[:, 2:3].astype(np.int64) + tz[None, :])
    vs = F(params.voxelSize)
    if semantics == SEM_REFERENCE:
        r = _mat4_rows(pose_inv, vx.astype(F), vy.astype(F), vz.astype(F))
        cx, cy, cz = [f2i_rz(c).astype(F) * vs for c in r]
    else:
        cx, cy, cz = _mat4_rows(pose_inv, vx.astype(F) * vs, vy.astype(F) * vs, vz.astype(F) * vs)
    sx, sy = _project(proj, cx, cy, cz)
    ok = (sx >= 0) & (sx < width) & (sy >= 0) & (sy < height)
    depth = _depth_at(depth_source, np.where(ok, sx, 0), np.where(ok, sy, 0))
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= ~(depth <= F(0.0))
        s = depth - cz
        trunc = np.full(s.shape, F(params.truncation), F)
        if flags & FLAG_DEPTH_TRUNCATION:
            trunc = F(params.truncation) + (F(params.truncScale) * depth)
        ok &= s > -trunc
        s = np.where(s >= F(0.0), np.minimum(trunc, s), np.maximum(-trunc, s)).astype(F)
        cw = np.full(s.shape, F(0.1), F)
        if flags & FLAG_WEIGHT_SAMPLE:
            zero_one = (depth - F(0.5)) / (F(5.0) - F(0.5))
            wd = float(params.integrationWeightSample) * 1.5 * (1.0 - zero_one.astype(np.float64))
            cw = np.maximum(wd.astype(F), F(1.0))
    return ok, s, cw


def apply_frame(voxels, entries, params, semantics, proj, pose_inv, pose, depth_source, flags, sign):
    """A copy of `voxels` (the whole volume, VOXEL_DTYPE) after one frame went through the blocks `entries` (VoxelEntry
    records with their ptr; the compact set of `pose`, see visible_entries): sign=+1 the TSDF update, sign=-1 its removal.
    pose_inv: the library's inverse of `pose` (cofactor form; oracle.invert4x4).  Returns (voxels, stats) with the counts
    of voxels untouched / reset to zero / partially removed (sign=-1) or updated (sign=+1) over the listed blocks."""
    out = voxels.copy()
    n = len(entries)
    if n == 0:
        return out, dict(untouched=0, reset=0, partial=0, updated=0)
    ok, s, cw = frame_samples(entries, params, semantics, proj, pose_inv, depth_source, flags)
    at = entries["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
    os_, ow = out["sdf"][at], out["weight"][at]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if sign > 0:
            nsdf = ((os_ * ow) + (s * cw)) / (ow + cw)
            nw = np.fmin(F(params.integrationWeightMax), ow + cw)         # fminf: a stored NaN weight becomes the cap
            change = ok
            stats = dict(untouched=int((~ok).sum()), reset=0, partial=0, updated=int(ok.sum()))
        else:
            change = ok & (ow > F(0.0))
            floor = F(0.5) if flags & FLAG_WEIGHT_SAMPLE else F(0.05)
            nw = ow - cw
            gone = change & ~(nw >= floor)
            nsdf = ((os_ * ow) - (s * cw)) / nw
            nsdf = np.where(gone, F(0.0), nsdf)
            nw = np.where(gone, F(0.0), nw)
            stats = dict(untouched=int((~change).sum()), reset=int(gone.sum()), partial=int((change & ~gone).sum()), updated=0)
    sdf, wgt = out["sdf"], out["weight"]
    sdf[at[change]] = nsdf.astype(F)[change]
    wgt[at[change]] = nw.astype(F)[change]
    return out, stats
