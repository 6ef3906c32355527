"""The specification of vh_merge in vectorised numpy, float32 throughout (unfused multiply and add, as the library is built), over
model dictionaries as tests/mesh_models.py defines them: {block key (x, y, z): (sdf[512], weight[512])}, voxel index
((z&7)<<6)|((y&7)<<3)|(x&7).  It is built on sample_ref.sample / sample_ref.Field, does not import the product and knows
nothing of a table.

Rule (include/voxelhash.h, "one model into another"):
  candidates  the box [8k - 0.5, 8k + 8] of src block k in src voxels, its eight corners times vs_s, through T (rows summed
              left to right), over vs_d; per axis gmin = (int)ceil(min), gmax = (int)ceil(max) - 1, all block keys
              gmin >> 3 .. gmax >> 3.  A block with a corner coordinate failing |u| < 2^30 is skipped.
  update      dst voxel g: p = (float)g * vs_d, q = Tinv . p, (s, w) = the sample of SRC at q (sample_ref); no sample or
              !(w > 0): untouched; s clamped to +-trunc; !(ow > 0): {s, min(wmax, w)}; else
              sdf = ((os * ow) + (s * w)) / (ow + w), weight = min(wmax, ow + w)."""
import numpy as np

import sample_ref as S

F = np.float32
NEAREST, TRILINEAR = S.NEAREST, S.TRILINEAR
DOMAIN = S.DOMAIN


def rows(M, x, y, z):
    """Rows 0..2 of the 4x4 M applied to (x, y, z, 1): ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3], float32."""
    M = np.asarray(M, F).reshape(4, 4)
    return [((((M[r, 0] * x).astype(F) + (M[r, 1] * y).astype(F)).astype(F) + (M[r, 2] * z).astype(F)).astype(F) + M[r, 3]).astype(F)
            for r in range(3)]


def boxes(src_keys, T, vs_s, vs_d):
    """Per src block: (ok [N] bool, first key [N, 3], keys per axis [N, 3]) of its candidate range."""
    k = np.asarray(list(src_keys), np.int64).reshape(-1, 3)
    vs_s, vs_d = F(vs_s), F(vs_d)
    low = ((k * 8).astype(F) - F(0.5)).astype(F)
    high = (k * 8 + 8).astype(F)
    ok = np.ones(len(k), bool)
    lo = np.full((len(k), 3), np.inf, F)
    hi = np.full((len(k), 3), -np.inf, F)
    with np.errstate(all="ignore"):
        for c in range(8):
            e = [np.where((c >> a) & 1, high[:, a], low[:, a]).astype(F) for a in range(3)]
            q = rows(T, *[(e[a] * vs_s).astype(F) for a in range(3)])
            for r in range(3):
                u = (q[r] / vs_d).astype(F)
                ok &= np.abs(u) < DOMAIN                                 # False for NaN
                lo[:, r] = np.minimum(lo[:, r], u)
                hi[:, r] = np.maximum(hi[:, r], u)
    lo, hi = np.where(ok[:, None], lo, F(0)), np.where(ok[:, None], hi, F(0))
    gmin = np.ceil(lo).astype(np.int64)
    gmax = np.ceil(hi).astype(np.int64) - 1
    first = gmin >> 3
    count = np.maximum(0, (gmax >> 3) - first + 1)
    count[~ok] = 0
    return ok, first, count


def candidates(src_keys, T, vs_s, vs_d):
    """(the candidate key set, the record count with multiplicity)."""
    ok, first, count = boxes(src_keys, T, vs_s, vs_d)
    keys, records = set(), 0
    for f, n in zip(first.tolist(), count.tolist()):
        records += n[0] * n[1] * n[2]
        for z in range(n[2]):
            for y in range(n[1]):
                for x in range(n[0]):
                    keys.add((f[0] + x, f[1] + y, f[2] + z))
    return keys, records


def multiplicity(src_keys, T, vs_s, vs_d):
    """{candidate key: how many records name it}."""
    _, first, count = boxes(src_keys, T, vs_s, vs_d)
    out = {}
    for f, n in zip(first.tolist(), count.tolist()):
        for z in range(n[2]):
            for y in range(n[1]):
                for x in range(n[0]):
                    k = (f[0] + x, f[1] + y, f[2] + z)
                    out[k] = out.get(k, 0) + 1
    return out


def skipped(src_keys, T, vs_s, vs_d):
    """src blocks outside the domain."""
    return int((~boxes(src_keys, T, vs_s, vs_d)[0]).sum())


_I = np.arange(512)
LOCAL = np.stack([_I & 7, (_I >> 3) & 7, _I >> 6], 1).astype(np.int64)


def samples(src_model, keys, Tinv, vs_s, vs_d, mode=TRILINEAR):
    """(s, w) [len(keys), 512] that the voxels of the dst blocks `keys` see of src: NaN / 0 where there is none."""
    keys = np.asarray(list(keys), np.int64).reshape(-1, 3)
    g = (keys[:, None, :] * 8 + LOCAL[None, :, :]).reshape(-1, 3)
    p = [(g[:, a].astype(F) * F(vs_d)).astype(F) for a in range(3)]
    q = np.stack(rows(Tinv, *p), 1)
    s, w, _ = S.sample(src_model, q, vs_s, mode)
    return s.reshape(-1, 512), w.reshape(-1, 512)


def apply(dst_model, src_model, keys, Tinv, vs_s, vs_d, trunc, wmax, mode=TRILINEAR):
    """dst_model after the update over `keys` (those of them that dst_model holds; a block the allocation has just made is in
    dst_model as zeros): (model, stats).  stats counts voxels by branch, and the updated blocks left without any weight."""
    keys = [tuple(int(c) for c in k) for k in keys if tuple(int(c) for c in k) in dst_model]
    out = {k: (np.array(v[0], F), np.array(v[1], F)) for k, v in dst_model.items()}
    stats = dict(blocks=len(keys), untouched=0, fresh=0, combined=0, capped=0, empty_blocks=0)
    if not keys:
        return out, stats
    trunc, wmax = F(trunc), F(wmax)
    s, w = samples(src_model, keys, Tinv, vs_s, vs_d, mode)
    with np.errstate(all="ignore"):
        for i, k in enumerate(keys):
            os_, ow = out[k]
            si, wi = s[i], w[i]
            take = (si == si) & (wi > 0)
            sc = np.where(si >= 0, np.minimum(trunc, si), np.maximum(-trunc, si)).astype(F)
            fresh = take & ~(ow > 0)
            comb = take & (ow > 0)
            wsum = (ow + wi).astype(F)
            mixed = ((((os_ * ow).astype(F) + (sc * wi).astype(F)).astype(F)) / wsum).astype(F)
            new_s = np.where(fresh, sc, np.where(comb, mixed, os_)).astype(F)
            new_w = np.where(fresh, np.minimum(wmax, wi), np.where(comb, np.minimum(wmax, wsum), ow)).astype(F)
            stats["untouched"] += int((~take).sum())
            stats["fresh"] += int(fresh.sum())
            stats["combined"] += int(comb.sum())
            stats["capped"] += int((fresh & (wi > wmax)).sum() + (comb & (wsum > wmax)).sum())
            stats["empty_blocks"] += int(not (new_w > 0).any() and (new_w == 0).all())
            out[k] = (new_s, new_w)
    return out, stats
