"""The rules of vh_merge_color and vh_deintegrate_color (include/voxelhash.h, "colour through merging, de-integration and saved
models") in executable form: numpy, float32 with every operation rounded on its own, in the order the header writes them.  It
does not import the product.

Merging is built on merge_ref.samples / merge_ref.apply (the geometry, unchanged) and on color_ref.ColorField (the corner
words), over model dictionaries {block key: (sdf[512], weight[512], colour[512])}.  The removal is color_ref.integrate's frame
walk with the sample taken back out of the running average."""
import numpy as np

import color_ref as CR
import merge_ref as R
import sample_ref as S

F = np.float32
U = np.uint32
NEAREST, TRILINEAR = S.NEAREST, S.TRILINEAR


def geometry(model):
    return {k: (v[0], v[1]) for k, v in model.items()}


def color_samples(src_model, keys, Tinv, vs_s, vs_d, mode=TRILINEAR, where=None):
    """(rgb, count) [len(keys), 512] uint32 that the voxels of the dst blocks `keys` see of src's colour at the point the TSDF
    sample is taken: count 0 where there is none.  (Whether the TSDF sample exists is merge_ref.samples' business; `where`
    [len(keys), 512] bool limits the work to the voxels the caller will look at, the others read 0.)"""
    field = src_model if isinstance(src_model, CR.ColorField) else CR.ColorField(src_model)
    keys = np.asarray(list(keys), np.int64).reshape(-1, 3)
    g = (keys[:, None, :] * 8 + R.LOCAL[None, :, :]).reshape(-1, 3)
    p = [(g[:, a].astype(F) * F(vs_d)).astype(F) for a in range(3)]
    q = np.stack(R.rows(Tinv, *p), 1)
    n = len(q)
    rgb, cnt = np.zeros(n, U), np.zeros(n, U)
    with np.errstate(all="ignore"):
        u = (q / F(vs_s)).astype(F)
        inside = (np.abs(u) < S.DOMAIN).all(1)
        if where is not None:
            inside &= np.asarray(where, bool).reshape(-1)
        u = u[inside]
        if mode == NEAREST:
            r = np.trunc((u + np.copysign(F(0.5), u)).astype(F)).astype(np.int64)
            word = field.words(r)
            rgb[inside], cnt[inside] = word & U(0xFFFFFF), CR.count(word)
        else:
            f = np.floor(u).astype(F)
            i = f.astype(np.int64)
            t = (u - f).astype(F)
            tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
            words = [field.words(i + np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64)) for c in range(8)]
            least = np.min([CR.count(wc) for wc in words], axis=0).astype(U)
            out = np.zeros(len(u), U)
            for k in (0, 8, 16):
                v = [((wc >> U(k)) & U(255)).astype(F) for wc in words]
                fk = S.lerp(S.lerp(S.lerp(v[0], v[1], tx), S.lerp(v[2], v[3], tx), ty),
                            S.lerp(S.lerp(v[4], v[5], tx), S.lerp(v[6], v[7], tx), ty), tz)
                out |= (fk + F(0.5)).astype(F).astype(U) << U(k)
            rgb[inside], cnt[inside] = np.where(least > 0, out, U(0)), least
    return rgb.reshape(-1, 512), cnt.reshape(-1, 512)


def combine(word, rgb, w_s, weight_max):
    """dst's words after the colour step with the samples (rgb, w_s), w_s > 0 everywhere."""
    word, rgb, w_s = np.asarray(word, U), np.asarray(rgb, U), np.asarray(w_s, U)
    w_d = CR.count(word)
    cap = U(weight_max)
    fresh = rgb | (np.minimum(w_s, cap) << U(24))
    fd, fs, den = w_d.astype(F), w_s.astype(F), (w_d + w_s).astype(F)
    mixed = np.minimum(w_d + w_s, cap) << U(24)
    with np.errstate(all="ignore"):
        for k, old, new in zip((0, 8, 16), CR.channels(word), CR.channels(rgb)):
            f = (((old.astype(F) * fd).astype(F) + (new.astype(F) * fs).astype(F)).astype(F) / den).astype(F)
            mixed = mixed | ((f + F(0.5)).astype(F).astype(U) << U(k))
    return np.where(w_d == 0, fresh, mixed).astype(U)


def apply(dst_model, src_model, keys, Tinv, vs_s, vs_d, trunc, wmax, mode=TRILINEAR, weight_max=255, merged=None):
    """dst_model (with colour; a block the allocation has just made is in it as zeros) after vh_merge_color's update over `keys`:
    (model, geometry stats of merge_ref.apply, colour stats).  The colour stats count voxels by branch: fresh (dst had no
    colour), combined, capped (the count was cut to weight_max), no_sample (the TSDF step happened, no colour sample), kept (dst
    words != 0 that the call leaves as they were).
    merged: the geometry after the update, {key: (sdf, weight)}, where the caller holds it already (a twin that received
    vh_merge, itself checked against merge_ref.apply elsewhere); merge_ref.apply is then not run and its stats are None."""
    keys = [tuple(int(c) for c in k) for k in keys if tuple(int(c) for c in k) in dst_model]
    if merged is None:
        geo, gstats = R.apply(geometry(dst_model), geometry(src_model), keys, Tinv, vs_s, vs_d, trunc, wmax, mode)
    else:
        geo, gstats = merged, None
    out = {k: (geo[k][0], geo[k][1], np.array(dst_model[k][2], U)) for k in dst_model}
    cstats = dict(fresh=0, combined=0, capped=0, no_sample=0, kept=0)
    touched = set(keys)
    if keys:
        s, w = R.samples(geometry(src_model), keys, Tinv, vs_s, vs_d, mode)
        with np.errstate(invalid="ignore"):
            rgb, cnt = color_samples(src_model, keys, Tinv, vs_s, vs_d, mode, where=(s == s) & (w > 0))
        for i, k in enumerate(keys):
            with np.errstate(invalid="ignore"):
                take = (s[i] == s[i]) & (w[i] > 0)
            step = take & (cnt[i] > 0)
            c = out[k][2]
            w_d = CR.count(c)
            new = np.where(step, combine(c, rgb[i], np.maximum(cnt[i], U(1)), weight_max), c).astype(U)
            cstats["fresh"] += int((step & (w_d == 0)).sum())
            cstats["combined"] += int((step & (w_d > 0)).sum())
            cstats["capped"] += int((step & (w_d + cnt[i] > U(weight_max))).sum())
            cstats["no_sample"] += int((take & ~step).sum())
            cstats["kept"] += int((~step & (c != 0)).sum())
            out[k] = (out[k][0], out[k][1], new)
    cstats["kept"] += sum(int((np.asarray(v[2], U) != 0).sum()) for k, v in dst_model.items() if k not in touched)
    return out, gstats, cstats


# ---- taking a frame's colour back out ----------------------------------------------------------------------------------------
def unblend(word, pixel):
    """The words `word` (count >= 1 each) with one sample `pixel` each taken back out."""
    word, pixel = np.asarray(word, U), np.asarray(pixel, U)
    w = CR.count(word)
    fw, den = w.astype(F), (w - U(1)).astype(F)
    out = (w - U(1)) << U(24)
    with np.errstate(all="ignore"):
        for k, old, new in zip((0, 8, 16), CR.channels(word), CR.channels(pixel)):
            f = (((old.astype(F) * fw).astype(F) - new.astype(F)).astype(F) / den).astype(F)
            f = np.minimum(np.maximum(f, F(0.0)), F(255.0)).astype(F)
            f = np.where(w > 1, f, F(0.0)).astype(F)                        # (w == 1: 0 / 0 above; the word becomes 0 below)
            out = out | ((f + F(0.5)).astype(F).astype(U) << U(k))
    return np.where(w == 1, U(0), out).astype(U)


def deintegrate(color, voxels, entries, params, semantics, proj, pose_inv, depth_source, rgba, band):
    """A copy of the colour volume after vh_deintegrate_color over the blocks `entries`; `voxels` is the TSDF volume as it is at
    the call.  Returns (color, stats): swept (words of voxels that hold nothing), removed (count went down), emptied (w == 1),
    clamped (a channel left [0, 255] before the clamp)."""
    out = np.array(color, U, copy=True)
    n = len(entries)
    stats = dict(swept=0, removed=0, emptied=0, clamped=0)
    if n == 0:
        return out, stats
    at = entries["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
    holds = voxels["weight"][at] > F(0.0)
    ok, s, sx, sy = CR.surface_samples(entries, params, semantics, proj, pose_inv, depth_source)
    with np.errstate(invalid="ignore"):
        near = ok & (np.abs(s) <= F(band))
    word = out[at]
    take = holds & near & (CR.count(word) > 0)
    new = word.copy()
    new[~holds] = 0
    if take.any():
        pixel = np.asarray(rgba, U)[sy[take], sx[take]]
        new[take] = unblend(word[take], pixel)
        stats["clamped"] = clamped(word[take], pixel)
    out[at] = new
    stats.update(swept=int(((word != 0) & ~holds).sum()), removed=int(take.sum()), emptied=int((take & (CR.count(word) == 1)).sum()))
    return out, stats


def clamped(word, pixel):
    """How many channels of the removal leave [0, 255] before the clamp (w >= 2)."""
    word, pixel = np.asarray(word, U), np.asarray(pixel, U)
    w = CR.count(word)
    many = w > 1
    n = 0
    with np.errstate(all="ignore"):
        for old, new in zip(CR.channels(word), CR.channels(pixel)):
            f = (((old.astype(F) * w.astype(F)).astype(F) - new.astype(F)).astype(F) / (w - U(1)).astype(F)).astype(F)
            n += int((many & ((f < 0) | (f > 255))).sum())
    return n
