"""The colour arithmetic (include/voxelhash.h: step 6 and 7 of FUSING, the colour step of MERGING, TAKING A FRAME'S COLOUR BACK
OUT) a second time, in integers: numpy int64, no float anywhere, every channel (2 * num + den) // (2 * den), which is num / den
rounded half up.  It imports neither the product nor tests/color_ref.py / tests/merge_color_ref.py: tests/
test_color_count_ref_cpu.py holds those float32 forms to this one over every input, and tests/test_gpu_color_counts.py holds the
kernels to both.

The result of each rule depends on its inputs only through the count(s) and the numerator, so what a test must cover is stated
in (count, num) pairs -- the enumerators below: the exact ties (2 * num mod 2 * den == den, where a rounding that is a hair off
falls the other way) and the pairs on which a division done as a multiplication by the float32 reciprocal, num * (1 / den),
gives another byte than the rule (rcp_discriminators_*: the only function here that touches float32, as the thing to tell apart
from)."""
import functools

import numpy as np

I = np.int64
F = np.float32
U = np.uint32


def _parts(word):
    word = np.asarray(word).astype(I)
    return [(word >> k) & 255 for k in (0, 8, 16)], (word >> 24) & 255


def _round_half_up(num, den):
    return (2 * num + den) // (2 * den)


def _word(chans, count):
    return (chans[0] | (chans[1] << 8) | (chans[2] << 16) | (count << 24)).astype(U)


def blend_exact(word, pixel, weight_max):
    """The words after one sample `pixel` each: num = old * w + new over den = w + 1; the count min(w + 1, weight_max)."""
    old, w = _parts(word)
    new, _ = _parts(pixel)
    den = w + 1
    return _word([_round_half_up(o * w + n, den) for o, n in zip(old, new)], np.minimum(w + 1, I(weight_max)))


def unblend_exact(word, pixel):
    """The words with one sample `pixel` each taken back out: num = old * w - new clamped to [0, 255 * den], den = w - 1; the
    count w - 1; a word of count 1 becomes 0 whole; a word of count 0 has nothing to take out and stays."""
    old, w = _parts(word)
    new, _ = _parts(pixel)
    den = np.maximum(w - 1, 1)
    out = _word([_round_half_up(np.clip(o * w - n, 0, 255 * den), den) for o, n in zip(old, new)], w - 1)
    return np.where(w == 0, np.asarray(word).astype(U), np.where(w == 1, U(0), out)).astype(U)


def combine_exact(word, rgb, w_s, weight_max):
    """dst's words after the colour step with the samples (rgb, w_s), w_s > 0: num = old * wd + new * ws over den = wd + ws, the
    count min(wd + ws, weight_max); a word of count 0 becomes rgb | min(ws, weight_max) << 24."""
    old, wd = _parts(word)
    new, _ = _parts(rgb)
    ws = np.asarray(w_s).astype(I)
    cap = I(weight_max)
    mixed = _word([_round_half_up(o * wd + n * ws, wd + ws) for o, n in zip(old, new)], np.minimum(wd + ws, cap))
    fresh = ((np.asarray(rgb).astype(I) & 0xFFFFFF) | (np.minimum(ws, cap) << 24)).astype(U)
    return np.where(wd == 0, fresh, mixed).astype(U)


# ---- the realisable numerators -------------------------------------------------------------------------------------------------
# add: old * w + new takes every value of 0 .. 255 * (w + 1) (w <= 255 < 256 = the values of `new`).
# removal: old * w - new takes every value of -255 .. 255 * w.
# combine: old * wd + new * ws with wd + ws = den: realisation() finds the (wd, ws, old, new) of a (den, num).
def nums_add(w):
    return np.arange(0, 255 * (w + 1) + 1, dtype=I)


def nums_remove(w):
    return np.arange(-255, 255 * w + 1, dtype=I)


def nums_combine(den):
    return np.arange(0, 255 * den + 1, dtype=I)


# (the enumerators below are computed once and shared: treat what they return as read-only)
def _ties(dens, nums_of, den_of):
    out = []
    for c in dens:
        den = den_of(c)
        if den % 2:
            continue
        num = nums_of(c)
        num = num[(num >= 0) & (num <= 255 * den)]                         # (the removal's clamp: ties lie inside it)
        num = num[(2 * num) % (2 * den) == den]
        out.append(np.stack([np.full(len(num), c, I), num], 1))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def ties_add():
    """[n, 2] (w, num): 2 * num mod 2 * (w + 1) == w + 1."""
    return _ties(range(0, 256), nums_add, lambda w: w + 1)


@functools.lru_cache(maxsize=None)
def ties_remove():
    """[n, 2] (w, num), w >= 2: 2 * num mod 2 * (w - 1) == w - 1."""
    return _ties(range(2, 256), nums_remove, lambda w: w - 1)


def realisation(den, num, spread=0):
    """(wd, ws, old, new) [n] each with wd + ws == den, 1 <= wd, ws <= 255 and old * wd + new * ws == num, or wd == 0 where
    (den, num) has none.  Which of the splits of den is tried first moves with `spread` [n], so that a list of pairs of one den
    does not land on one (wd, ws)."""
    den, num = np.asarray(den, I).reshape(-1), np.asarray(num, I).reshape(-1)
    spread = np.broadcast_to(np.asarray(spread, I), den.shape)
    lo, hi = np.maximum(1, den - 255), np.minimum(255, den - 1)
    found = np.zeros((4, len(den)), I)
    old = np.arange(256, dtype=I)[None, :]
    for step in range(255):
        todo = np.nonzero((found[0] == 0) & (step < hi - lo + 1))[0]
        if len(todo) == 0:
            break
        wd = lo[todo] + (spread[todo] + step) % (hi[todo] - lo[todo] + 1)
        ws = den[todo] - wd
        rest = num[todo][:, None] - old * wd[:, None]
        ok = (rest >= 0) & (rest % ws[:, None] == 0) & (rest // ws[:, None] <= 255)
        hit = ok.any(1)
        o = ok.argmax(1)
        t = todo[hit]
        found[:, t] = np.stack([wd[hit], ws[hit], o[hit], (num[t] - o[hit] * wd[hit]) // ws[hit]])
    return tuple(found)


@functools.lru_cache(maxsize=None)
def ties_combine():
    """[n, 6] (den, num, wd, ws, old, new): 2 * num mod 2 * den == den over den = 2 .. 510, one realising input each (every tie
    has one: wd = ws = den / 2, old = k + 1, new = k gives num = den / 2 + k * den)."""
    pairs = _ties(range(2, 511), nums_combine, lambda den: den)
    wd, ws, old, new = realisation(pairs[:, 0], pairs[:, 1], spread=pairs[:, 1] // pairs[:, 0])
    assert (wd > 0).all()
    return np.concatenate([pairs, np.stack([wd, ws, old, new], 1)], 1)


# ---- what a reciprocal multiply would get wrong ------------------------------------------------------------------------------------
def rcp_byte(num, den, clamp=False):
    """The byte of num * float32(1 / den), then the rule's (clamp,) + 0.5 and truncation: every operation rounded to float32."""
    num, den = np.asarray(num, I), np.asarray(den, I)
    f = (num.astype(F) * (F(1.0) / den.astype(F)).astype(F)).astype(F)
    if clamp:
        f = np.minimum(np.maximum(f, F(0.0)), F(255.0)).astype(F)
    return (f + F(0.5)).astype(F).astype(I)


def _discriminators(counts, nums_of, den_of, clamp=False):
    out = []
    for c in counts:
        den = I(den_of(c))
        num = nums_of(c)
        exact = _round_half_up(np.clip(num, 0, 255 * den) if clamp else num, den)
        bad = num[rcp_byte(num, den, clamp) != exact]
        out.append(np.stack([np.full(len(bad), c, I), bad], 1))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def rcp_discriminators_add():
    """[n, 2] (w, num) on which the reciprocal multiply differs from the exact byte."""
    return _discriminators(range(0, 256), nums_add, lambda w: w + 1)


@functools.lru_cache(maxsize=None)
def rcp_discriminators_remove():
    """[n, 2] (w, num), w >= 2, num the numerator before the clamp."""
    return _discriminators(range(2, 256), nums_remove, lambda w: w - 1, clamp=True)


@functools.lru_cache(maxsize=None)
def rcp_discriminators_combine():
    """[n, 6] (den, num, wd, ws, old, new) over den = 2 .. 510 and every num of 0 .. 255 * den that some input realises."""
    pairs = _discriminators(range(2, 511), nums_combine, lambda den: den)
    wd, ws, old, new = realisation(pairs[:, 0], pairs[:, 1], spread=pairs[:, 1])
    have = wd > 0
    return np.concatenate([pairs, np.stack([wd, ws, old, new], 1)], 1)[have]
