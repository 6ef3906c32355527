"""Crafted colour words for tests/test_color_count_ref_cpu.py and tests/test_gpu_color_counts.py: the room model of
tests/deintegrate_cases.py (64x48 frames, 2^11 buckets, 512 blocks) taken out whole as a chunk -- what stream_out returns: keys,
voxels, colours -- edited on the host and put back with stream_in, so that crafted contents sit at natural keys and the flatten,
the frustum test and the references work unchanged.  Sample counts of 0..255 in every word, which no fused model of the suite
reaches (tests/merge_color_cases.py: 4).

The frame calls: every voxel is given a positive weight and the band is metres wide, so every voxel of a visible block that
projects onto a pixel with depth > 0 is sampled; color_ref.surface_samples says which pixel before anything is chosen.  The image
is drawn from a seeded generator and the words are picked greedily against a FrameGoal: the (count, old byte) pairs and the
(count, numerator) pairs of tests/color_count_ref.py (ties and reciprocal discriminators) that are still uncovered.  A frame
samples some 25 000 voxels, so a goal takes a few rounds: craft, stream_in, call, compare, again.
vh_merge_color: under an identity transform in nearest mode a dst voxel sees the word of the src voxel of its own key and index,
so both words are free per voxel (merge_specs); under a translation by half voxels at voxelSize 2^-5 every trilinear weight is
exactly 0.5 (fine_words gives the corner counts a wide range).

Nothing here needs a GPU: host_state() stands in for a context that received the chunk, with the entry layout the references
read (pos, ptr), and the CPU module proves the coverage conditions of every crafted input on the oracle's model before any GPU
run.  The GPU tests assert the same conditions on the model the GPU fused."""
import numpy as np

import color_count_ref as X
import color_ref as CR
import deintegrate_cases as DC
import deintegrate_ref as D

F = np.float32
U = np.uint32
I = np.int64
W, H = DC.W, DC.H
BAND = 8.0                                                    # metres: past every voxel of the room
FINE_VS = 2.0 ** -5                                           # the voxel size of the half-voxel cases: g * vs and t are exact
HALF_SHIFT = (2.5, 0.5, 1.5)                                  # voxels
# the contexts of the half-voxel merge: 2^13 buckets, because the room's 2^11 leave some bucket the home of more keys than its
# slots once the shifted candidates are added, and vh_merge then leaves them unplaced (tests/test_color_count_ref_cpu.py counts)
FINE_KW = dict(voxelSize=FINE_VS, numBuckets=1 << 13)
ENTRY = np.dtype([("pos", np.int32, 3), ("ptr", np.int32)])
VOXEL = np.dtype([("sdf", F), ("weight", F)])
LOCAL = np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], 1).astype(I)


def codes(count, num):
    """One integer per (count, num) pair (num >= -255): what the coverage sets are kept as."""
    return np.asarray(count, I) * (1 << 20) + (np.asarray(num, I) + 255)


# ---- the room as a chunk, with and without a GPU -------------------------------------------------------------------------------
def host_room(oracle, sem, **kw):
    """(chunk, params) of the three-frame room by the repository's CPU oracle."""
    ot = DC.oracle_table(oracle, sem, **kw)
    for pose, _, verts in DC.frames(oracle):
        ot.integrate(pose, verts)
    tab, vox = ot.hash_table(), ot.sdf_blocks()
    live = tab[tab["ptr"] != -1]
    voxels = np.zeros((len(live), 512), VOXEL)
    for i, e in enumerate(live):
        p = int(e["ptr"])
        voxels[i]["sdf"], voxels[i]["weight"] = vox["sdf"][p:p + 512], vox["weight"][p:p + 512]
    chunk = {"keys": live["pos"].astype(np.int32).copy(), "voxels": voxels, "colors": None}
    vs = float(ot.params.voxelSize)
    ot.close()
    return chunk, vs


def host_state(chunk):
    """What the references read of a context that took `chunk` into an empty table: entries (pos, ptr), the SDF volume, the
    colour volume."""
    n = len(chunk["keys"])
    table = np.zeros(n, ENTRY)
    table["pos"], table["ptr"] = chunk["keys"], np.arange(n) * 512
    vox = np.zeros(n * 512, VOXEL)
    vox["sdf"], vox["weight"] = chunk["voxels"]["sdf"].reshape(-1), chunk["voxels"]["weight"].reshape(-1)
    return dict(table=table, vox=vox, color=np.asarray(chunk["colors"], U).reshape(-1).copy())


def chunk_model(chunk):
    """{key: (sdf, weight, colour)} of a chunk."""
    return {tuple(k): (chunk["voxels"]["sdf"][i].copy(), chunk["voxels"]["weight"][i].copy(), np.asarray(chunk["colors"][i], U).copy())
            for i, k in enumerate(np.asarray(chunk["keys"]).tolist())}


class Params:
    """The one field of the table parameters the frame references read."""
    def __init__(self, voxel_size):
        self.voxelSize = float(voxel_size)


def depth_source(frame, sensor):
    return (frame[1], DC.k_inv()) if sensor else frame[2][..., 2]


def frame_take(oracle, state, vs, sem, frame, sensor, band=BAND):
    """(entries, at, take, pixel index): the voxels color_ref.integrate / merge_color_ref.deintegrate sample in `state` -- the
    references' own steps 1 to 3 (a removal further asks for a count > 0)."""
    proj, inv = DC.projection(sem), oracle.invert4x4(frame[0])
    table = state["table"]
    entries = table[D.visible_entries(table, Params(vs), sem, proj, frame[0], inv, W, H)]
    at = entries["ptr"].astype(I)[:, None] + np.arange(512)[None, :]
    holds = state["vox"]["weight"][at] > F(0.0)
    ok, s, sx, sy = CR.surface_samples(entries, Params(vs), sem, proj, inv, depth_source(frame, sensor))
    with np.errstate(invalid="ignore"):
        take = holds & ok & (np.abs(s) <= F(band))
    return entries, at, take, sy * W + sx


# ---- what a frame call must see --------------------------------------------------------------------------------------------------
class FrameGoal:
    """The (count, old byte) pairs and the (count, num) pairs (ties and reciprocal discriminators) that no round has placed
    yet.  kind: "add" (vh_integrate_color: counts 0..255) or "remove" (vh_deintegrate_color: counts 1..255, and for every count
    >= 2 a channel below 0 and one above 255 before the clamp)."""

    def __init__(self, kind, spread=False):
        self.kind = kind
        self.spread = spread                                  # a round gives every count an equal share of its voxels
        self.pairs = np.ones((256, 256), bool)
        if kind == "add":
            listed = np.concatenate([X.ties_add(), X.rcp_discriminators_add()])
        else:
            self.pairs[0] = False
            listed = np.concatenate([X.ties_remove(), X.rcp_discriminators_remove()])
        self.nums = {}
        for w, num in np.unique(listed, axis=0).tolist():
            self.nums.setdefault(w, set()).add(num)
        self.low = np.zeros(256, bool)                        # (removal) counts whose clamp at 0 / at 255 is still to place
        self.high = np.zeros(256, bool)
        if kind == "remove":
            self.low[2:] = self.high[2:] = True

    def left(self):
        return int(self.pairs.sum()) + sum(len(v) for v in self.nums.values()) + int(self.low.sum()) + int(self.high.sum())

    def inputs_of(self, w, num):
        """The (old, pixel byte) that give `num` at count w."""
        if self.kind == "add":                                # num = old * w + new
            olds = range(max(0, -((255 - num) // w)), min(255, num // w) + 1)
            return [(o, num - o * w) for o in olds]
        olds = range(max(0, -(-num // w)), min(255, (num + 255) // w) + 1)        # num = old * w - new
        return [(o, o * w - num) for o in olds]

    def assign(self, nb, rng):
        """nb [m, 3]: the pixel bytes the m sampled voxels will receive.  Returns (count [m], old [m, 3]) with -1 where the goal
        asks for nothing (the caller's fill stays), and strikes what it placed."""
        m = len(nb)
        nb = np.asarray(nb, I)
        count, old = np.full(m, -1, I), np.full((m, 3), -1, I)
        used = np.zeros(m, bool)
        order = rng.permutation(m).tolist()
        by_byte = [[] for _ in range(256)]
        for v in order:
            for ch in range(3):
                by_byte[nb[v, ch]].append((v, ch))
        spare = list(order)

        def any_voxel():
            while spare:
                v = spare.pop()
                if not used[v]:
                    used[v] = True
                    return v
            return None

        def voxel_with(byte):
            lst = by_byte[byte]
            while lst:
                v, ch = lst.pop()
                if not used[v]:
                    used[v] = True
                    return v, ch
            return None

        remove = self.kind == "remove"
        share = m // 256 if self.spread else m                # the voxels one count may take
        for w in range(255, -1, -1):                          # (high counts first: their numerators fit one pixel byte only)
            slots = []
            for num in sorted(self.nums.get(w, ())):
                if len(slots) >= 2 * share:
                    break
                options = self.inputs_of(w, num)
                k = int(rng.integers(len(options)))
                for o, byte in options[k:] + options[:k]:
                    got = voxel_with(byte)
                    if got is not None:
                        v, ch = got
                        count[v], old[v, ch] = w, o
                        self.nums[w].discard(num)
                        self.pairs[w, o] = False
                        slots += [(v, c) for c in range(3) if c != ch]
                        break
            wanted = np.nonzero(self.pairs[w])[0].tolist()
            if remove and self.low[w]:
                wanted = [0] + [o for o in wanted if o != 0]  # (old 0 under a pixel > 0 falls below 0, old 255 under one < 255
            if remove and self.high[w]:                       # rises above 255)
                wanted = [255] + [o for o in wanted if o != 255]
            for o in wanted:
                need = (lambda b: b > 0) if remove and o == 0 and self.low[w] else \
                       (lambda b: b < 255) if remove and o == 255 and self.high[w] else (lambda b: True)
                at = next((j for j in range(len(slots) - 1, -1, -1) if need(nb[slots[j]])), None)
                while at is None:
                    v = any_voxel() if not self.spread or (count == w).sum() < share else None
                    if v is None:
                        break
                    count[v] = w
                    slots += [(v, c) for c in range(3)]
                    at = next((j for j in range(len(slots) - 1, max(len(slots) - 4, -1), -1) if need(nb[slots[j]])), None)
                if at is None:
                    break                                     # the frame's voxels are used up: the next round goes on
                v, ch = slots.pop(at)
                old[v, ch] = o
                self.pairs[w, o] = False
                if remove and w >= 2 and o == 0 and nb[v, ch] > 0:
                    self.low[w] = False
                if remove and w >= 2 and o == 255 and nb[v, ch] < 255:
                    self.high[w] = False
        return count, old


def draw_words(rng, shape, counts=None):
    """Words with every byte from the generator; counts: the values the count byte is drawn from (0..255 if None)."""
    words = rng.integers(0, 1 << 24, shape, dtype=np.int64).astype(U)
    c = rng.integers(0, 256, shape) if counts is None else np.asarray(counts)[rng.integers(0, len(counts), shape)]
    return (words | (c.astype(U) << U(24))).astype(U)


def draw_image(rng):
    """A colour image with every byte value in every channel; byte 3 is noise the library must ignore."""
    image = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(U).reshape(-1)
    ramp = np.arange(256, dtype=U)
    image[:256] = (image[:256] & U(0xFF000000)) | ramp | (rng.permutation(ramp) << U(8)) | (rng.permutation(ramp) << U(16))
    return image[rng.permutation(H * W)].reshape(H, W)


def craft_frame(oracle, room, vs, sem, frame, sensor, seed, goal=None, counts=None, zero=0.0, plain_empty=False):
    """(chunk, image) for one frame call on the room's blocks: every weight positive, the words from the generator (counts:
    what their count byte is drawn from; zero: the share of words that are 0; plain_empty: a count of 0 only as the word 0),
    then the goal's picks over the voxels the call will sample."""
    rng = np.random.default_rng(seed)
    n = len(room["keys"])
    voxels = room["voxels"].copy()
    voxels["weight"] = np.maximum(voxels["weight"], F(1.0))
    words = draw_words(rng, (n, 512), counts)
    words[rng.random((n, 512)) < zero] = 0
    if plain_empty:
        words[CR.count(words) == 0] = 0
    image = draw_image(rng)
    chunk = {"keys": room["keys"].copy(), "voxels": voxels, "colors": words}
    if goal is not None:
        entries, at, take, pixel = frame_take(oracle, host_state(chunk), vs, sem, frame, sensor)
        if zero:
            take &= words.reshape(-1)[at] != 0                # (the words of 0 under the frame stay: a removal must leave them)
        where = at[take]
        nb = np.stack(CR.channels(image.reshape(-1)[pixel[take]]), 1)
        count, old = goal.assign(nb, rng)
        flat = words.reshape(-1)
        picked = count >= 0
        drawn = np.stack(CR.channels(flat[where]), 1).astype(I)
        old = np.where(old >= 0, old, drawn)
        flat[where[picked]] = CR.pack(old[picked, 0], old[picked, 1], old[picked, 2], count[picked])
    return chunk, image


def frame_coverage(kind, words, pixels):
    """(pairs [256, 256] bool by (count, old byte), the codes of the (count, num) pairs) over sampled words and their pixels."""
    w = CR.count(words).astype(I)
    pairs = np.zeros((256, 256), bool)
    seen = []
    for old, new in zip(CR.channels(words), CR.channels(pixels)):
        pairs[w, old.astype(I)] = True
        num = old.astype(I) * w + new.astype(I) if kind == "add" else old.astype(I) * w - new.astype(I)
        seen.append(codes(w, num))
    return pairs, np.unique(np.concatenate(seen))


def clamps(words, pixels):
    """(low [256], high [256]) bool by count: a removal's channel falls below 0 / rises above 255 before the clamp."""
    w = CR.count(words).astype(I)
    low, high = np.zeros(256, bool), np.zeros(256, bool)
    for old, new in zip(CR.channels(words), CR.channels(pixels)):
        num = old.astype(I) * w - new.astype(I)
        low[w[(w >= 2) & (num < 0)]] = True
        high[w[(w >= 2) & (num > 255 * (w - 1))]] = True
    return low, high


# ---- vh_merge_color, identity, nearest: both words free per voxel -------------------------------------------------------------------
_SPECS = {}


def merge_specs(seed=11):
    """(wd [n], ws [n], old [n, 3], new [n, 3]): one entry per voxel to craft -- every (wd, ws) of 0..255 x 1..255, every
    (den, num) of ties_combine() and rcp_discriminators_combine() in some channel (further voxels of a (wd, ws) where its three
    channels do not hold them), 64 voxels whose src word is 0 (ws == 0) -- in a seeded random order."""
    if seed in _SPECS:
        return _SPECS[seed]
    rng = np.random.default_rng(seed)
    listed = np.unique(np.concatenate([X.ties_combine(), X.rcp_discriminators_combine()]), axis=0)
    pid = listed[:, 2] * 256 + listed[:, 3]
    listed = listed[np.argsort(pid, kind="stable")]
    pid = np.sort(pid, kind="stable")
    held = np.bincount(pid, minlength=256 * 256)
    base = np.zeros(256 * 256, bool)
    base[np.arange(256 * 256) % 256 >= 1] = True              # ws >= 1, wd 0..255
    voxels = np.where(base, np.maximum(1, -(-held // 3)), 0)
    start = np.concatenate([[0], np.cumsum(voxels)])
    n = int(start[-1]) + 64
    which = np.repeat(np.arange(256 * 256), voxels)
    wd = np.concatenate([which // 256, rng.integers(1, 256, 64)])
    ws = np.concatenate([which % 256, np.zeros(64, I)])
    old, new = rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3))
    rank = np.arange(len(pid)) - np.searchsorted(pid, pid, side="left")
    at, ch = start[pid] + rank // 3, rank % 3
    old[at, ch], new[at, ch] = listed[:, 4], listed[:, 5]
    order = rng.permutation(n)
    _SPECS[seed] = (wd[order].astype(I), ws[order].astype(I), old[order].astype(I), new[order].astype(I))
    return _SPECS[seed]


def merge_rounds(room):
    return -(-len(merge_specs()[0]) // (len(room["keys"]) * 512))


def craft_merge(room, rnd, seed=12):
    """(dst chunk, src chunk) of round `rnd`: the room's blocks with every weight positive in both, the specs rnd * voxels ..
    of merge_specs() in the blocks' voxels in order, and drawn words behind the last spec."""
    rng = np.random.default_rng(seed + rnd)
    n = len(room["keys"]) * 512
    wd, ws, old, new = [a[rnd * n:(rnd + 1) * n] for a in merge_specs()]
    voxels = room["voxels"].copy()
    voxels["weight"] = np.maximum(voxels["weight"], F(1.0))
    dst, src = draw_words(rng, n), draw_words(rng, n)
    dst[:len(wd)] = CR.pack(old[:, 0], old[:, 1], old[:, 2], wd)
    src[:len(ws)] = CR.pack(new[:, 0], new[:, 1], new[:, 2], ws)
    dst[CR.count(dst) == 0] = 0                               # (a count of 0 is the word 0 in a model)
    src[CR.count(src) == 0] = 0
    return ({"keys": room["keys"].copy(), "voxels": voxels, "colors": dst.reshape(-1, 512)},
            {"keys": room["keys"].copy(), "voxels": voxels.copy(), "colors": src.reshape(-1, 512)})


def merge_coverage(words, rgb, cnt):
    """(pairs [256, 256] bool by (wd, ws), codes of (den, num), wd >= 1) over dst words and the samples they take."""
    wd, ws = CR.count(words).astype(I), np.asarray(cnt, I)
    pairs = np.zeros((256, 256), bool)
    pairs[wd, ws] = True
    mixed = wd > 0
    seen = [codes((wd + ws)[mixed], (o.astype(I) * wd + n.astype(I) * ws)[mixed]) for o, n in zip(CR.channels(words), CR.channels(rgb))]
    return pairs, np.unique(np.concatenate(seen))


# ---- the half-voxel models ------------------------------------------------------------------------------------------------------------
def fine_words(room, seed, cell=4):
    """Words for the blocks of a voxelSize 2^-5 room: every byte drawn, the count constant over cells of `cell`^3 voxels and
    drawn per cell from 1..255 with 1, 2, 254 and 255 as likely as all the others together, so that the least count of a
    trilinear sample's eight corners reaches both ends."""
    rng = np.random.default_rng(seed)
    keys = np.asarray(room["keys"], I)
    g = keys[:, None, :] * 8 + LOCAL[None, :, :]
    c = g // cell
    h = (c[..., 0] * 73856093) ^ (c[..., 1] * 19349663) ^ (c[..., 2] * 83492791) ^ (seed * 2654435761)
    h = (h ^ (h >> 13)) * 0x5BD1E995
    h = (h ^ (h >> 15)) & 0x7FFFFFFF
    ends = np.array([1, 2, 254, 255])
    count = np.where(h % 2 == 0, ends[(h >> 1) % 4], 1 + (h >> 3) % 255)
    words = (rng.integers(0, 1 << 24, count.shape, dtype=np.int64) | (count << 24)).astype(U)
    voxels = room["voxels"].copy()
    voxels["weight"] = np.maximum(voxels["weight"], F(1.0))
    return {"keys": room["keys"].copy(), "voxels": voxels, "colors": words}


def half_shift(vs=FINE_VS):
    T = np.eye(4, dtype=F)
    T[:3, 3] = np.asarray(HALF_SHIFT, F) * F(vs)
    return T


# ---- the rounds of a frame goal, and what they covered ---------------------------------------------------------------------------------
def frame_rounds(oracle, room, vs, kind, sem, sensor, seed, most, **fill):
    """Yields (frame, chunk, image) per round until the goal of `kind` is placed or `most` rounds are out: round r uses frame
    r mod 3 of tests/deintegrate_cases.py and the generator seed + r.  A single round spreads its voxels over all counts."""
    goal = FrameGoal(kind, spread=most == 1)
    frames = DC.frames(oracle)
    for rnd in range(most):
        frame = frames[rnd % 3]
        chunk, image = craft_frame(oracle, room, vs, sem, frame, sensor, seed + rnd, goal, **fill)
        yield frame, chunk, image
        if goal.left() == 0:
            return


class FrameCoverage:
    """What the sampled channels of the rounds so far held, from the words before each call and the pixels the reference's
    own `take` mask gives them."""

    def __init__(self, kind):
        self.kind = kind
        self.pairs = np.zeros((256, 256), bool)
        self.codes = np.zeros(0, I)
        self.bytes = np.zeros(256, bool)
        self.low, self.high = np.zeros(256, bool), np.zeros(256, bool)
        self.samples = 0
        if kind == "add":
            self.ties, self.rcp = X.ties_add(), X.rcp_discriminators_add()
        else:
            self.ties, self.rcp = X.ties_remove(), X.rcp_discriminators_remove()

    def add(self, words, pixels):
        pairs, seen = frame_coverage(self.kind, words, pixels)
        self.pairs |= pairs
        self.codes = np.union1d(self.codes, seen)
        for new in CR.channels(pixels):
            self.bytes[new] = True
        if self.kind == "remove":
            low, high = clamps(words, pixels)
            self.low |= low
            self.high |= high
        self.samples += len(words)

    def ties_seen(self):
        return int(np.isin(codes(self.ties[:, 0], self.ties[:, 1]), self.codes).sum())

    def rcp_seen(self):
        return int(np.isin(codes(self.rcp[:, 0], self.rcp[:, 1]), self.codes).sum())

    def report(self):
        first = 0 if self.kind == "add" else 1
        return (f"{self.kind}: {self.samples} samples, (count, old) pairs {int(self.pairs.sum())} of {(256 - first) * 256}, ties "
                f"{self.ties_seen()} of {len(self.ties)}, reciprocal discriminators {self.rcp_seen()} of {len(self.rcp)}, pixel bytes "
                f"{int(self.bytes.sum())}, clamped low / high at {int(self.low.sum())} / {int(self.high.sum())} counts")

    def check_full(self):
        """Every pair, every tie, every discriminator, every pixel byte (and for a removal both clamps at every count >= 2)."""
        first = 0 if self.kind == "add" else 1
        assert self.pairs[first:].all(), np.argwhere(~self.pairs[first:])[:4] + [first, 0]
        assert self.ties_seen() == len(self.ties) > 30000
        assert self.rcp_seen() == len(self.rcp) > 1000        # (every discriminator is among what was covered)
        assert self.bytes.all()
        if self.kind == "remove":
            assert self.low[2:].all() and self.high[2:].all()

    def check_every_count(self, ties):
        """The lesser condition of the rounds that guard another instantiation of the same tail."""
        first = 0 if self.kind == "add" else 1
        assert self.pairs[first:].any(1).all() and self.ties_seen() >= ties


class MergeCoverage:
    def __init__(self):
        self.pairs = np.zeros((256, 256), bool)
        self.codes = np.zeros(0, I)
        self.samples = 0
        self.ties, self.rcp = X.ties_combine(), X.rcp_discriminators_combine()

    def add(self, words, rgb, cnt):
        pairs, seen = merge_coverage(words, rgb, cnt)
        self.pairs |= pairs
        self.codes = np.union1d(self.codes, seen)
        self.samples += len(words)

    def ties_seen(self):
        return int(np.isin(codes(self.ties[:, 0], self.ties[:, 1]), self.codes).sum())

    def rcp_seen(self):
        return int(np.isin(codes(self.rcp[:, 0], self.rcp[:, 1]), self.codes).sum())

    def report(self):
        return (f"merge: {self.samples} samples, (wd, ws) pairs {int(self.pairs[1:, 1:].sum())} of {255 * 255}, fresh with "
                f"{int(self.pairs[0, 1:].sum())} of 255 counts, ties {self.ties_seen()} of {len(self.ties)}, reciprocal discriminators "
                f"{self.rcp_seen()} of {len(self.rcp)}")

    def check_full(self):
        assert self.pairs[:, 1:].all()                        # every (wd, ws) of 0..255 x 1..255: the fresh branch with every ws
        assert self.ties_seen() == len(self.ties) > 60000
        assert self.rcp_seen() == len(self.rcp) > 1000


def merge_take(src_model, dst_model, keys, Tinv, vs, mode):
    """(step, rgb, cnt) [len(keys), 512]: where the colour step happens for dst's blocks `keys` and what it takes of src -- the
    references' own sampling (merge_ref.samples, merge_color_ref.color_samples)."""
    import merge_color_ref as M
    import merge_ref as R
    s, w = R.samples(M.geometry(src_model), keys, Tinv, vs, vs, mode)
    with np.errstate(invalid="ignore"):
        take = (s == s) & (w > 0)
    rgb, cnt = M.color_samples(src_model, keys, Tinv, vs, vs, mode, where=take)
    return take & (cnt > 0), rgb, cnt


def half_weights(keys, Tinv, vs):
    """The trilinear weights t [n * 512, 3] of the voxels of dst's blocks `keys` under Tinv, by the references' arithmetic."""
    import merge_ref as R
    keys = np.asarray(list(keys), I).reshape(-1, 3)
    g = (keys[:, None, :] * 8 + LOCAL[None, :, :]).reshape(-1, 3)
    q = np.stack(R.rows(Tinv, *[(g[:, a].astype(F) * F(vs)).astype(F) for a in range(3)]), 1)
    u = (q / F(vs)).astype(F)
    return (u - np.floor(u)).astype(F)


# ---- the cases of tests/test_gpu_color_counts.py, proved without a GPU in tests/test_color_count_ref_cpu.py -----------------------------
SEED_ADD, SEED_REMOVE, SEED_CAPS, SEED_FINE, SEED_INOUT = 40, 60, 1000, 80, 90
MOST_ROUNDS = 4                                               # (two are enough on the oracle's model)
OTHER_ADDS = [(1, False), (0, True)]                          # (semantics, uint16 sensor image): the vertex map, REFERENCE semantics
CAPS = [254, 100, 1]
FINE_CAP = 100


def cap_counts(cap):
    """What the counts of a cap round are drawn from: 0..255, every third draw from the five counts around the cap."""
    around = [c for c in range(cap - 2, cap + 3) if 0 <= c <= 255]
    return np.concatenate([np.arange(256), np.resize(around, 128)])


def check_cap_counts(count, cap):
    """Counts below, at the step below, at and above the cap are all sampled (a word above the cap comes from a session with a
    higher one: step 7 brings it down to the cap at once)."""
    below, at, above = int((count < cap - 1).sum()), int((count == cap).sum()), int((count > cap).sum())
    assert (count == cap - 1).any() and at > 0 and above > 0 and (below > 0 or cap == 1)
    return f"cap {cap}: {len(count)} samples, counts below / at / above the cap: {below + int((count == cap - 1).sum())} / {at} / {above}"


def check_half_voxel(t, wd, least, cap):
    assert len(t) > 1000 and (t == F(0.5)).all()
    seen = np.unique(least)
    total = wd.astype(I) + least.astype(I)
    assert len(seen) >= 64 and seen[0] == 1 and seen[-1] == 255 and (least < cap).any() and (least > cap).any()
    assert ((wd > 0) & (total > cap)).any() and ((wd > 0) & (total <= cap)).any() and (wd == 0).any()
    return (f"half-voxel merge: {len(t)} samples with t == 0.5, {len(seen)} distinct least counts, {int((total > cap).sum())} above "
            f"the cap of {cap}")


def check_restored(words, back):
    """Counts 0..253, one image in and out again: the count is back and every channel within 1 (the bound
    tests/test_color_count_ref_cpu.py proves for the rule over every input)."""
    assert np.array_equal(CR.count(back), CR.count(words))
    worst = max(int(np.abs(a.astype(I) - b.astype(I)).max()) for a, b in zip(CR.channels(back), CR.channels(words)))
    assert worst <= 1
    return f"in and out: {len(words)} samples, the largest channel difference is {worst}"
