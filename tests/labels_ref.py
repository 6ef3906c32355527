"""The rule of the label calls (include/voxelhash.h, "the model with labels") in executable form: numpy, all integers.  It does
not import the product.

Fusing: integrate() applies one frame's label image to a label volume (uint32 per voxel, label | votes << 16, the word 0 = no
label) over the blocks `entries`, the compact set of the pose (deintegrate_ref.visible_entries).  The camera point, projection,
bounds test and depth read are colour's, taken from tests/color_ref.py (surface_samples).
Reading, counting, removing: over a model dictionary {block key: (sdf[512], weight[512], labels[512])} (removing: a fourth
member, the colour words), with the domain, voxel choice and validity of tests/sample_ref.py."""
import numpy as np

import color_ref as CR
import sample_ref as S

F = np.float32
U = np.uint32
TRANSITIONS = ("fresh", "increment", "held", "decrement", "reset")


def pack(label, votes):
    return (np.asarray(label, U) | (np.asarray(votes, U) << U(16))).astype(U)


def label_of(word):
    return np.asarray(word, U) & U(0xFFFF)


def votes_of(word):
    return np.asarray(word, U) >> U(16)


def vote(word, pixel, vote_max):
    """Step 4: the words `word` after one vote for the label `pixel` each (pixel >= 1, vote_max >= 1).  Returns (words, kind):
    kind indexes TRANSITIONS."""
    word, pixel = np.asarray(word, U), np.broadcast_to(np.asarray(pixel, U), np.shape(word))
    l, n = label_of(word).astype(np.int64), votes_of(word).astype(np.int64)
    L = pixel.astype(np.int64)
    fresh = n == 0
    same = ~fresh & (l == L)
    held = same & (np.minimum(n + 1, vote_max) == n)                        # at the cap: the word stays
    down = ~fresh & ~same & (n > 1)
    reset = ~fresh & ~same & (n == 1)
    out = np.zeros(word.shape, np.int64)
    out = np.where(fresh, L | (1 << 16), out)
    out = np.where(same, l | (np.minimum(n + 1, vote_max) << 16), out)
    out = np.where(down, l | ((n - 1) << 16), out)
    out = np.where(reset, 0, out)
    kind = np.select([fresh, same & ~held, held, down, reset], [0, 1, 2, 3, 4], -1)
    return out.astype(U), kind


def integrate(labels, voxels, entries, params, semantics, proj, pose_inv, depth_source, image, band, vote_max):
    """A copy of the label volume `labels` after vh_integrate_labels over the blocks `entries` (VoxelEntry records with their
    ptr); `voxels` is the TSDF volume as it is at the call.  image: uint16 [H, W].  Returns (labels, stats): stats counts the
    swept words, the held voxels rejected, the in-band voxels a label-0 pixel left alone (`spared`: those of them that carry a
    label), and every transition by name."""
    out = np.array(labels, U, copy=True)
    n = len(entries)
    stats = dict(swept=0, rejected=0, unlabelled=0, spared=0, voted=0, **{k: 0 for k in TRANSITIONS})
    if n == 0:
        return out, stats
    at = entries["ptr"].astype(np.int64)[:, None] + np.arange(512)[None, :]
    holds = voxels["weight"][at] > F(0.0)
    ok, s, sx, sy = CR.surface_samples(entries, params, semantics, proj, pose_inv, depth_source)
    with np.errstate(invalid="ignore"):
        near = ok & (np.abs(s) <= F(band))
    pixel = np.asarray(image).astype(U)[sy, sx]
    inband = holds & near
    take = inband & (pixel != 0) & (vote_max != 0)
    word = out[at]
    new = word.copy()
    new[~holds] = 0
    if take.any():
        new[take], kind = vote(word[take], pixel[take], vote_max)
        for i, k in enumerate(TRANSITIONS):
            stats[k] = int((kind == i).sum())
    out[at] = new
    stats.update(swept=int(((word != 0) & ~holds).sum()), rejected=int((holds & ~near).sum()),
                 unlabelled=int((inband & (pixel == 0)).sum()), spared=int((inband & (pixel == 0) & (word != 0)).sum()),
                 voted=int(take.sum()))
    return out, stats


class LabelField(S.Field):
    """The model's voxels and label words by global integer coordinate: model = {key: (sdf[512], weight[512], labels[512], ...)}."""

    def __init__(self, model):
        super().__init__({k: (v[0], v[1]) for k, v in model.items()})
        self.label = np.zeros((len(self.row) + 1, 512), U)                  # row n: the absent block
        for i, v in enumerate(model.values()):
            self.label[i] = np.asarray(v[2], U)
        self.label[~(self.sdf == self.sdf)] = 0                             # a voxel that is not valid shows no label

    def words(self, g):
        g = np.asarray(g, np.int64)
        flat = g.reshape(-1, 3)
        keys, inverse = np.unique(flat >> 3, axis=0, return_inverse=True)
        rows = np.array([self.row.get(tuple(k), len(self.row)) for k in keys.tolist()], np.int64).reshape(-1)
        row = rows[inverse.reshape(-1)]
        index = ((flat[:, 2] & 7) << 6) | ((flat[:, 1] & 7) << 3) | (flat[:, 0] & 7)
        return self.label[row, index].reshape(g.shape[:-1])


def read(word, min_votes):
    """The word as a reader with min_votes sees it."""
    word = np.asarray(word, U)
    return np.where(votes_of(word) >= max(int(min_votes), 1), word, U(0)).astype(U)


def sample(model, points, voxel_size, min_votes=1):
    """points [n, 3] float32 world metres -> uint32 [n]: the nearest voxel's word, or 0."""
    field = model if isinstance(model, LabelField) else LabelField(model)
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    vs = F(voxel_size)
    out = np.zeros(len(p), U)
    with np.errstate(all="ignore"):
        u = (p / vs).astype(F)
        inside = (np.abs(u) < S.DOMAIN).all(1)                              # False for NaN
        u = u[inside]
        r = np.trunc((u + np.copysign(F(0.5), u)).astype(F)).astype(np.int64)
    out[inside] = read(field.words(r), min_votes)
    return out


def sample_map(model, pose, points4, voxel_size, min_votes=1):
    q, _ = CR.to_world(pose, points4)                                       # (.z == 0: NaN, which no sample accepts)
    return sample(model, q, voxel_size, min_votes)


def in_region(key, region):
    return region is None or all(int(lo) <= int(c) < int(hi) for c, lo, hi in zip(key, region[0], region[1]))


def valid_mask(sdf, weight):
    sdf, weight = np.asarray(sdf, F), np.asarray(weight, F)
    with np.errstate(invalid="ignore"):
        return (weight > 0) & ~np.isnan(sdf)


def counts(model, n_bins, min_votes=1, region=None):
    """vh_label_counts: uint32 [n_bins] over the blocks of `model` inside `region` = ((lo), (hi)) in blocks."""
    out = np.zeros(int(n_bins), np.int64)
    for key, v in model.items():
        if not in_region(key, region):
            continue
        valid = valid_mask(v[0], v[1])
        l = label_of(read(v[2], min_votes)).astype(np.int64)[valid]
        out += np.bincount(np.where(l < n_bins, l, 0), minlength=int(n_bins))
    return out.astype(U)


def remove(model, label, min_votes=1, region=None):
    """vh_remove_label on model = {key: (sdf, weight, labels, colour)}: (the model afterwards, stats, freed keys).  Every voxel
    whose word has `label` with votes >= max(min_votes, 1) becomes {0, 0} with colour 0 and label 0; a block in which a voxel
    was cleared and whose 512 weights are then all 0 leaves the model; everything else keeps its bits."""
    out, freed = {}, []
    stats = dict(blocks=0, removed_voxels=0, freed_blocks=0)
    for key, v in model.items():
        s, w, lab, col = (np.array(v[0], F), np.array(v[1], F), np.array(v[2], U), np.array(v[3], U))
        if in_region(key, region):
            stats["blocks"] += 1
            gone = (label_of(lab) == int(label)) & (votes_of(lab) >= max(int(min_votes), 1))
            if gone.any():
                s[gone], w[gone], lab[gone], col[gone] = 0, 0, 0, 0
                stats["removed_voxels"] += int(gone.sum())
                if (w == 0).all():
                    freed.append(key)
                    continue
        out[key] = (s, w, lab, col)
    stats["freed_blocks"] = len(freed)
    return out, stats, freed
