"""The rule of vh_components / vh_remove_components (include/voxelhash.h) in executable form, on a model dictionary in
tests/mesh_models.py's format: {block key: (sdf[512], weight[512])}, voxel index ((z&7)<<6)|((y&7)<<3)|(x&7).

A voxel is valid iff weight > 0 and its sdf is not NaN.  The nodes are the valid voxels with sdf <= 0 (INSIDE) or the other
valid voxels (OUTSIDE) of the listed blocks: the keys of `order` (the table's allocated entries in ascending entry index; the
dictionary's order when None) that lie inside `region` = ((lo), (hi)) in blocks.  Nodes A and B are joined iff B - A = +-o
for o an axis unit (connectivity 6) or o in {0,1}^3 minus 0 (14).  A node's id is rank * 512 + voxel index, a component's
root its least id, components come in ascending root id.

label() is a union-find by label propagation: every edge's two ends take the smaller of their labels, every label is
replaced by its own label, until nothing changes; then a component's label is its least id.  label_plain() is the textbook
union-find, node by node, for the small models tests/test_components_ref_cpu.py pins label() on."""
import numpy as np

INSIDE, OUTSIDE = 0, 1
NONE = 0xFFFFFFFF
MAX_BLOCKS = (1 << 23) - 1
RECORD = np.dtype([("voxel", "<i4", (3,)), ("size", "<u4")])
OFFSETS = {6: (1, 2, 4), 14: (1, 2, 3, 4, 5, 6, 7)}              # bit 0: +x, bit 1: +y, bit 2: +z
V = np.arange(512)
LOCAL = np.stack([V & 7, (V >> 3) & 7, V >> 6], 1)               # [512, 3] (x, y, z)


def order_of(table):
    """The allocated keys of a downloaded table in ascending entry index: the ordered block list."""
    return [tuple(int(c) for c in p) for p in table["pos"][table["ptr"] != -1]]


def node_mask(sdf, weight, target):
    sdf, weight = np.asarray(sdf, np.float32), np.asarray(weight, np.float32)
    with np.errstate(invalid="ignore"):
        valid = (weight > 0) & ~np.isnan(sdf)
        inside = sdf <= 0
    return valid & (inside if target == INSIDE else ~inside)


def listed(model, order=None, region=None):
    keys = [tuple(int(c) for c in k) for k in (order if order is not None else model)]
    if region is not None:
        lo, hi = region
        keys = [k for k in keys if all(int(l) <= c < int(h) for c, l, h in zip(k, lo, hi))]
    return keys


class Labelling:
    """keys: the listed blocks in order; node [n, 512]; index [n, 512] uint32: the component index of every node, NONE
    elsewhere; records: RECORD per component in output order; stats: what vh_component_stats reports of the labelling."""

    def __init__(self, keys, node, root):
        self.keys, self.node = keys, node
        self.rank = {k: i for i, k in enumerate(keys)}
        flat = node.reshape(-1)
        roots, inverse, sizes = np.unique(root[flat], return_inverse=True, return_counts=True)
        self.roots = roots.astype(np.int64)
        self.index = np.full(flat.shape, NONE, np.uint32)
        self.index[flat] = inverse.astype(np.uint32)
        self.index = self.index.reshape(node.shape)
        self.records = np.zeros(len(roots), RECORD)
        if len(roots):
            k = np.array(keys, np.int64).reshape(-1, 3)[self.roots >> 9]
            self.records["voxel"] = (k * 8 + LOCAL[self.roots & 511]).astype(np.int32)
            self.records["size"] = sizes
        self.stats = dict(blocks=len(keys), nodes=int(flat.sum()), components=len(roots),
                          largest=int(sizes.max()) if len(roots) else 0, removed_components=0, removed_voxels=0, freed_blocks=0)

    def labels(self, lo, dims):
        """The lattice box lo <= g < lo + dims as [dims[2], dims[1], dims[0]] uint32: component index or NONE."""
        lo, dims = np.asarray(lo, np.int64), np.asarray(dims, np.int64)
        out = np.full((dims[2], dims[1], dims[0]), NONE, np.uint32)
        if (dims == 0).any():
            return out
        g = np.stack(np.meshgrid(*(np.arange(lo[a], lo[a] + dims[a]) for a in (2, 1, 0)), indexing="ij"), -1)[..., ::-1]
        key, v = g >> 3, ((g[..., 2] & 7) << 6) | ((g[..., 1] & 7) << 3) | (g[..., 0] & 7)
        for k in {tuple(int(c) for c in q) for q in key.reshape(-1, 3)}:
            if k in self.rank:
                here = (key == np.array(k)).all(-1)
                out[here] = self.index[self.rank[k]][v[here]]
        return out

    def blocks_of(self):
        """Per component, the number of listed blocks it has nodes in."""
        r, c = np.nonzero(self.node)
        pairs = np.unique(np.stack([self.index[r, c].astype(np.int64), r], 1), axis=0)
        return np.bincount(pairs[:, 0], minlength=len(self.records))

    def canonical(self):
        """The partition without the table: (global voxels [N, 3] of the nodes sorted by (z, y, x), for each the position in that
        order of the first node of its component)."""
        r, c = np.nonzero(self.node)
        g = np.array(self.keys, np.int64).reshape(-1, 3)[r] * 8 + LOCAL[c]
        o = np.lexsort((g[:, 0], g[:, 1], g[:, 2]))
        comp = self.index[r, c][o].astype(np.int64)
        first = np.full(len(self.records), len(o), np.int64)
        np.minimum.at(first, comp, np.arange(len(o)))
        return g[o], first[comp]


def _arrays(model, keys):
    if not keys:
        return np.zeros((0, 512), np.float32), np.zeros((0, 512), np.float32)
    return (np.stack([np.asarray(model[k][0], np.float32) for k in keys]),
            np.stack([np.asarray(model[k][1], np.float32) for k in keys]))


def edges(keys, node, connectivity):
    """Per offset o, the node pairs (id of A, id of A + o) [E] each.  Within one offset no id occurs twice on either side."""
    if connectivity not in OFFSETS:
        raise ValueError("connectivity must be 6 or 14")
    n = len(keys)
    rank = {k: i for i, k in enumerate(keys)}
    flat = node.reshape(-1)
    neighbour = {0: np.arange(n)}
    out = []
    for o in OFFSETS[connectivity]:
        q = LOCAL + np.array([o & 1, (o >> 1) & 1, o >> 2])
        cross = (q[:, 0] >> 3) | ((q[:, 1] >> 3) << 1) | ((q[:, 2] >> 3) << 2)
        u = ((q[:, 2] & 7) << 6) | ((q[:, 1] & 7) << 3) | (q[:, 0] & 7)
        a_all, b_all = [], []
        for d in np.unique(cross):
            d = int(d)
            if d not in neighbour:
                neighbour[d] = np.array([rank.get((k[0] + (d & 1), k[1] + ((d >> 1) & 1), k[2] + (d >> 2)), -1) for k in keys], np.int64)
            nb, sel = neighbour[d], cross == d
            have = nb >= 0                                   # an absent (or unlisted) neighbour block cuts
            a = (np.arange(n)[have, None] * 512 + V[sel][None, :]).reshape(-1)
            b = (nb[have, None] * 512 + u[sel][None, :]).reshape(-1)
            keep = flat[a] & flat[b]
            a_all.append(a[keep])
            b_all.append(b[keep])
        out.append((np.concatenate(a_all) if a_all else np.zeros(0, np.int64), np.concatenate(b_all) if b_all else np.zeros(0, np.int64)))
    return out


def label(model, order=None, target=INSIDE, connectivity=14, region=None):
    if target not in (INSIDE, OUTSIDE):
        raise ValueError("unknown target")
    keys = listed(model, order, region)
    if len(keys) > MAX_BLOCKS:
        raise ValueError("more than 2^23 - 1 listed blocks")
    sdf, weight = _arrays(model, keys)
    node = node_mask(sdf, weight, target)
    L = np.arange(node.size, dtype=np.int64)                 # a node's label: an id of its component, never above its own
    pairs = edges(keys, node, connectivity)
    ids = np.nonzero(node.reshape(-1))[0]
    while True:
        changed = False
        for a, b in pairs:
            la, lb = L[a], L[b]
            if (la != lb).any():
                changed = True
                m = np.minimum(la, lb)
                L[a] = m                                     # (no id twice in a, nor in b; one may be in both)
                L[b] = np.minimum(L[b], m)
        while True:                                          # every label replaced by its own label
            up = L[L[ids]]
            if (up == L[ids]).all():
                break
            L[ids] = up
        if not changed:
            break
    return Labelling(keys, node, L)


def label_plain(model, order=None, target=INSIDE, connectivity=14, region=None):
    """The textbook union-find over global voxels; returns the records.  For small models."""
    keys = listed(model, order, region)
    ident, parent = {}, {}
    for r, k in enumerate(keys):
        m = node_mask(model[k][0], model[k][1], target)
        for v in np.nonzero(m)[0]:
            g = (k[0] * 8 + (int(v) & 7), k[1] * 8 + ((int(v) >> 3) & 7), k[2] * 8 + (int(v) >> 6))
            ident[g] = r * 512 + int(v)
            parent[g] = g

    def find(g):
        while parent[g] != g:
            parent[g] = parent[parent[g]]
            g = parent[g]
        return g

    for g in list(parent):
        for o in OFFSETS[connectivity]:
            h = (g[0] + (o & 1), g[1] + ((o >> 1) & 1), g[2] + (o >> 2))
            if h in parent:
                a, b = find(g), find(h)
                if a != b:
                    if ident[a] < ident[b]:
                        parent[b] = a
                    else:
                        parent[a] = b
    size = {}
    for g in parent:
        r = find(g)
        size[r] = size.get(r, 0) + 1
    roots = sorted(size, key=lambda g: ident[g])
    out = np.zeros(len(roots), RECORD)
    for i, g in enumerate(roots):
        out[i] = (g, size[g])
    return out


def remove(model, min_size, order=None, target=INSIDE, connectivity=14, region=None):
    """vh_remove_components on the model: (the model afterwards, stats, cleared {key: bool[512]}, freed keys).  Every node of
    a component smaller than min_size becomes {0, 0}; a block in which a voxel was cleared and whose 512 weights are then all
    0 leaves the model; everything else keeps its bits."""
    lab = label(model, order, target, connectivity, region)
    small = lab.records["size"].astype(np.int64) < int(min_size)
    out = {k: (np.array(s, np.float32), np.array(w, np.float32)) for k, (s, w) in model.items()}
    cleared, freed = {}, []
    for r, k in enumerate(lab.keys):
        idx = lab.index[r]
        gone = lab.node[r] & small[np.where(lab.node[r], idx, 0).astype(np.int64)] if len(small) else np.zeros(512, bool)
        if gone.any():
            s, w = out[k]
            s[gone] = 0
            w[gone] = 0
            cleared[k] = gone
            if (w == 0).all():
                freed.append(k)
                del out[k]
    stats = dict(lab.stats)
    stats.update(removed_components=int(small.sum()), removed_voxels=int(lab.records["size"][small].sum()), freed_blocks=len(freed))
    return out, stats, cleared, freed
