"""The rule of vh_stream_out / vh_stream_in (include/voxelhash.h, "block streaming") in executable form: the
selection predicate one key at a time in numpy float32 scalars (every operation rounded on its own, in the header's order), the
two calls on a model kept as {key: (sdf[512], weight[512], colour[512])} (tests/merge_color_cases.py: model_of), and a
dict-backed stand-in for SDFHashtable that drives streaming.BlockStore without a GPU."""
import numpy as np

F = np.float32
U = np.uint32
BOX, SPHERE = 0, 1
PLACED, PRESENT, UNPLACED, FOREIGN = 0, 1, 2, 3
VOXEL = np.dtype([("sdf", "<f4"), ("weight", "<f4")])


def box(lo, hi, invert=False):
    return {"kind": BOX, "invert": invert, "lo": tuple(lo), "hi": tuple(hi)}


def sphere(centre, radius, invert=False):
    return {"kind": SPHERE, "invert": invert, "centre": tuple(centre), "radius": radius}


def selects(key, region, voxel_size):
    """Whether `region` selects the block `key` (three ints)."""
    if region["kind"] == BOX:
        inside = all(region["lo"][a] <= int(key[a]) < region["hi"][a] for a in range(3))
    else:
        vs = F(voxel_size)
        x = [F(F(F(F(8 * int(key[a])) + F(3.5)) * vs) - F(region["centre"][a])) for a in range(3)]
        d2 = F(F(F(x[0] * x[0]) + F(x[1] * x[1])) + F(x[2] * x[2]))
        r = F(region["radius"])
        inside = bool(d2 <= F(r * r))
    return inside != bool(region.get("invert", False))


def selected(keys, region, voxel_size):
    return np.array([selects(k, region, voxel_size) for k in np.asarray(keys).reshape(-1, 3).tolist()], bool)


def selection_of_table(table, region, voxel_size):
    """Entry indices of a downloaded hash table that the region selects, ascending: the order vh_stream_out writes in."""
    live = np.nonzero(table["ptr"] != -1)[0]
    return live[selected(table["pos"][live], region, voxel_size)]


def hash_block(key, num_buckets):
    """calculateHash (VoxelUtils.cu:250-259): the bucket of a block key."""
    x, y, z = (int(v) & 0xffffffff for v in key)
    return (((x * 73856093) ^ (y * 19349669) ^ (z * 83492791)) & 0xffffffff) % num_buckets


def chunk_of(model, keys, colors=True):
    """The records of `keys` as SDFHashtable.stream_out returns them."""
    vox = np.zeros((len(keys), 512), VOXEL)
    col = np.zeros((len(keys), 512), U)
    for i, k in enumerate(keys):
        vox["sdf"][i], vox["weight"][i], col[i] = model[k]
    return {"keys": np.asarray(keys, np.int32).reshape(-1, 3), "voxels": vox, "colors": col if colors else None, "selected": len(keys)}


def stream_out(model, region, voxel_size, capacity=None, colors=True):
    """(chunk, model afterwards).  A dict has no entry index: the order is that of the sorted keys."""
    keys = sorted(model)
    chosen = [k for k, s in zip(keys, selected(keys, region, voxel_size).tolist()) if s] if keys else []
    taken = chosen if capacity is None else chosen[:capacity]
    chunk = chunk_of(model, taken, colors)
    chunk["selected"] = len(chosen)
    return chunk, {k: v for k, v in model.items() if k not in set(taken)}


def stream_in(model, chunk, room=None, refuse=(), bucket_range=None, num_buckets=None):
    """(status [n], model afterwards).  room: free blocks of the pool (None = enough); refuse: keys whose bucket is full;
    bucket_range with num_buckets: the shard's buckets (keys outside are FOREIGN)."""
    out = dict(model)
    cols = chunk.get("colors")
    status = []
    for i, k in enumerate(map(tuple, np.asarray(chunk["keys"]).reshape(-1, 3).tolist())):
        if bucket_range is not None and not bucket_range[0] <= hash_block(k, num_buckets) < bucket_range[1]:
            status.append(FOREIGN)
        elif k in out:
            status.append(PRESENT)
        elif k in refuse or (room is not None and room <= 0):
            status.append(UNPLACED)
        else:
            v = chunk["voxels"][i]
            out[k] = (v["sdf"].copy(), v["weight"].copy(), np.zeros(512, U) if cols is None else np.array(cols[i], U))
            room = None if room is None else room - 1
            status.append(PLACED)
    return np.array(status, np.int32), out


def same_models(a, b):
    assert a.keys() == b.keys(), (len(a), len(b), sorted(set(a) ^ set(b))[:4])
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(np.asarray(x).view(U), np.asarray(y).view(U)), k


class DictTable:
    """What streaming.BlockStore needs of an SDFHashtable, on a dict model: stream_out(region) and stream_in(chunk)."""

    def __init__(self, model, voxel_size, pool=None, refuse=()):
        self.model, self.voxel_size, self.pool, self.refuse = dict(model), voxel_size, pool, set(refuse)

    def stream_out(self, region, capacity=None, colors=None):
        chunk, self.model = stream_out(self.model, region, self.voxel_size, capacity, colors is None or colors)
        return chunk

    def stream_in(self, chunk):
        room = None if self.pool is None else self.pool - len(self.model)
        status, self.model = stream_in(self.model, chunk, room, self.refuse)
        st = {n: int(np.sum(status == c)) for n, c in (("placed", PLACED), ("present", PRESENT), ("unplaced", UNPLACED), ("foreign", FOREIGN))}
        st["rounds"] = 1
        st["status"] = status
        return st
