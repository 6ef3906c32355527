"""The rule of the block silhouettes (include/voxelhash.h: vh_render_blocks), with no culling of any kind.

Plain numpy float32 and nothing of the product or the oracle: every block is tested against every pixel by the ray/box test the
header describes, in the order of operations of ray_box (csrc/vh_blocks.hip, oracle/vh_oracle.c).  There is no screen box, no
depth pre-test and no block list, so whatever those get wrong in an implementation shows as a difference from this file.

    cube of block k        lo = float(int32(8 k)) * vs,  hi = (float(int32(8 k)) + 8) * vs           per axis
    ray of pixel (px, py)  o = pose[:3, 3],  d[a] = (pose[a, 0] * dx + pose[a, 1] * dy) + pose[a, 2]
                           dx = (float(px) - cx) / fx,  dy = (float(py) - cy) / fy                    (d is per unit camera depth)
    per axis               d[a] == 0: the ray misses unless lo[a] <= o[a] <= hi[a]
                           else t0 = (lo[a] - o[a]) / d[a], t1 = (hi[a] - o[a]) / d[a],
                                tNear = fmax(tNear, fmin(t0, t1)),  tFar = fmin(tFar, fmax(t0, t1))
    hit                    tNear <= tFar;  kept unless tFar < t_min or tNear > t_max
    images                 front = min over the kept blocks of fmax(tNear, t_min) + 0,  back = max of fmin(tFar, t_max) + 0,
                           both 0 where no block is kept

render() also returns, per block, the mask of the pixels that keep it: the conditions of tests/blocks_cases.py (how many blocks
a view keeps, how many a 16x16 region keeps, which pixels are empty) are functions of that mask alone."""
import numpy as np

F = np.float32
U = np.uint32
BIG = F(3.0e38)


def cubes(keys, voxel_size):
    """(lo, hi) [N, 3] float32 of the blocks' cubes; 8 * key wraps in int32 as the table's arithmetic does."""
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    k8 = ((k * 8 + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32).astype(F)
    vs = F(voxel_size)
    return k8 * vs, (k8 + F(8.0)) * vs


def directions(W, H, fx, fy, cx, cy, pose):
    """d [3, H, W] float32: the ray direction of every pixel per unit camera depth."""
    pose = np.asarray(pose, F).reshape(4, 4)
    dx = ((np.arange(W, dtype=np.int32).astype(F) - F(cx)) / F(fx))[None, :]
    dy = ((np.arange(H, dtype=np.int32).astype(F) - F(cy)) / F(fy))[:, None]
    return np.stack([(pose[a, 0] * dx + pose[a, 1] * dy) + pose[a, 2] for a in range(3)])


def render(keys, voxel_size, W, H, fx, fy, cx, cy, pose, t_min, t_max, batch=64):
    """(front [H, W] float32, back [H, W] float32, kept [N, H, W] bool)."""
    pose = np.asarray(pose, F).reshape(4, 4)
    lo, hi = cubes(keys, voxel_size)
    n = len(lo)
    d = directions(W, H, fx, fy, cx, cy, pose).reshape(3, 1, H * W)
    o = pose[:3, 3]
    t_min, t_max = F(t_min), F(t_max)
    front = np.full(H * W, np.inf, F)
    back = np.zeros(H * W, F)
    kept = np.zeros((n, H * W), bool)
    with np.errstate(all="ignore"):
        for b in range(0, n, batch):
            l, h = lo[b:b + batch], hi[b:b + batch]
            m = len(l)
            t_near = np.full((m, H * W), -BIG, F)
            t_far = np.full((m, H * W), BIG, F)
            hit = np.ones((m, H * W), bool)
            for a in range(3):
                zero = d[a] == 0                                                            # [1, P]
                inside = ~((o[a] < l[:, a]) | (o[a] > h[:, a]))[:, None]                     # [m, 1]
                t0, t1 = (l[:, a, None] - o[a]) / d[a], (h[:, a, None] - o[a]) / d[a]
                t_near = np.where(zero, t_near, np.fmax(t_near, np.fmin(t0, t1)))
                t_far = np.where(zero, t_far, np.fmin(t_far, np.fmax(t0, t1)))
                hit &= ~zero | inside
            keep = hit & (t_near <= t_far) & ~((t_far < t_min) | (t_near > t_max))
            f = np.where(keep, np.fmax(t_near, t_min) + F(0.0), F(np.inf))
            k = np.where(keep, np.fmin(t_far, t_max) + F(0.0), F(0.0))
            front = np.minimum(front, f.min(0))
            back = np.maximum(back, k.max(0))
            kept[b:b + m] = keep
    front[np.isinf(front)] = F(0.0)
    return front.reshape(H, W), back.reshape(H, W), kept.reshape(n, H, W)


def render_scalar(keys, voxel_size, W, H, fx, fy, cx, cy, pose, t_min, t_max):
    """The same rule as nested loops over pixels and blocks, one numpy float32 scalar at a time (for tiny cases: it pins render)."""
    pose = np.asarray(pose, F).reshape(4, 4)
    lo, hi = cubes(keys, voxel_size)
    front, back = np.zeros((H, W), F), np.zeros((H, W), F)
    kept = np.zeros((len(lo), H, W), bool)
    o = [pose[a, 3] for a in range(3)]
    t_min, t_max = F(t_min), F(t_max)
    with np.errstate(all="ignore"):
        for py in range(H):
            for px in range(W):
                dx, dy = (F(px) - F(cx)) / F(fx), (F(py) - F(cy)) / F(fy)
                d = [(pose[a, 0] * dx + pose[a, 1] * dy) + pose[a, 2] for a in range(3)]
                best_f, best_b = F(np.inf), F(0.0)
                for i in range(len(lo)):
                    tn, tf, miss = -BIG, BIG, False
                    for a in range(3):
                        if d[a] == 0:
                            if o[a] < lo[i, a] or o[a] > hi[i, a]:
                                miss = True
                                break
                            continue
                        t0, t1 = (lo[i, a] - o[a]) / d[a], (hi[i, a] - o[a]) / d[a]
                        tn, tf = max(tn, min(t0, t1)), min(tf, max(t0, t1))
                    if miss or not tn <= tf or tf < t_min or tn > t_max:
                        continue
                    kept[i, py, px] = True
                    f, k = max(tn, t_min) + F(0.0), min(tf, t_max) + F(0.0)
                    if f < best_f:
                        best_f = f
                    if k > best_b:
                        best_b = k
                front[py, px] = best_f if best_f != np.inf else F(0.0)
                back[py, px] = best_b
    return front, back, kept


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


# ---- facts about a view, from the masks alone ------------------------------------------------------------------------
def kept_blocks(kept):
    """How many blocks at least one pixel keeps."""
    return int(kept.any(axis=(1, 2)).sum())


def region_counts(kept, size=16):
    """[ceil(H / size), ceil(W / size)]: the blocks that at least one pixel of each size x size region keeps."""
    n, H, W = kept.shape
    out = np.zeros(((H + size - 1) // size, (W + size - 1) // size), np.int64)
    for ry in range(out.shape[0]):
        for rx in range(out.shape[1]):
            out[ry, rx] = kept[:, ry * size:(ry + 1) * size, rx * size:(rx + 1) * size].any(axis=(1, 2)).sum()
    return out


def alone_somewhere(kept):
    """[N] bool: the block is the only one kept at some pixel (without it that pixel of both images changes)."""
    single = kept.sum(0) == 1
    return (kept & single[None]).any(axis=(1, 2))
