"""Crafted depth and stored voxels for the TSDF update (tsdf_apply, vh_integrate.hip), shared by tests/test_tsdf_cases_cpu.py
(the oracle against tests/deintegrate_ref.py, and the coverage of the inputs) and tests/test_gpu_tsdf_crafted.py.

A CASE is one table: its parameters, semantics, projection, integrate flags, the blocks it is loaded with ({key: (sdf[512],
weight[512])}) and one or more FRAMES (a pose, an allocation vertex map, a depth source).  The projection has a focal length of
two pixels (band_cases.wide), so the few dozen blocks next to the camera meet every pixel of a 48x32 or 33x17 image, and the
voxels of one block read many different pixels.

The camera of the families a, b, d and e looks along -z of the world from z = 0.425: the ORIGIN of a block, which the frustum
test judges, is then its far corner, the block is listed, and its voxels reach camera depths down to 0.075 and image columns
and rows beyond all four sides.

Family a, STORED: finite stored weights and sdf of every size against ordinary depth; the weight cap from below, at and above.
Family b, DEPTH: special finite values in the depth plane; sdf exactly -trunc, 0, +trunc and one ulp beside -trunc.
Family c, PROJECTION: the camera inside a block, quotients at the image's edges, index truncation under REFERENCE semantics.
Family d, NON-FINITE: NaN and infinities in the plane and in the stored voxels (step-level update and removal only).
Family e, SENSOR: uint16 images with a K^-1 whose third row differs from pixel to pixel.
Family f, SEQUENCE: three frames with different poses and planes over partly the same blocks.
Family r, REMOVAL: 64x48 variants of a, b and d for vh_deintegrate, with stored weights that leave wFloor and its neighbours."""
import itertools
from types import SimpleNamespace

import numpy as np

import deintegrate_ref as R

F = np.float32
I4 = np.eye(4, dtype=F)
ENTRY_DTYPE = np.dtype([("pos", "<i4", (3,)), ("ptr", "<i4"), ("offset", "<i4")])
VOXEL_DTYPE = np.dtype([("sdf", "<f4"), ("weight", "<f4")])
NAN, INF = float("nan"), float("inf")
VS, TRUNC = 0.05, 0.3
CW = F(0.1)                                                # the sample weight without the weight-sample flag


def up(v):
    return F(np.nextafter(F(v), F(np.inf)))


def dn(v):
    return F(np.nextafter(F(v), F(-np.inf)))


def wide(W, H):
    return np.array((2, 0, W / 2, 0, 2, H / 2, 0, 0, 1), F)


def flip_pose(t=(0.01, -0.015, 0.425), yaw_deg=0.0):
    """Camera -> world: the camera looks along -z of the world (a half turn about x, then a yaw), from t."""
    a = np.radians(yaw_deg)
    c, s = np.cos(a), np.sin(a)
    yaw = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    T = np.eye(4)
    T[:3, :3] = yaw @ np.diag([1.0, -1.0, -1.0])
    T[:3, 3] = t
    return T.astype(F)


def ring(xs, ys, zs):
    return [k for k in itertools.product(xs, ys, zs)]


RING = ring(range(-3, 3), range(-2, 2), (-1, 0))           # 48 blocks around the flipped camera


class Frame:
    """pose; verts [H, W, 4]: what allocation sees, and -- its .z -- the depth of the whole-frame forms; plane [H, W]: a depth
    that only the step-level update and the removal are given (family d), else None; sensor: (uint16 [H, W], K^-1 [9]), else None."""

    def __init__(self, pose, verts, plane=None, sensor=None):
        self.pose = np.ascontiguousarray(np.asarray(pose, F).reshape(4, 4))
        self.verts, self.plane, self.sensor = verts, plane, sensor

    def depth_source(self):
        if self.sensor is not None:
            return self.sensor
        return self.plane if self.plane is not None else self.verts[..., 2]

    def depth_verts(self):
        """The float4 map the step-level update and the removal read their depth from."""
        if self.plane is None:
            return self.verts
        v = self.verts.copy()
        v[..., 2] = self.plane
        return v


class Case:
    def __init__(self, name, family, W, H, sem, flags, blocks, frames, proj=None, table=None, **kw):
        self.name, self.family, self.W, self.H, self.sem, self.flags = name, family, W, H, sem, flags
        self.proj = wide(W, H) if proj is None else np.asarray(proj, F)
        self.table = dict(numBuckets=1 << 11, numVoxelBlocks=256)
        self.table.update(table or {})
        self.kw = dict(voxelSize=VS, truncation=TRUNC, truncScale=0.05, integrationWeightSample=1, integrationWeightMax=0.25)
        self.kw.update(kw)
        self.blocks, self.frames = blocks, frames
        self.whole_frame = family != "d" and family != "r"
        self.marks = {}                                    # what the generator aimed at: {tag: [(block index, voxel)]}

    def params(self, module):
        return module.default_params(**self.table, **self.kw)

    @property
    def rule_params(self):
        return SimpleNamespace(**self.kw)

    def entries(self):
        """The loaded blocks as VoxelEntry records of a volume of their own: block i at voxel 512 * i."""
        e = np.zeros(len(self.blocks), ENTRY_DTYPE)
        e["pos"] = np.array(list(self.blocks), np.int32).reshape(-1, 3)
        e["ptr"] = 512 * np.arange(len(self.blocks))
        return e

    def volume(self):
        v = np.zeros(512 * len(self.blocks), VOXEL_DTYPE)
        for i, (s, w) in enumerate(self.blocks.values()):
            v["sdf"][512 * i:512 * i + 512], v["weight"][512 * i:512 * i + 512] = s, w
        return v

    def chunk(self):
        """What SDFHashtable.stream_in takes."""
        vol = self.volume().reshape(-1, 512)
        return {"keys": np.array(list(self.blocks), np.int32).reshape(-1, 3), "voxels": vol}


def trace(entries, params, sem, proj, pose_inv, depth_source, flags):
    """The sample computation of deintegrate_ref.frame_samples with its intermediate values kept, [n, 512] each: cz, the
    quotients qx, qy of the projection, the pixel sx, sy, inb (inside the image), depth (0 where not inb), raw (depth - cz),
    trunc, ok, s, cw.  Checked against frame_samples itself."""
    plane = depth_source[0] if isinstance(depth_source, tuple) else depth_source
    height, width = np.asarray(plane).shape[:2]
    n = len(entries)
    lin = np.arange(512)
    tx, ty, tz = lin & 7, (lin >> 3) & 7, lin >> 6
    base = R._wrap_i32(entries["pos"].astype(np.int64) * 8).reshape(n, 3)
    vx, vy, vz = [R._wrap_i32(base[:, a:a + 1].astype(np.int64) + t[None, :]).astype(F) for a, t in enumerate((tx, ty, tz))]
    vs = F(params.voxelSize)
    if sem == R.SEM_REFERENCE:
        cx, cy, cz = [R.f2i_rz(c).astype(F) * vs for c in R._mat4_rows(pose_inv, vx, vy, vz)]
    else:
        cx, cy, cz = R._mat4_rows(pose_inv, vx * vs, vy * vs, vz * vs)
    p = np.asarray(proj, F).reshape(9)
    with np.errstate(all="ignore"):
        qz = (p[6] * cx + p[7] * cy) + p[8] * cz
        qx, qy = ((p[0] * cx + p[1] * cy) + p[2] * cz) / qz, ((p[3] * cx + p[4] * cy) + p[5] * cz) / qz
        sx, sy = R.f2i_rz(qx), R.f2i_rz(qy)
        inb = (sx >= 0) & (sx < width) & (sy >= 0) & (sy < height)
        depth = np.where(inb, R._depth_at(depth_source, np.where(inb, sx, 0), np.where(inb, sy, 0)), F(0)).astype(F)
        raw = depth - cz
        trunc = np.full(raw.shape, F(params.truncation), F)
        if flags & R.FLAG_DEPTH_TRUNCATION:
            trunc = F(params.truncation) + (F(params.truncScale) * depth)
    ok, s, cw = R.frame_samples(entries, params, sem, proj, pose_inv, depth_source, flags)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(ok, inb & ~(depth <= F(0)) & (raw > -trunc))
    return dict(cz=cz, qx=qx, qy=qy, sx=sx, sy=sy, inb=inb, depth=depth, raw=raw, trunc=trunc, ok=ok, s=s, cw=cw)


def alloc_map(plane, W, H, focal=40.0):
    """A vertex map whose .z is `plane` (finite): x and y as a camera of focal length `focal` pixels would give them, so the
    points of one frame fall into a few dozen blocks; 0 where |z| is beyond 1e30."""
    z = np.asarray(plane, F)
    py, px = np.mgrid[0:H, 0:W]
    v = np.zeros((H, W, 4), F)
    tame = np.abs(z) < 1e30
    v[..., 0] = np.where(tame, z * ((px - W / 2) / focal).astype(F), F(0))
    v[..., 1] = np.where(tame, z * ((py - H / 2) / focal).astype(F), F(0))
    v[..., 2], v[..., 3] = z, 1.0
    assert np.isfinite(v).all()
    return v


def ordinary_plane(rng, W, H, lo=0.05, hi=0.95):
    return rng.uniform(lo, hi, (H, W)).astype(F)


def draw_blocks(rng, keys, weights, sdfs, p_rare=None):
    """Every voxel of every block draws its weight and its sdf from the lists, independently."""
    out = {}
    for k in keys:
        w = np.asarray(weights, F)[rng.integers(0, len(weights), 512)]
        s = np.asarray(sdfs, F)[rng.integers(0, len(sdfs), 512)]
        out[tuple(k)] = (s, w)
    return out


def read_pixels(case, frame, inv):
    """[(x, y)] of the pixels at least one voxel of the loaded blocks reads, most-read first."""
    t = trace(case.entries(), case.rule_params, case.sem, case.proj, inv, frame.depth_source(), case.flags)
    flat = (t["sy"][t["inb"]].astype(np.int64) * case.W + t["sx"][t["inb"]])
    count = np.bincount(flat, minlength=case.W * case.H)
    order = np.argsort(-count, kind="stable")
    return [(int(i % case.W), int(i // case.W)) for i in order if count[i] > 0]


def scatter(plane, pixels, values, every=3, start=0):
    """values, in turn, onto every `every`-th of `pixels`; returns {value index: [pixels]}."""
    where = {}
    for j, xy in enumerate(pixels[start::every]):
        i = j % len(values)
        plane[xy[1], xy[0]] = values[i]
        where.setdefault(i, []).append(xy)
    return where


# ---------------------------------------------------------------------------
# the lists of the issue
# ---------------------------------------------------------------------------
SUB, SUB_BIG = F(1e-45), F(1e-40)                          # the smallest subnormal and an ordinary one
A_WEIGHTS_CAP025 = [0.0, -0.0, CW, F(0.25), F(0.25) - CW, 0.3, 2.95, 2.0 ** 21, 2.0 ** 24, 3e38, SUB, SUB_BIG, 0.2]
A_WEIGHTS_CAP3 = [0.0, -0.0, 1.0, 3.0, 1.5, 2.0, 2.95, 3.5, 2.0 ** 21, 2.0 ** 24, 3e38, SUB, SUB_BIG, 0.1]
A_SDFS = [0.0, -0.0, TRUNC, -TRUNC, SUB, -SUB, SUB_BIG, -SUB_BIG, 3e38, -3e38, 0.01]
B_DEPTHS = [0.0, -0.0, -1.0, -SUB, SUB, SUB_BIG, 1e-38, 3e38, 0.5, 5.0, 5.5, 40.0, TRUNC, up(TRUNC), dn(TRUNC), 1.0, 1.3, 2.0]
D_DEPTHS = [NAN, INF, -INF, 0.0, -0.0, -1.0, SUB, 1e-38, 3e38, 0.5, 5.0, 40.0, TRUNC]
D_WEIGHTS = [INF, NAN, -0.1, 3e38, 2.0 ** 21, SUB, 1e-30]
D_SDFS = [INF, -INF, NAN, 3e38, -3e38, SUB, -SUB]
ORD_WEIGHTS, ORD_SDFS = [0.0, 0.1, 0.2, 0.25, 0.3], [0.0, -0.0, 0.3, -0.3, 0.01, -0.12, 0.2]


def family_a(W=48, H=32, family="a"):
    out = []
    for name, flags, cap, weights, seed in (("cap025", 0, 0.25, A_WEIGHTS_CAP025, 11), ("cap3-weight-sample", 2, 3.0, A_WEIGHTS_CAP3, 12),
                                            ("cap3-both-flags", 3, 3.0, A_WEIGHTS_CAP3, 13)):
        rng = np.random.default_rng(seed)
        plane = ordinary_plane(rng, W, H)
        plane[rng.random((H, W)) < 0.15] = 0.0              # holes: cells of which one voxel changes
        if flags & 2:
            plane[rng.random((H, W)) < 0.1] = 2.5           # cw clamps to 1 there: 2.0 + 1.0 is the cap exactly
        c = Case(f"{family}-{name}-{W}x{H}", family, W, H, 1, flags, draw_blocks(rng, RING, weights, A_SDFS),
                 [Frame(flip_pose(), alloc_map(plane, W, H))], integrationWeightMax=cap)
        c.weights, c.sdfs = weights, A_SDFS
        out.append(c)
    return out


def solve_depth(cz, target):
    """A positive fp32 depth d with fl(d - cz) == target, bit for bit; None if there is none within a few ulps."""
    cz, target = F(cz), F(target)
    d = F(cz + target)
    cands = [d]
    lo = hi = d
    for _ in range(6):
        lo, hi = dn(lo), up(hi)
        cands += [lo, hi]
    for c in cands:
        if c > 0 and F(c - cz).tobytes() == target.tobytes():
            return c
    return None


EXACT_TARGETS = (("raw==-trunc", F(-TRUNC), False), ("raw==-trunc+ulp", up(-TRUNC), True), ("raw==-trunc-ulp", dn(-TRUNC), False),
                 ("raw==0", F(0.0), True), ("raw==+trunc", F(TRUNC), True), ("raw==+trunc+ulp", up(TRUNC), True))


def family_b(W=48, H=32, family="b", all_flags=True, weights=ORD_WEIGHTS):
    out = []
    inv = np.linalg.inv(flip_pose().astype(np.float64)).astype(F)          # (only to choose pixels; the tests use the library's inverse)
    for flags in (0, 1, 2, 3) if all_flags else (0, 3):
        rng = np.random.default_rng(20 + flags)
        plane = ordinary_plane(rng, W, H)
        c = Case(f"{family}-flags{flags}-{W}x{H}", family, W, H, 1, flags, draw_blocks(rng, RING, weights, ORD_SDFS),
                 [Frame(flip_pose(), None)], integrationWeightMax=3.0, integrationWeightSample=2)
        c.frames[0].verts = alloc_map(plane, W, H)
        pixels = read_pixels(c, c.frames[0], inv)
        c.special = scatter(plane, pixels, B_DEPTHS, every=3, start=1)
        c.depths = B_DEPTHS
        if flags == 0:
            # one voxel per target: its pixel (one no other target has, and none of the special ones) gets the depth made for it
            t = trace(c.entries(), c.rule_params, 1, c.proj, inv, plane, flags)
            taken = {xy for v in c.special.values() for xy in v}
            cand = np.argwhere(t["inb"] & (t["cz"] > F(TRUNC + 0.02)))
            rng.shuffle(cand)
            want = [(tag, tgt, ok) for tag, tgt, ok in EXACT_TARGETS for _ in range(4)]
            for b, v in cand:
                if not want:
                    break
                xy = (int(t["sx"][b, v]), int(t["sy"][b, v]))
                if xy in taken:
                    continue
                tag, tgt, ok = want[0]
                d = solve_depth(t["cz"][b, v], tgt)
                if d is None:
                    continue
                plane[xy[1], xy[0]] = d
                taken.add(xy)
                c.marks.setdefault(tag, []).append((int(b), int(v), ok))
                want.pop(0)
            assert not want, want
        c.frames[0].verts = alloc_map(plane, W, H)
        if flags == 0:                                                      # the targets fall where they were aimed
            t = trace(c.entries(), c.rule_params, 1, c.proj, inv, plane, flags)
            for tag, tgt, _ in EXACT_TARGETS:
                for b, v, ok in c.marks[tag]:
                    assert t["raw"][b, v].tobytes() == F(tgt).tobytes() and bool(t["ok"][b, v]) == ok, (tag, b, v)
        out.append(c)
    return out


# ---------------------------------------------------------------------------
# family c
# ---------------------------------------------------------------------------
VS4 = 2.0 ** -4                                            # dyadic: camera coordinates and quotients of the pinhole cases are exact


def family_c():
    out = []
    for W, H, xs, ys in ((48, 32, range(-6, 6), range(-4, 5)), (33, 17, range(-5, 5), range(-6, 6))):
        rng = np.random.default_rng(W)
        keys = ring(xs, ys, (-1, 0))
        plane = ordinary_plane(rng, W, H, 0.05, 0.9)
        plane[0, 0] = 0.2                                                   # the voxel at the camera centre reads pixel (0, 0)
        plane[rng.random((H, W)) < 0.1] = 0.0
        plane[0, 0] = 0.2
        c = Case(f"c-pinhole-{W}x{H}", "c", W, H, 1, 0, draw_blocks(rng, keys, ORD_WEIGHTS, ORD_SDFS),
                 [Frame(flip_pose((0.0, 0.0, 0.25)), alloc_map(plane, W, H))], table=dict(numBuckets=1 << 12, numVoxelBlocks=512),
                 voxelSize=VS4, truncation=0.25, integrationWeightMax=3.0)
        out.append(c)
    # REFERENCE semantics: the inverse pose acts on the voxel INDEX and the result is truncated towards zero
    perm = np.eye(4, dtype=F)
    perm[:3, 3] = (0.5, -0.5, 1.0)                                          # indices land on k + 0.5 and on whole numbers
    from voxelhashing_demo_amd import synth
    for name, W, H, pose in (("yaw", 48, 32, synth.yaw_pose(5.0, (0.1, 0.0, 0.05))), ("half-shift", 33, 17, perm)):
        rng = np.random.default_rng(H)
        keys = ring(range(-2, 2), range(-2, 2), (0, 1))
        plane = ordinary_plane(rng, W, H, 0.05, 0.9)
        plane[rng.random((H, W)) < 0.1] = 0.0
        c = Case(f"c-reference-{name}-{W}x{H}", "c", W, H, 0, 0, draw_blocks(rng, keys, ORD_WEIGHTS, ORD_SDFS),
                 [Frame(pose, alloc_map(plane, W, H))], integrationWeightMax=3.0)
        out.append(c)
    return out


# ---------------------------------------------------------------------------
# family d
# ---------------------------------------------------------------------------
def family_d(W=48, H=32, family="d", weights_extra=()):
    out = []
    inv = np.linalg.inv(flip_pose().astype(np.float64)).astype(F)
    for flags in (0, 3):
        rng = np.random.default_rng(40 + flags)
        blocks = draw_blocks(rng, RING, ORD_WEIGHTS + list(weights_extra), ORD_SDFS)
        for s, w in blocks.values():                                        # one voxel in ten holds something rare
            rare = rng.random(512) < 0.1
            w[rare] = np.asarray(D_WEIGHTS, F)[rng.integers(0, len(D_WEIGHTS), int(rare.sum()))]
            rare = rng.random(512) < 0.1
            s[rare] = np.asarray(D_SDFS, F)[rng.integers(0, len(D_SDFS), int(rare.sum()))]
        tame = ordinary_plane(rng, W, H)
        c = Case(f"{family}-flags{flags}-{W}x{H}", family, W, H, 1, flags, blocks, [Frame(flip_pose(), alloc_map(tame, W, H))],
                 integrationWeightMax=3.0, integrationWeightSample=2)
        plane = tame.copy()
        c.special = scatter(plane, read_pixels(c, c.frames[0], inv), D_DEPTHS, every=4, start=1)
        c.depths, c.weights, c.sdfs = D_DEPTHS, D_WEIGHTS, D_SDFS
        c.frames[0].plane = plane
        out.append(c)
    return out


# ---------------------------------------------------------------------------
# family e
# ---------------------------------------------------------------------------
def sensor_k_inv(W, H):
    """A K^-1 whose third row makes pz differ from pixel to pixel, 1 + 0.001 x - 0.002 y > 0.9 (the update reads only that
    row); rows 0 and 1, which allocation reads, are those of a focal length of 40 pixels: a frame's points fall into a few
    dozen blocks."""
    return np.array((1 / 40, 0, -W / 80, 0, 1 / 40, -H / 80, 0.001, -0.002, 1.0), F)


def family_e(oracle, W=48, H=32, family="e", weights=ORD_WEIGHTS):
    out = []
    for flags in (0, 3):
        rng = np.random.default_rng(50 + flags)
        d16 = rng.integers(300, 2500, (H, W)).astype(np.uint16)            # 0.06 .. 0.5 m
        if family != "e" and flags & 2:
            d16[rng.random((H, W)) < 0.2] = 20000                           # 4 m: cw clamps to 1
        kinv = sensor_k_inv(W, H)
        c = Case(f"{family}-flags{flags}-{W}x{H}", family, W, H, 1, flags, draw_blocks(rng, RING, weights, ORD_SDFS),
                 [Frame(flip_pose(), np.zeros((H, W, 4), F), sensor=(d16, kinv))], table=dict(numBuckets=1 << 12, numVoxelBlocks=1024),
                 integrationWeightMax=3.0, integrationWeightSample=2)
        inv = np.linalg.inv(flip_pose().astype(np.float64)).astype(F)
        c.depths = [0, 1, 65535]
        c.special = scatter(d16, read_pixels(c, c.frames[0], inv), c.depths, every=5, start=1)
        c.frames[0].verts = oracle.preprocess(d16, kinv)[0]                 # what vh_integrate_depth allocates from
        assert (R._depth_at((d16, kinv), *np.mgrid[0:H, 0:W][::-1]) >= 0).all()
        out.append(c)
    return out


# ---------------------------------------------------------------------------
# family f
# ---------------------------------------------------------------------------
def family_f():
    return _family_f(48, 32) + _family_f(33, 17)


def _family_f(W, H):
    out = []
    poses = [flip_pose(), flip_pose((0.08, -0.03, 0.47), 8.0), flip_pose((-0.06, 0.02, 0.52), -6.0)]
    for flags in (0, 3):
        rng = np.random.default_rng(60 + flags + W)
        frames = []
        for k, pose in enumerate(poses):
            plane = ordinary_plane(rng, W, H, 0.1 + 0.3 * k, 0.8 + 0.5 * k)  # later frames look farther: new blocks
            plane[rng.random((H, W)) < 0.1] = 0.0
            frames.append(Frame(pose, alloc_map(plane, W, H, focal=30.0)))
        c = Case(f"f-flags{flags}-{W}x{H}", "f", W, H, 1, flags, draw_blocks(rng, RING, ORD_WEIGHTS, ORD_SDFS), frames,
                 table=dict(numBuckets=1 << 12, numVoxelBlocks=512), integrationWeightMax=0.45, integrationWeightSample=2)
        out.append(c)
    return out


# ---------------------------------------------------------------------------
# family r: the removal, at 64x48
# ---------------------------------------------------------------------------
W_FLOOR = {0: F(0.05), 2: F(0.5)}


def family_r(oracle):
    """a, b, d and e at the removal's image size.  The stored weights gain those that leave wFloor after the sample is taken out:
    with the weight-sample flag cw clamps to 1 at depths of 2 m and more and 1.5 - 1 is the floor exactly; without it
    ow - 0.1f is an odd multiple of 2^-27 for every fp32 ow next to 0.15 and 0.05f is an odd multiple of 2^-28, so the
    floor itself cannot be left and the two weights that leave its neighbours stand in."""
    near = [F(1.5), up(1.5), dn(1.5), F(0.15), up(0.15), dn(0.15), dn(dn(0.15))]
    out = []
    for c in family_a(64, 48, "r-a"):
        rng = np.random.default_rng(len(out))
        c.blocks = draw_blocks(rng, RING, list(c.weights) + near, A_SDFS)
        c.weights = list(c.weights) + near
        if c.flags & 2:                                                     # depths at which cw is 1
            plane = c.frames[0].verts[..., 2].copy()
            plane[rng.random(plane.shape) < 0.3] = 2.5
            c.frames[0].verts = alloc_map(plane, 64, 48)
        out.append(c)
    out += family_b(64, 48, "r-b", all_flags=False, weights=ORD_WEIGHTS + [1.5, 2.0, 2.95, 20.0])
    out += family_d(64, 48, "r-d", weights_extra=near)
    out += family_e(oracle, 64, 48, "r-e", weights=ORD_WEIGHTS + near + [2.0, 2.95])
    for c in out:
        c.family, c.whole_frame = "r", False
    return out


_cache = {}


def cases(oracle, family):
    if family not in _cache:
        make = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": lambda: family_e(oracle), "f": family_f,
                "r": lambda: family_r(oracle)}[family]
        _cache[family] = make()
    return _cache[family]


FAMILIES = "abcdefr"


def names(family):
    """Case names without building the oracle (for parametrize)."""
    if family == "e":
        return [f"e-flags{f}-48x32" for f in (0, 3)]
    if family == "r":
        return ([f"r-a-{n}-64x48" for n in ("cap025", "cap3-weight-sample", "cap3-both-flags")] +
                [f"r-{x}-flags{f}-64x48" for x in "bde" for f in (0, 3)])
    return [c.name for c in cases(None, family)]


def case(oracle, name):
    for f in FAMILIES:
        if name.startswith(f + "-"):
            return {c.name: c for c in cases(oracle, f)}[name]
    raise KeyError(name)


def _tiled_frame(oracle, f, W, H, pose, shift):
    """Frame f's plane (or sensor image) rolled by `shift` pixels and tiled over a W x H image, seen from `pose`."""
    h, w = f.verts.shape[:2]
    reps = (-(-H // h), -(-W // w))
    if f.sensor is not None:
        d16 = np.ascontiguousarray(np.tile(np.roll(f.sensor[0], shift, (0, 1)), reps)[:H, :W])
        # a long focal length in rows 0 and 1, which only allocation reads; pz = 1 + 0.0001 x - 0.0002 y > 0.95
        kinv = np.array((1 / 2000, 0, -W / 4000, 0, 1 / 2000, -H / 4000, 0.0001, -0.0002, 1.0), F)
        return Frame(pose, oracle.preprocess(d16, kinv)[0], sensor=(d16, kinv))
    plane = np.ascontiguousarray(np.tile(np.roll(f.verts[..., 2], shift, (0, 1)), reps)[:H, :W])
    return Frame(pose, alloc_map(plane, W, H, focal=2000.0))


SECOND_CAMERA = flip_pose((0.05, -0.02, 0.45), 7.0)


def multi_camera(oracle, c, W, H, batch):
    """The case as `batch` multi-camera frames of two cameras on a W x H image: a copy of the case whose .steps[b] are the
    two cameras' Frames.  A one-frame case gives camera 0 its own frame and camera 1 the same plane shifted, from another
    pose (the two swap in the second step); a three-frame case gives step b the frames b and b + 1."""
    t = Case(f"{c.name}-two-cameras-{W}x{H}-batch{batch}", c.family, W, H, c.sem, c.flags, c.blocks, [],
             table=dict(numBuckets=1 << 12, numVoxelBlocks=1024), **c.kw)
    t.steps = []
    for b in range(batch):
        if len(c.frames) >= 3:
            pair = [(c.frames[b], c.frames[b].pose, (0, 0)), (c.frames[b + 1], c.frames[b + 1].pose, (0, 0))]
        else:
            f = c.frames[0]
            pair = [(f, f.pose, (3 * b, 5 * b)), (f, SECOND_CAMERA, (7 + b, 11 + b))][::1 if b == 0 else -1]
        t.steps.append([_tiled_frame(oracle, f, W, H, pose, shift) for f, pose, shift in pair])
    t.frames = [f for step in t.steps for f in step]
    return t
