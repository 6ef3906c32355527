"""Crafted pixels for band allocation (VH_BAND_RAY, VH_BAND_NORMAL_DDA, VH_BAND_RAY_DDA), packed many to an image.

Pose, voxel size, band and mode belong to the table, so an IMAGE is a group of pixels that share them; a pixel is a camera-space
vertex (x, y, z, w) and -- for the normal band -- a camera-space normal.  Images are 48x32 (six full launch tiles) or 33x17
(partial tiles on the right and at the bottom).  In the families a, b and c the pixels stand on every other column and row, so
that no pixel has a valid neighbour and the per-wave collapse of equal keys cannot hide one; family d fills whole images on purpose.

Two projections: ALL_PASS (reference semantics, a projection matrix whose first two rows are zero: every block projects to
pixel (0, 0), so the frustum test of VoxelUtils.cu:673 holds for every key and every key of a pixel is observable), and WIDE
(pinhole semantics, a focal length of 2 pixels: the test is live and drops the blocks behind the camera or far off axis).

Family a, EXACT: voxelSize = 2^-6, dyadic end points, poses that are signed axis permutations with a dyadic shift, direction
components 0 or +-2^j voxels: every fp32 operation of the set-up and of the walk is exact (the generator asserts it: the end
points come out as intended, and every crossing parameter tmax0 + i * tdelta, i <= 62, is an fp32 value), so band_ref.walk_exact
predicts the key sequence with no tolerance.  Two cases are marked `separated` instead: the walks of exactly 62 steps, whose
lengths (62 = 31 + 31 blocks) are no power of two.  Their crossings are not fp32 values, but no two of them are closer than
2^-8 in the segment's parameter and the last lies 2^-8 before the end, where 62 roundings move a crossing by less than 2^-17.
Family b, GENERAL: seeded random segments and hand-made special values, checked within band_ref.must_may.
Family c, DIVISION: VH_BAND_RAY vertices whose quotients sit next to a rounding tie of world2voxel at a block boundary.
Family d, WAVE: whole images whose lanes differ as much as lanes can."""
from fractions import Fraction

import numpy as np

import band_ref as R

F = np.float32
RAY, NORMAL_DDA, RAY_DDA = 0, 1, 2
ALL_PASS = dict(sem=0, proj=(0, 0, 0, 0, 0, 0, 0, 0, 1))
TABLE = dict(numBuckets=1 << 14, bucketSize=5, numVoxelBlocks=1 << 14)
VS6 = 2.0 ** -6
I4 = np.eye(4, dtype=np.float32)


def wide(W, H):
    return dict(sem=1, proj=(2, 0, W / 2, 0, 2, H / 2, 0, 0, 1))


class Image:
    """One table's frame: verts / normals [H, W, 4] float32 and what the table is set to.  pixels: {(x, y): tag}."""

    def __init__(self, name, W, H, mode, vs, band, T=I4, view=ALL_PASS, family="a"):
        self.name, self.W, self.H, self.mode, self.vs, self.band = name, W, H, mode, float(F(vs)), float(F(band))
        self.T = np.ascontiguousarray(np.asarray(T, F).reshape(4, 4))
        self.sem, self.proj = view["sem"], np.asarray(view["proj"], F)
        self.family = family
        self.verts = np.zeros((H, W, 4), F)
        self.normals = np.zeros((H, W, 4), F) if mode == NORMAL_DDA else None
        self.pixels = {}
        self._next = 0

    def put(self, x, y, v, n=None, tag=""):
        assert (x, y) not in self.pixels and 0 <= x < self.W and 0 <= y < self.H
        self.verts[y, x] = v
        if n is not None and self.normals is not None:
            self.normals[y, x, :3] = n[:3]
        self.pixels[(x, y)] = tag

    def add(self, v, n=None, tag=""):
        """The next free place on the grid of every other column and row."""
        per_row = (self.W + 1) // 2
        assert self._next < per_row * ((self.H + 1) // 2), f"image {self.name} is full"
        x, y = 2 * (self._next % per_row), 2 * (self._next // per_row)
        self._next += 1
        self.put(x, y, v, n, tag)
        return x, y

    def params(self, module):
        return module.default_params(voxelSize=self.vs, **TABLE)

    def vertex(self, xy):
        return self.verts[xy[1], xy[0]]

    def normal(self, xy):
        return self.normals[xy[1], xy[0]]

    def reference_ends(self, xy):
        """(A, B) fp32 of the pixel's segment; B is None for a surface-only pixel of the normal band."""
        if self.mode == NORMAL_DDA:
            g, a, b = R.ends_normal(self.vertex(xy), self.normal(xy), self.T, self.band)
            return (g, None) if a is None else (a, b)
        return R.ends_ray(self.vertex(xy), self.T, self.band)


def perm_pose(perm, signs, shift):
    """x_world[a] = signs[a] * x_cam[perm[a]] + shift[a]."""
    T = np.zeros((4, 4), F)
    for a in range(3):
        T[a, perm[a]] = signs[a]
        T[a, 3] = shift[a]
    T[3, 3] = 1
    return T


def _is_f32(q):
    return q == Fraction(float(F(float(q)))) and abs(q) < 2 ** 100


def assert_walk_is_fp32_exact(A, B, vs):
    """Every value the kernel's DDA forms for this segment is an fp32 value: boundary, tmax0, tdelta and tmax0 + i * tdelta."""
    vsq = Fraction(vs)
    for a in range(3):
        a0, b0 = Fraction(float(A[a])), Fraction(float(B[a]))
        d = b0 - a0
        assert _is_f32(d)
        if d == 0:
            continue
        c = R.block_of_exact(a0 / vsq)
        bound = (8 * (c + (1 if d > 0 else 0)) - Fraction(1, 2)) * vsq
        t0, td = (bound - a0) / d, 8 * vsq / abs(d)
        assert _is_f32(bound) and _is_f32(bound - a0) and _is_f32(td), (A, B)
        for i in range(R.MAX_STEPS + 2):
            assert _is_f32(t0 + i * td), (A, B, a, i)


# ---------------------------------------------------------------------------
# family a
# ---------------------------------------------------------------------------
def exact_segments():
    """[(tag, A, B, separated)] in VOXEL units (world = voxel * 2^-6); direction components 0 or +-2^j."""
    out = []
    corners = [(7.5, 7.5, 7.5), (-0.5, -0.5, -0.5), (-8.5, 7.5, -0.5)]
    for c in corners:                                                   # through a block corner: three-way tie
        for s in [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]:
            out.append(("corner", tuple(c[a] - 4 * s[a] for a in range(3)), tuple(c[a] + 4 * s[a] for a in range(3)), False))
    for c in corners[:2]:                                               # through a block edge: two-way tie, each pair of axes
        for free in range(3):
            for s1 in (1, -1):
                for s2 in (1, -1):
                    s = [s1, s2]
                    A, B = [0, 0, 0], [0, 0, 0]
                    for a in range(3):
                        if a == free:
                            A[a], B[a] = c[a] + 2.0, c[a] + 4.0                  # stays inside the block on the free axis
                        else:
                            sg = s.pop(0)
                            A[a], B[a] = c[a] - 4 * sg, c[a] + 4 * sg
                    out.append(("edge", tuple(A), tuple(B), False))
    for free in range(3):                                               # ALONG a block edge: two coordinates stay on a boundary
        for c in (7.5, -0.5, -8.5):
            A, B = [c, c, c], [c, c, c]
            A[free], B[free] = 1.5, 33.5
            out.append(("along-edge", tuple(A), tuple(B), False))
            out.append(("along-edge", tuple(B), tuple(A), False))
    for k in (7.5, -0.5, -8.5, 15.5):                                   # start exactly on 8k - 0.5, leaving both ways; inside a face
        for a in range(3):
            for sg in (1, -1):
                A, B = [2.0, 3.0, 4.0], [6.0, 3.0, 4.0]
                A[a], B[a] = k, k + 8 * sg
                out.append(("face-start", tuple(A), tuple(B), False))
            A, B = [1.0, 2.0, 3.0], [17.0, 10.0, 7.0]
            A[a], B[a] = k, k
            out.append(("in-face", tuple(A), tuple(B), False))
    for a in range(3):                                                  # axis-parallel, six directions, across 0
        for sg in (1, -1):
            A, B = [2.0, 3.0, 4.0], [2.0, 3.0, 4.0]
            A[a], B[a] = -14.0 * sg, 18.0 * sg
            out.append(("axis", tuple(A), tuple(B), False))
    for p in ((5.0, 5.0, 5.0), (-9.0, -8.0, -7.0), (-0.25, 7.25, -8.25)):   # zero length
        out.append(("zero", p, p, False))
    for lo in (-17.0, -16.5, -9.0, -8.5, -8.0, -7.5, -1.0, -0.5, -0.25, 0.0, 7.25, 7.5):    # both sides of 8k, k < 0: voxel2block's floor
        out.append(("floor", (lo, lo, lo), (lo + 2.0, lo + 2.0, lo + 2.0), False))
        out.append(("floor", (lo + 2.0, lo, lo + 2.0), (lo, lo + 2.0, lo), False))
    out.append(("cap", (1.0, 2.0, 3.0), (257.0, 258.0, 259.0), False))           # 96 crossings: stops at the cap, far from its end
    out.append(("cap", (1.0, 2.0, 3.0), (-255.0, 258.0, -253.0), False))
    out.append(("cap", (-0.5, -0.5, -0.5), (255.5, 255.5, 255.5), False))        # ... every one of them a three-way tie
    out.append(("cap-62", (2.0, 3.0, 4.0), (498.0, 3.0, 4.0), True))             # exactly 62 steps, one axis
    out.append(("cap-62", (2.0, 6.0, 3.0), (250.0, -242.0, 3.0), True))          # exactly 62 steps, 31 + 31
    out.append(("cap-63", (2.0, 3.0, 4.0), (506.0, 3.0, 4.0), True))             # one more: the cap cuts the last block off
    return out


def _exact_normal_image(name, W, H, T, segments, ws=(1.0,), spread=0):
    """Normal band of 8 voxels: g = (A + B) / 2, R n = (B - A) / 16; the vertex and the normal are the pose's pre-images.
    spread: segment i is moved by i * spread whole blocks along y, which keeps every tie and puts every pixel's blocks in a
    slab of its own -- the normal band's keys show only as the allocated SET, and there a block one pixel takes by a wrong
    order must not be a block another pixel takes rightly."""
    img = Image(name, W, H, NORMAL_DDA, VS6, 8 * VS6, T, ALL_PASS, "a")
    Rm, t = img.T[:3, :3].astype(np.float64), img.T[:3, 3].astype(np.float64)
    img.exact = {}
    for i, (tag, A, B, separated) in enumerate(segments):
        w = ws[i % len(ws)]
        off = np.array((0.0, 8.0 * spread * i, 0.0))
        A, B = (np.array(A) + off) * VS6, (np.array(B) + off) * VS6
        g, rn = (A + B) / 2, (B - A) / (2 * img.band)
        v = Rm.T @ (g - t * w)
        n = Rm.T @ rn
        if tag == "zero":
            n = np.array([2.0 ** -100, 0, 0])                            # a normal, but band * n vanishes beside g
        if v[2] == 0:
            continue                                                     # (z = 0 is "no measurement"; asserted below that few go)
        xy = img.add((v[0], v[1], v[2], w), n, tag)
        a, b = img.reference_ends(xy)
        assert all(float(a[k]) == A[k] and float(b[k]) == B[k] for k in range(3)), (name, tag, A, B, a, b)
        if not separated:
            assert_walk_is_fp32_exact(a, b, VS6)
        img.exact[xy] = separated
    assert len(img.pixels) >= len(segments) - 4
    return img


def _exact_ray_image(name, W, H, T, band_vox):
    """Ray DDA: the segment is the vertex scaled to depths z - b (or z) and z + b; x, y in {0, +-2^j} voxels and z chosen so
    that both scale factors and every product are exact."""
    img = Image(name, W, H, RAY_DDA, VS6, band_vox * VS6, T, ALL_PASS, "a")
    img.exact = {}
    b = band_vox
    for z, tag in ((2 * b, "z-b>0"), (b, "z-b=0"), (b / 2, "z-b<0"), (4 * b, "z-b>0")):
        for x in (0.0, 4.0, -16.0, 64.0, -128.0):
            for y in (0.0, -8.0, 32.0):
                for w in (1.0,) if (x, y) != (4.0, -8.0) else (1.0, 0.0, 2.0):
                    xy = img.add((x * VS6, y * VS6, z * VS6, w), None, tag + f" w={w:g}")
                    a, e = img.reference_ends(xy)
                    assert_walk_is_fp32_exact(a, e, VS6)
                    img.exact[xy] = False
    return img


def family_a():
    segs = exact_segments()
    shift = (3 * 8 * VS6, -5 * VS6, 0.5 * VS6)                           # dyadic: a block edge, voxels, half a voxel
    P = perm_pose((2, 0, 1), (1, -1, -1), shift)
    P2 = perm_pose((1, 2, 0), (-1, 1, -1), (-2.0, 0.25, 1.0))
    return [_exact_normal_image("a-normal-identity", 48, 32, I4, segs),
            _exact_normal_image("a-normal-permuted-w", 33, 17, P, segs[::2][:150], ws=(1.0, 0.0, 2.0)),
            _exact_normal_image("a-normal-permuted2-spread", 48, 32, P2, segs, ws=(1.0, 2.0), spread=80),
            _exact_ray_image("a-ray-identity", 33, 17, I4, 16),
            _exact_ray_image("a-ray-permuted", 48, 32, P, 8)]


# ---------------------------------------------------------------------------
# family b
# ---------------------------------------------------------------------------
def random_rigid(rng, reach):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, rng.uniform(-reach, reach, 3)
    return T.astype(F)


SEED_B, GROUPS_B = 20261, ((NORMAL_DDA, 48, 32), (RAY_DDA, 33, 17), (NORMAL_DDA, 33, 17), (RAY_DDA, 48, 32))


def family_b():
    rng = np.random.default_rng(SEED_B)
    out = []
    for gi, (mode, W, H) in enumerate(GROUPS_B):
        vs = float(np.exp(rng.uniform(np.log(0.005), np.log(0.05))))
        band = float(rng.uniform(1, 40)) * vs
        img = Image(f"b-random-{gi}", W, H, mode, vs, band, random_rigid(rng, 3.0), wide(W, H), "b")
        for _ in range(((W + 1) // 2) * ((H + 1) // 2)):
            z = float(rng.uniform(0.3, 4.0))
            v = (float(rng.uniform(-1.2, 1.2)) * z, float(rng.uniform(-1.2, 1.2)) * z, z, 1.0)
            n = rng.normal(size=3)
            img.add(v, n / np.linalg.norm(n) * rng.uniform(0.05, 1.0))
        out.append(img)
    # special values: the identity pose, so that a component of the vertex or of the normal IS the world component
    vs, band = 0.02, 0.1
    img = Image("b-special-normal", 33, 17, NORMAL_DDA, vs, band, I4, ALL_PASS, "b")
    nan = float("nan")
    for v, n, tag in [((0.3, 0.0, 1.2, 1), (0.6, 2.0 ** -140, 0.8), "dir.y denormal"),
                      ((0.0, 0.3, 1.2, 1), (2.0 ** -146, -0.6, 0.8), "dir.x denormal, smallest"),
                      ((0.3, 1.2, 0.0 + 2.0 ** -140, 1), (0.6, 0.8, 2.0 ** -135), "z and dir.z denormal"),
                      ((0.3, 0.0, 1.2, 1), (0.6, 2.0 ** -117, 0.8), "dir.y = 2^-120: tdelta overflows"),
                      ((0.0, 0.0, 1.2, 1), (2.0 ** -117, -2.0 ** -117, 1.0), "two such components"),
                      ((0.3, 0.1, 1.2, 1), (0.6, -0.0, 0.8), "-0.0"),
                      ((0.3, 0.1, 1.2, 1), (-0.0, -0.0, -1.0), "-0.0 twice"),
                      ((0.3, 0.1, 1.2, 1), (-0.0, -0.0, -0.0), "all -0.0: no normal"),
                      ((0.3, 0.1, 1.2, 1), (nan, 0.6, 0.8), "NaN x"), ((0.3, 0.1, 1.2, 1), (0.6, nan, 0.8), "NaN y"),
                      ((0.3, 0.1, 1.2, 1), (0.6, 0.8, nan), "NaN z"), ((0.3, 0.1, 1.2, 1), (nan, nan, nan), "NaN all"),
                      ((0.3, 0.1, 1.2, 1), (0.0, 0.0, 0.0), "zero normal"),
                      ((-0.7, 0.4, 2.2, 1), (1.0, 2.0, 2.0), "length 3"), ((-0.7, 0.4, 2.2, 1), (-2.0, 1.0, -2.0), "length 3"),
                      ((0.5, -0.2, 2.0 ** -130, 1), (0.0, 0.6, 0.8), "z denormal"),
                      ((0.5, -0.2, -1.1, 1), (0.6, 0.0, 0.8), "z negative"), ((-0.01, 0.01, -0.01, 1), (0.3, 0.3, -0.9), "z negative")]:
        img.add(v, n, tag)
    out.append(img)
    img = Image("b-special-ray", 33, 17, RAY_DDA, vs, band, I4, ALL_PASS, "b")
    for v, tag in [((2.0 ** -128, -2.0 ** -129, 2.0 ** -127, 1), "z denormal"), ((0.4, -0.3, -1.1, 1), "z negative"),
                   ((0.4, -0.3, -0.05, 1), "z negative, -b < z"), ((-0.0, 0.0, 0.7, 1), "-0.0"), ((2.0 ** -140, 0.2, 0.7, 1), "x denormal"),
                   ((2.0 ** -120, 2.0 ** -120, 0.7, 1), "dir = 2^-120 twice"), ((0.3, 0.2, 0.1, 1), "z = b"),
                   ((0.3, 0.2, float(np.nextafter(F(0.1), F(1))), 1), "z just above b")]:
        img.add(v, None, tag)
    out.append(img)
    return out


# ---------------------------------------------------------------------------
# family c
# ---------------------------------------------------------------------------
DIVISORS = (0.02, 0.005, 0.01, 1.0 / 3.0, float.fromhex("0x1.fffffep-6"), 2.0 ** -6)
LO_D, HI_D, LO_N, HI_N = F(2.0 ** -40), F(2.0 ** 40), F(2.0 ** -50), F(2.0 ** 50)


def in_range(x, lo, hi):
    a = abs(F(x))
    return bool(a >= lo and a <= hi)


def division_paths(img, xy):
    """{'scale': set of 'fast' / 'plain', 'vs': ...}: which form of each division the samples of this pixel take, from the range
    gates alone (2^-40 <= |divisor| <= 2^40 and 2^-50 <= |numerator| <= 2^50 take the hoisted reciprocal, all else the plain
    division; one sample per pixel -- no band -- always divides plainly)."""
    x, y, z, w = [F(c) for c in img.vertex(xy)]
    half = R.ray_half(img.vs, img.band)
    step = F(F(4) * F(img.vs))
    paths = {"scale": set(), "vs": set()}
    if half == 0:
        return paths
    with np.errstate(all="ignore"):
        for k in range(2 * half + 1):
            if k == half:
                p = R.mat4_f32(img.T, x, y, z, w)
            else:
                s = F(z + F(F(F(k) - F(half)) * step))
                if not s > 0:
                    continue
                paths["scale"].add("fast" if in_range(z, LO_D, HI_D) and in_range(s, LO_N, HI_N) else "plain")
                sc = F(s / z)
                p = R.mat4_f32(img.T, F(x * sc), F(y * sc), s, w)
            for c in p:
                paths["vs"].add("fast" if in_range(img.vs, LO_D, HI_D) and in_range(c, LO_N, HI_N) else "plain")
    return paths


def _block1(q):
    with np.errstate(all="ignore"):
        return R.voxel2block1(R.f2i_rz(F(F(q) + np.copysign(F(0.5), F(q)))))


def _block1_vec(q):
    """_block1 for an array of quotients of ordinary size."""
    v = np.trunc((q + np.copysign(F(0.5), q)).astype(F)).astype(np.int64)
    return np.floor_divide(v, 8)


def ulp_sensitive(q):
    """The block of quotient q differs from that of nextafter(q, +inf) or nextafter(q, -inf)."""
    q = F(q)
    return _block1(q) != _block1(np.nextafter(q, F(np.inf))) or _block1(q) != _block1(np.nextafter(q, F(-np.inf)))


def _tie(rng, reach_vox):
    """m + 0.5 with m = 7 (mod 8): the voxel coordinate at which world2voxel's rounding changes the block."""
    j = int(rng.integers(-reach_vox // 8, reach_vox // 8))
    return 8 * j - 1 + 0.5


def find_numerator(vs, tie, through=None):
    """An fp32 x whose quotient (x * scale) / vs, correctly rounded at each step, is ulp_sensitive -- next to the tie -- and,
    where `through` = (scale, scale one ulp down, one ulp up) is given, changes its block when the scale moves by an ulp."""
    vs = F(vs)
    scale = F(1) if through is None else through[0]
    with np.errstate(all="ignore"):
        x = F(F(F(tie) * vs) / scale)
        lo = x
        for _ in range(24):
            lo = np.nextafter(lo, F(-np.inf))
        cand = lo
        for _ in range(49):
            q = F(F(cand * scale) / vs)
            if abs(float(q) - tie) < 1.0 and ulp_sensitive(q):
                if through is None:
                    return float(cand)
                if any(_block1(F(F(cand * sc) / vs)) != _block1(q) for sc in through[1:]):
                    return float(cand)
            cand = np.nextafter(cand, F(np.inf))
    return None


SEED_C = 9071


def family_c():
    rng = np.random.default_rng(SEED_C)
    out = []
    for di, vs in enumerate(DIVISORS):
        vs = float(F(vs))
        clamp = di == 2                  # one image with half = 31, the clamp's value: vh_set_alloc_band refuses what the clamp would cut
        band = 4 * vs * 30.5 if clamp else 4 * vs * 2
        img = Image(f"c-div-{di}", 48, 32, RAY, vs, band, I4, ALL_PASS, "c")
        half = R.ray_half(vs, band)
        assert half == (31 if clamp else 2)
        img.kind, img.sensitive_sample = {}, {}
        n_direct = n_scaled = 0
        while n_direct < 36:                                             # the surface sample carries the vertex bit for bit: three free coordinates
            v = [find_numerator(vs, _tie(rng, 1600)) for _ in range(3)]
            if None in v or v[2] == 0:
                continue
            xy = img.add((v[0], v[1], v[2], 1.0), None, "direct")
            img.kind[xy] = "direct"
            n_direct += 1
        step = F(F(4) * F(vs))
        while n_scaled < (12 if clamp else 40):                          # s / z, then / voxelSize: sample k != half
            k = int(rng.integers(0, 2 * half + 1))
            if k == half:
                continue
            off = F(F(F(k) - F(half)) * step)
            zmag = float(np.exp(rng.uniform(np.log(0.05), np.log(50.0))))
            tz = round(zmag / vs / 8) * 8 - 0.5                          # the sample's own depth s next to a tie as well
            z = None
            z0 = F(F(F(tz) * F(vs)) - off)
            for d in range(-6, 7):
                zc = z0
                for _ in range(abs(d)):
                    zc = np.nextafter(zc, F(np.inf) if d > 0 else F(-np.inf))
                s = F(zc + off)
                if s > 0 and zc > 0 and ulp_sensitive(F(s / F(vs))):
                    z, sz = zc, s
                    break
            if z is None:
                continue
            sc = F(sz / z)
            through = (sc, np.nextafter(sc, F(0)), np.nextafter(sc, F(np.inf)))
            x, y = find_numerator(vs, _tie(rng, 1600), through), find_numerator(vs, _tie(rng, 1600), through)
            if x is None or y is None:
                continue
            xy = img.add((x, y, float(z), 1.0), None, f"scaled k={k}")
            img.kind[xy], img.sensitive_sample[xy] = "scaled", k
            n_scaled += 1
        out.append(img)
    out += _gate_images()
    return out


def _gate_images():
    """Operands on both sides of every range gate of the hoisted divisions."""
    up, dn = (lambda v: float(np.nextafter(F(v), F(np.inf)))), (lambda v: float(np.nextafter(F(v), F(0))))
    out = []
    img = Image("c-gate-z-g", 33, 17, RAY, 0.02, 0.16, I4, ALL_PASS, "c")
    for z in (2.0 ** 40, up(2.0 ** 40), 2.0 ** -40, dn(2.0 ** -40), 2.0 ** 39, 2.0 ** -39):              # |z|, the divisor of s / z
        img.add((1.5 if z > 1 else z * 3, -0.25 if z > 1 else -z, z, 1.0), None, f"z={z.hex()}")
    for g in (2.0 ** 50, up(2.0 ** 50), 2.0 ** -50, dn(2.0 ** -50), -2.0 ** 50, -up(2.0 ** 50), -dn(2.0 ** -50), 0.0):   # |g|, numerator of / vs
        img.add((g, -g, 1.0, 1.0), None, f"g={g.hex()}")
    out.append(img)
    for name, vs in (("lo-in", 2.0 ** -40), ("lo-out", dn(2.0 ** -40)), ("hi-in", 2.0 ** 40), ("hi-out", up(2.0 ** 40))):   # voxelSize
        img = Image(f"c-gate-vs-{name}", 33, 17, RAY, vs, 8 * vs, I4, ALL_PASS, "c")
        for m in (3.0, 7.4, 7.5, 100.0, -8.5, -8.4):
            img.add((m * vs, -m * vs, 20.0 * vs, 1.0), None, f"{m} voxels")
        out.append(img)
    # |s| below 2^-50 by cancellation: vs = 2^-32, step = 2^-30, z just above a multiple of the step
    vs = 2.0 ** -32
    img = Image("c-gate-s-lo", 33, 17, RAY, vs, 8 * vs, I4, ALL_PASS, "c")
    for z in (2.0 ** -30 * (1 + 2.0 ** -23), 2.0 ** -29 * (1 + 2.0 ** -23), 2.0 ** -30 * 1.5):
        img.add((z, -z / 2, z, 1.0), None, f"z={z.hex()}")
    out.append(img)
    # |s| above 2^50: vs = 2^46, step = 2^48, half = 8
    vs = 2.0 ** 46
    img = Image("c-gate-s-hi", 33, 17, RAY, vs, 2.0 ** 51, I4, ALL_PASS, "c")
    for z in (2.0 ** 30, 2.0 ** 40, 2.0 ** 47):
        img.add((z / 4, -z / 8, z, 1.0), None, f"z={z.hex()}")
    out.append(img)
    for g in out:
        g.kind, g.sensitive_sample = {xy: "gate" for xy in g.pixels}, {}
    return out


def sensor_image():
    """The sensor path cannot reach the vertices of family c: a vertex there is (K_inv (px, py, 1)) * (depth / 5000) with a
    16-bit depth.  What it can reach is searched instead: for pixels of a 48x32 image, the depth whose vertex has the most
    coordinates with an ulp-sensitive quotient.  Returns (depth uint16 [H, W], K_inv float32 [9], {(x, y): sensitive coordinates})."""
    W, H, vs = 48, 32, F(0.02)
    kinv = np.array([1 / 40.0, 0, -24 / 40.0, 0, 1 / 40.0, -16 / 40.0, 0, 0, 1], F)
    depth = np.zeros((H, W), np.uint16)
    d = (np.arange(1, 65536).astype(F) / F(5000.0)).astype(F)
    found = {}
    for py in range(0, H, 4):
        for px in range(0, W, 2):
            fx, fy = F(px), F(py)
            row = [F(F(F(kinv[3 * r] * fx) + F(kinv[3 * r + 1] * fy)) + F(kinv[3 * r + 2] * F(1))) for r in range(3)]
            hits = np.zeros(len(d), np.int32)
            for r in range(3):
                q = ((row[r] * d).astype(F) / vs).astype(F)
                b = _block1_vec(q)
                hits += (b != _block1_vec(np.nextafter(q, F(np.inf)))) | (b != _block1_vec(np.nextafter(q, F(-np.inf))))
            best = int(np.argmax(hits))
            if hits[best] > 0:
                depth[py, px] = best + 1
                found[(px, py)] = int(hits[best])
    return depth, kinv, found


# ---------------------------------------------------------------------------
# family d
# ---------------------------------------------------------------------------
def _fill_surface_only(img, skip=()):
    """Every pixel valid, none with a normal (normal band) / all with a short walk on the axis (ray DDA)."""
    for y in range(img.H):
        for x in range(img.W):
            if (x, y) in skip:
                continue
            if img.mode == NORMAL_DDA:
                img.put(x, y, ((x % 7) * 3 * VS6, (y % 5) * 3 * VS6, 40 * VS6, 1.0), (0, 0, 0), "idle")
            else:
                img.put(x, y, (0.0, 0.0, (40 + (x + 3 * y) % 9) * VS6, 1.0), None, "short")


def family_d():
    out = []
    spots = {"wave0": (5, 1), "wave1": (9, 6), "wave2": (0, 9), "wave3": (15, 14), "partial": (32, 16)}
    for name, xy in spots.items():                                       # one 62-step walker among idle lanes
        img = Image(f"d-long-normal-{name}", 33, 17, NORMAL_DDA, VS6, 8 * VS6, I4, ALL_PASS, "d")
        _fill_surface_only(img, {xy})
        A, B = np.array((1.0, 2.0, 3.0)) * VS6, np.array((257.0, 258.0, 259.0)) * VS6          # 96 crossings: capped at 62
        img.put(*xy, tuple((A + B) / 2) + (1.0,), (B - A) / (2 * img.band), "long")
        assert_walk_is_fp32_exact(*img.reference_ends(xy), VS6)
        out.append(img)
        img = Image(f"d-long-ray-{name}", 33, 17, RAY_DDA, VS6, 8 * VS6, I4, ALL_PASS, "d")
        _fill_surface_only(img, {xy})
        img.put(*xy, (512 * VS6, -256 * VS6, 16 * VS6, 1.0), None, "long")    # depths 8 .. 24 voxels: scaled by 0.5 and 1.5, 64 + 32 + 2 blocks
        assert_walk_is_fp32_exact(*img.reference_ends(xy), VS6)
        out.append(img)
    # 256 lanes of one tile, walks of 0 .. 62 steps in scrambled order (axis-parallel, from a block the row shares; one axis, so
    # nothing is ordered, and the last crossing lies 4.5 / (8 n) >= 2^-7 before the segment's end: predicted exactly all the same)
    rng = np.random.default_rng(77)
    lengths = rng.permutation(256) % 63
    img = Image("d-lengths", 48, 32, NORMAL_DDA, VS6, 8 * VS6, I4, ALL_PASS, "d")
    for t in range(256):
        x, y, n = 16 + (t & 15), 16 + (t >> 4), int(lengths[t])
        axis = (t >> 4) % 3
        A = np.array((4.0, 3.0 + 8 * ((t >> 4) % 2), 5.0))
        B = A.copy()
        B[axis] += 8.0 * n * (1 if (t >> 5) % 2 else -1)
        n_cam = (B - A) * VS6 / (2 * img.band) if n else np.array((0.0, 0.0, 0.0))
        img.put(x, y, tuple((A + B) / 2 * VS6) + (1.0,), n_cam, f"len {n}")
    out.append(img)
    out.append(_dedup_image("d-dedup", 48, 32, [(3, 1), (14, 3), (15, 7), (20, 15), (30, 30)]))
    out.append(_dedup_image("d-dedup-partial", 33, 17, [(3, 3), (15, 15), (31, 15), (20, 7)]))
    # the same, confined to the last column and the last row of the 33x17 image
    for src in (out[-3], out[-1]):
        img = Image(src.name + "-rim", 33, 17, src.mode, src.vs, src.band, src.T, ALL_PASS, "d")
        rim = [(32, y) for y in range(17)] + [(x, 16) for x in range(32)]
        donors = sorted(src.pixels, key=lambda p: (p[1], p[0]))
        donors = [p for p in donors if src.pixels[p] != "fill"][:len(rim)]
        for xy, p in zip(rim, donors):
            img.put(*xy, src.vertex(p).copy(), src.normal(p).copy(), src.pixels[p])
        out.append(img)
    return out


def _dedup_image(name, W, H, spots):
    """Pairs of adjacent pixels with bit-identical vertices and normals (walking along +x); their right and lower neighbours
    start in the same block -- equal keys at sample 0 -- and walk elsewhere, so at every later sample the pair's second pixel
    equals its LEFT neighbour and differs from the one ABOVE / the pixel below equals nobody."""
    img = Image(name, W, H, NORMAL_DDA, VS6, 8 * VS6, I4, ALL_PASS, "d")

    def pix(A, B):
        A, B = np.array(A), np.array(B)
        return tuple((A + B) / 2 * VS6) + (1.0,), (B - A) * VS6 / (2 * img.band)
    for i, (x, y) in enumerate(spots):
        base = np.array((4.0 + 64 * i, 3.0, 5.0))
        twin = pix(base, base + (40, 0, 0))
        right = pix(base, base + (0, 40, 0))
        lower = pix(base, base + (0, 0, 40))
        lower2 = pix(base, base + (-40, 0, 0))
        for p, (v, n), tag in (((x, y), twin, "twin"), ((x + 1, y), twin, "twin"), ((x + 2, y), right, "right"),
                               ((x, y + 1), lower, "lower"), ((x + 1, y + 1), lower2, "lower"), ((x + 2, y + 1), twin, "twin-diag")):
            if p[0] < W and p[1] < H and p not in img.pixels:
                img.put(*p, v, n, tag)
    return img


_cache = {}


def images(family):
    if family not in _cache:
        _cache[family] = {"a": family_a, "b": family_b, "c": family_c, "d": family_d}[family]()
    return _cache[family]


def all_images():
    return [i for f in "abcd" for i in images(f)]
