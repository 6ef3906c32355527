"""Crafted inputs for the block silhouettes (vh_render_blocks): key sets, image sizes, intrinsics, poses and depth ranges chosen
so that every path of csrc/vh_blocks.hip is reached, each with the conditions that prove it is.

A silhouette depends on which blocks are allocated and on nothing they hold, so a case is a set of keys with zeroed voxels.  The
conditions are functions of the rule's per-block masks (tests/blocks_ref.py) or, for the near-plane cubes, of the corners'
camera depths; tests/test_blocks_ref_cpu.py asserts them on the rule alone, tests/test_gpu_blocks_crafted.py renders the cases.

What reaches what (kernel constants: a workgroup = a 16x16 region of four 8x8 wave tiles, 256 records staged per round, 1024
boxes filtered per chunk):
  shape_WxH     partial regions and tiles in x and in y, images smaller than a tile; a ring of blocks leaves the centre empty and
                reaches the last column and row, under the identity attitude and rolled by 90 degrees
  rounds_N      N = 256, 257, 512, 513 blocks one behind the other in ONE region, every one kept by some pixel: exactly N boxes
                are listed (the list holds at least the kept blocks and at most the allocated ones): 1, 2, 2 and 3 staging rounds
  rounds_beside the 513 in one region of a 48x32 image whose other five regions keep nothing
  chunks_N      N = 1024, 1025, 2049 blocks, every one kept: 1, 2 and 3 chunks.  View 0 sees the wall head-on and every block is
                the ONLY block of some pixel, so whichever records land in a late chunk decide pixels of their own; view 1 looks
                along the wall, where a region keeps more than 256 blocks of one chunk
  calls         one context, four calls: 2049 blocks, fewer than 10, none, 2049 again (the two counter words in turn)
  geometry      negative keys, voxel sizes 0.005 and 1, fx != fy, a principal point outside the image, t_min = 0, a cube cut by
                t_max and cubes beyond it, a cube smaller than a pixel between and on pixel centres, cubes that straddle the near
                plane with 1, 3, 4 and 7 corners beyond it (a screen box culls per 8x8 tile, so the 1- and 4-corner cases put those
                corners in one tile and the cut in the next), the camera inside a cube, attitudes that are exact multiples of 90 degrees
  far_2^k       the same small scene and camera at key offsets 2^10, 2^15, 2^18, 2^20"""
import numpy as np

import blocks_ref as br
import mesh_models as mm

F = np.float32
VS = 0.02
S = 8 * VS                        # a block's side in metres at the default voxel size


# ---- poses (camera -> world, row-major 4x4; the camera looks along its +z) --------------------------------------------
def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


ROLL90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
YAW90 = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])             # looks along +x
YAW180 = np.diag([-1.0, 1, -1])
YAW270 = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])            # looks along -x
PITCH90 = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])           # looks along -y
PITCH270 = np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]])          # looks along +y
ROLL180 = np.diag([-1.0, -1, 1])


def pose_of(R, eye):
    p = np.eye(4)
    p[:3, :3], p[:3, 3] = R, eye
    return p.astype(F)


def looking_along(n):
    """A rotation whose optical axis is n."""
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    x = np.cross([0.0, 1.0, 0.0], n) if abs(n[1]) < 0.9 else np.cross(n, [1.0, 0.0, 0.0])
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(n, x), n], 1)


class View:
    """One call: a pose, a depth range, and what the rule's answer must show (see check())."""

    def __init__(self, pose, t_min=0.1, t_max=5.0, **conditions):
        self.pose, self.t_min, self.t_max, self.conditions = np.asarray(pose, F).reshape(4, 4), float(t_min), float(t_max), conditions


class Case:
    def __init__(self, name, keys, size, intrinsics, views, voxel_size=VS, buckets=4093, bucket_size=8):
        self.name = name
        self.keys = np.asarray(keys, np.int64).reshape(-1, 3)
        assert len(set(map(tuple, self.keys.tolist()))) == len(self.keys)
        self.W, self.H = size
        self.fx, self.fy, self.cx, self.cy = (float(F(v)) for v in intrinsics)
        self.views, self.voxel_size = views, voxel_size
        self.table = dict(numBuckets=buckets, bucketSize=bucket_size, numVoxelBlocks=len(self.keys) + 8, voxelSize=voxel_size)
        self._expected = {}

    def model(self):
        return {tuple(int(c) for c in k): (np.zeros(512, F), np.zeros(512, F)) for k in self.keys}

    def expected(self, i):
        """(front, back, kept) of view i by the rule, computed once."""
        if i not in self._expected:
            v = self.views[i]
            self._expected[i] = br.render(self.keys, self.voxel_size, self.W, self.H, self.fx, self.fy, self.cx, self.cy, v.pose,
                                          v.t_min, v.t_max)
        return self._expected[i]


def corners_beyond(case, view):
    """How many of the (single) cube's corners lie beyond the plane z = 0.999 t_min of the view, and the smallest distance of a
    corner from that plane (float64)."""
    lo, hi = br.cubes(case.keys[:1], case.voxel_size)
    c = np.array([[(hi if (i >> a) & 1 else lo)[0, a] for a in range(3)] for i in range(8)], np.float64)
    p = view.pose.astype(np.float64)
    z = (c - p[:3, 3]) @ p[:3, 2]
    zn = 0.999 * view.t_min
    return int((z >= zn).sum()), float(np.abs(z - zn).min())


def check(case, i, front, back, kept):
    """Asserts the conditions of view i on an answer of the rule; returns the measured facts."""
    v = case.views[i]
    c = v.conditions
    n_kept = br.kept_blocks(kept)
    regions = br.region_counts(kept)
    facts = dict(blocks=len(case.keys), kept=n_kept, regions=regions, nonzero=int((back > 0).sum()), pixels=back.size)
    assert ((front == 0) == (back == 0)).all() or v.t_min == 0
    assert np.array_equal(back > 0, kept.any(0)) or v.t_min == 0
    if "kept" in c:
        assert n_kept == c["kept"], (case.name, i, n_kept)
    if "kept_below" in c:
        assert 1 <= n_kept < c["kept_below"], (case.name, i, n_kept)
    if "regions" in c:                                   # {(ry, rx): blocks kept}: every other region keeps none
        want = np.zeros_like(regions)
        for at, n in c["regions"].items():
            want[at] = n
        assert np.array_equal(regions, want), (case.name, i, regions)
    if "region_above" in c:
        assert regions.max() > c["region_above"], (case.name, i, regions.max())
    if c.get("alone"):
        assert br.alone_somewhere(kept).all(), (case.name, i, int((~br.alone_somewhere(kept)).sum()))
    if c.get("edges"):                                   # the last column and the last row hold a pixel, some pixel is empty
        assert (back[:, -1] > 0).any() and (back[-1, :] > 0).any() and (back == 0).any(), (case.name, i)
    if c.get("partial"):
        assert (back > 0).any() and (back == 0).any(), (case.name, i)
    if c.get("full"):
        assert (back > 0).all(), (case.name, i)
    if c.get("empty"):
        assert n_kept == 0 and not front.any() and not back.any(), (case.name, i)
    if c.get("cut"):                                     # a cube cut by t_max, and cubes wholly beyond it
        assert (back.view(np.uint32) == F(v.t_max).view(np.uint32)).any() and n_kept < len(case.keys), (case.name, i)
        facts["at_t_max"] = int((back.view(np.uint32) == F(v.t_max).view(np.uint32)).sum())
    if c.get("clipped"):                                 # a front face nearer than t_min: front == t_min bit for bit
        assert (front.view(np.uint32) == F(v.t_min).view(np.uint32)).any(), (case.name, i)
    if "corners" in c:
        n, margin = corners_beyond(case, v)
        assert n == c["corners"] and margin > 1e-3, (case.name, i, n, margin)
        facts["corners"] = n
    return facts


# ---- (a) image shapes -------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (8, 8), (15, 17), (16, 16), (17, 16), (33, 9), (100, 75), (161, 121), (257, 3)]


def ring_keys():
    """A frame of 12 x 12 blocks without its middle 4 x 4, odd columns one block deeper (a transposed image differs)."""
    return [(x, y, 8 + (x & 1)) for y in range(-6, 6) for x in range(-6, 6) if not (-2 <= x <= 1 and -2 <= y <= 1)]


def shape_case(W, H):
    """The image spans tangents of about -0.5 .. 0.5 in each direction that has more than one pixel; the ring spans 0.25 .. 0.75."""
    eye = (0.01, -0.02, 0.03)
    if (W, H) == (1, 1):                                 # one pixel cannot be both: two views whose pixel is hit, one empty
        yaw = rot_y(np.arctan(0.5))
        views = [View(pose_of(yaw, eye), full=True), View(pose_of(yaw @ ROLL90, eye), full=True), View(pose_of(np.eye(3), eye), empty=True)]
        return Case("shape_1x1", ring_keys(), (1, 1), (1.0, 1.0, 0.0, 0.0), views)
    fx, cx = (W - 1, (W - 1) / 2 + 0.125) if W > 1 else (1.0, 0.0)
    fy, cy = (H - 1, (H - 1) / 2 - 0.25) if H > 1 else (1.0, 0.0)
    views = [View(pose_of(np.eye(3), eye), edges=True), View(pose_of(ROLL90, eye), edges=True)]
    return Case(f"shape_{W}x{H}", ring_keys(), (W, H), (fx, fy, cx, cy), views)


# ---- (b) staging rounds -----------------------------------------------------------------------------------------------
ROUNDS = (256, 257, 512, 513)


def bundle_keys(n):
    """2 x 2 columns of blocks along +z around the z axis, n blocks in all (an odd one extends the column x = y = -1)."""
    keys = [(x, y, z) for z in range(n // 4) for y in (-1, 0) for x in (-1, 0)]
    return keys + [(-1, -1, n // 4)] * (n % 4)


def rounds_case(n):
    """One 16x16 image; every ray stays inside its quadrant's column down to the last block (tangents below 0.004, 21.7 m)."""
    view = View(pose_of(np.eye(3), (0.0, 0.0, -1.0)), 0.1, 40.0, kept=n, regions={(0, 0): n})
    return Case(f"rounds_{n}", bundle_keys(n), (16, 16), (2000.0, 2000.0, 7.3, 7.6), [view])


def rounds_beside_case():
    """The 513 from 10 m in a 48x32 image: about 5 x 5 pixels inside region (1, 1), the other regions keep nothing."""
    view = View(pose_of(np.eye(3), (0.0, 0.0, -10.0)), 0.1, 40.0, kept=513, regions={(1, 1): 513})
    return Case("rounds_beside", bundle_keys(513), (48, 32), (150.0, 150.0, 23.4, 23.6), [view])


# ---- (c) chunks, (d) successive calls ---------------------------------------------------------------------------------
CHUNKS = {1024: (32, 32, 0), 1025: (32, 32, 1), 2049: (64, 32, 1)}
CHUNK_SIZES = {1024: (72, 64), 1025: (72, 64), 2049: (128, 64)}
CHUNK_F = 237.5                  # a block is 1.9 pixels wide from 20 m


def wall_keys(n):
    nx, ny, extra = CHUNKS[n]
    keys = [(x - nx // 2, y - ny // 2, 0) for y in range(ny) for x in range(nx)]
    return keys + [(nx // 2, 0, 0)] * extra


def chunk_views(n):
    nx = CHUNKS[n][0]
    head_on = View(pose_of(np.eye(3), (0.5 * S, 0.0, -20.0)), 0.1, 30.0, kept=n, alone=True)
    along = View(pose_of(YAW90, (-nx // 2 * S - 10.0, 0.05, 0.5 * S)), 0.1, 30.0, region_above=256 if n > 2048 else 128)
    return head_on, along


def chunks_case(n):
    W, H = CHUNK_SIZES[n]
    return Case(f"chunks_{n}", wall_keys(n), (W, H), (CHUNK_F, CHUNK_F, (W - 1) / 2 + 0.2, (H - 1) / 2 - 0.3), list(chunk_views(n)))


def calls_case():
    W, H = CHUNK_SIZES[2049]
    head_on = chunk_views(2049)[0]
    close = View(pose_of(np.eye(3), (0.5 * S + 0.03, 0.02, -0.3)), 0.1, 30.0, kept_below=10)
    away = View(pose_of(YAW180, (0.5 * S, 0.0, -20.0)), 0.1, 30.0, empty=True)
    views = [head_on, close, away, View(head_on.pose, 0.1, 30.0, kept=2049)]
    return Case("calls", wall_keys(2049), (W, H), (CHUNK_F, CHUNK_F, (W - 1) / 2 + 0.2, (H - 1) / 2 - 0.3), views)


# ---- (e) geometry -----------------------------------------------------------------------------------------------------
SMALL = (40, 30)
PLAIN = (45.0, 45.0, 19.3, 14.6)
ASKEW = rot_y(-0.35) @ rot_x(0.2)
TILT = rot_y(0.5) @ rot_x(-0.4)


def geometry_cases():
    out = []
    cluster = mm.cube_keys(-2, 1)                                                             # keys -2 .. 0: across the origin
    out.append(Case("negative_keys", cluster, SMALL, PLAIN, [View(pose_of(ASKEW, (0.5, -0.3, -1.2)), partial=True)]))
    out.append(Case("voxel_size_0.005", mm.cube_keys(-1, 2), SMALL, PLAIN,
                    [View(pose_of(ASKEW, (0.125, -0.075, -0.3)), 0.02, 2.0, partial=True)], voxel_size=0.005))
    out.append(Case("voxel_size_1", mm.cube_keys(-1, 2), SMALL, PLAIN,
                    [View(pose_of(ASKEW, (25.0, -15.0, -60.0)), 1.0, 200.0, partial=True)], voxel_size=1.0))
    out.append(Case("fx_ne_fy", cluster, SMALL, (60.0, 35.0, 19.3, 14.6), [View(pose_of(ASKEW, (0.5, -0.3, -1.2)), partial=True)]))
    out.append(Case("principal_point_outside", mm.cube_keys((8, -9, 8), (11, -6, 11)), SMALL, (45.0, 45.0, -25.0, 50.0),
                    [View(pose_of(np.eye(3), (0.0, 0.0, 0.0)), partial=True)]))
    out.append(Case("t_min_0", mm.cube_keys(-1, 2), SMALL, PLAIN,
                    [View(pose_of(ASKEW, (0.5, -0.3, -0.9)), 0.0, 5.0, partial=True),
                     View(pose_of(ASKEW, (0.1, 0.05, -S - 0.04)), 0.0, 5.0, full=True),         # 4 cm off a face: nearer than 0.05
                     View(pose_of(ASKEW, (0.07, 0.09, 0.11)), 0.0, 5.0, full=True)]))           # inside a cube
    column = [(0, 0, z) for z in range(10)] + [(4, 0, 6), (-3, 1, 7)]
    out.append(Case("t_max_cut", column, SMALL, PLAIN,
                    [View(pose_of(rot_y(0.03), (0.07, 0.09, -1.0)), 0.1, 1.0 + 3.5 * S, cut=True)]))
    # a cube of 0.4 pixels, 20 m away: its projection spans [cx, cx + 0.4] x [cy, cy + 0.4]
    lone = [(0, 0, 125)]
    origin = pose_of(np.eye(3), (0.0, 0.0, 0.0))
    out.append(Case("subpixel_between_centres", lone, SMALL, (50.0, 50.0, 19.3, 14.3), [View(origin, 0.1, 30.0, empty=True)]))
    out.append(Case("subpixel_on_a_centre", lone, SMALL, (50.0, 50.0, 18.8, 13.8), [View(origin, 0.1, 30.0, kept=1)]))
    # one cube [0, 0.16]^3 across the plane z = 0.999 t_min
    cube = [(0, 0, 0)]
    n = np.ones(3) / np.sqrt(3.0)
    diag = looking_along(n)
    side = np.array([0.01, -0.01, 0.0])                                                       # perpendicular to the diagonal
    out.append(Case("near_plane_4_corners", cube, (17, 9), (100.0, 100.0, -21.3, -19.6),      # (its right edge in the second tile, the far corners in the first)
                    [View(pose_of(np.eye(3), (0.07, 0.09, 0.5 * S - 0.3)), 0.3, 5.0, corners=4, partial=True)]))
    out.append(Case("near_plane_1_corner", cube, (33, 9), (40.0, 40.0, 19.2, 4.1),             # (the far corner in the third tile, the cut in the second to fourth)
                    [View(pose_of(diag, -0.07 * n + side), 0.3, 5.0, corners=1, partial=True)]))
    out.append(Case("near_plane_7_corners", cube, (15, 17), (20.0, 20.0, 7.2, 8.1),
                    [View(pose_of(diag, -0.25 * n + side), 0.3, 5.0, corners=7, partial=True)]))
    out.append(Case("near_plane_ragged", cube, (7, 5), (6.0, 6.0, 3.2, 2.1),
                    [View(pose_of(TILT, 0.5 * S - 0.29 * TILT[:, 2] + 0.01 * TILT[:, 0]), 0.3, 5.0, corners=3, partial=True)]))
    out.append(Case("camera_inside", cube, (17, 9), (20.0, 20.0, 8.2, 4.1),
                    [View(pose_of(rot_y(0.4) @ rot_x(-0.3), (0.08, 0.07, 0.03)), 0.05, 5.0, full=True, clipped=True)]))
    lump = [k for k in mm.cube_keys(-1, 2) if k not in ((1, 1, 1), (-1, 0, 1), (0, -1, -1))]
    centre = np.array([0.5 * S, 0.5 * S, 0.5 * S])
    turns = [View(pose_of(R, centre - 1.1 * R[:, 2] + 0.03 * R[:, 0] - 0.05 * R[:, 1]), partial=True)
             for R in (YAW90, YAW180, YAW270, PITCH90, PITCH270, ROLL180, YAW90 @ ROLL90)]
    out.append(Case("quarter_turns", lump, SMALL, PLAIN, turns))
    return out


# ---- (f) far from the origin ------------------------------------------------------------------------------------------
FAR_EXPONENTS = (10, 15, 18, 20)


def far_case(exponent):
    """6 x 6 x 4 blocks and a yawed camera 1.5 m off them, all moved by (2^k, -2^k, 2^k) blocks."""
    off = np.array([1, -1, 1], np.int64) << exponent
    keys = np.array(mm.cube_keys((0, 0, 0), (6, 6, 4)), np.int64) + off
    eye = off * S + np.array([1.8, 0.4, -1.5])
    views = [View(pose_of(rot_y(-0.35) @ rot_x(0.05), eye), 0.1, 5.0, partial=True),
             View(pose_of(rot_y(0.9) @ rot_x(-0.1), off * S + np.array([-1.3, 0.6, -0.9])), 0.1, 5.0, full=True),
             View(pose_of(rot_y(2.6) @ rot_x(0.4), off * S + np.array([0.1, 1.3, 1.9])), 0.1, 5.0, partial=True)]
    return Case(f"far_2^{exponent}", keys, SMALL, (300.0, 300.0, 19.3, 14.6), views)


# ---- all of them ------------------------------------------------------------------------------------------------------
_cases = {}


def all_cases():
    if not _cases:
        cs = [shape_case(W, H) for W, H in SHAPES] + [rounds_case(n) for n in ROUNDS] + [rounds_beside_case()]
        cs += [chunks_case(n) for n in CHUNKS] + [calls_case()] + geometry_cases() + [far_case(k) for k in FAR_EXPONENTS]
        for c in cs:
            assert c.name not in _cases
            _cases[c.name] = c
    return _cases


def names():
    return list(all_cases())


def case(name):
    return all_cases()[name]


# the views used on tables the frame path filled (the synthetic room of the suite), in a 64x48 image
ROOM_SIZE = (64, 48)
ROOM_INTRINSICS = (60.0, 58.0, 31.3, 23.6)


def room_views(keys, voxel_size=VS):
    """Three views of a model given by its keys: from outside its bounding box towards its middle, from its middle, and from
    inside one of its blocks with a far near plane."""
    lo, hi = br.cubes(keys, voxel_size)
    mid = (lo.min(0).astype(np.float64) + hi.max(0)) / 2
    out = [View(pose_of(rot_y(0.4) @ rot_x(0.1), mid - 2.5 * (rot_y(0.4) @ rot_x(0.1))[:, 2]), 0.1, 6.0),
           View(pose_of(rot_y(-2.0) @ rot_x(-0.2), mid), 0.3, 4.0)]
    k = np.asarray(keys, np.int64).reshape(-1, 3)
    if len(k):
        out.append(View(pose_of(rot_y(1.1), (k[len(k) // 2] * 8 + 3.5) * voxel_size), 0.5, 6.0))
    return out
