"""Crafted views of crafted models for the DDA raycast (tests/test_raycast_ref_cpu.py, tests/test_gpu_raycast_crafted.py): what
each case is there for is in its `why`.

Exact geometry: voxels of 1/64 m, fx = fy = 32, integer cx, cy, rotations with entries in {0, +-1} and translations that are
multiples of half a voxel make dx, dy, G and E exact dyadic numbers, so crossings of different axes fall on the SAME float
time: rays with |dx| = |dy| tie x with y at every event, power-of-two slopes give three-way ties, a camera on a voxel
boundary plane (G an integer) ties every axis of every ray at t = 1/2, the central row, column and pixel have inactive axes."""
import numpy as np

import mesh_models as mm

F = np.float32
VS = 0.015625
FOCAL = 32.0
SIZES = {"64x48": (64, 48, 32.0, 24.0), "40x24": (40, 24, 20.0, 12.0)}      # W, H, cx, cy
AXES = {"+x": (0, 1), "-x": (0, -1), "+y": (1, 1), "-y": (1, -1), "+z": (2, 1), "-z": (2, -1)}


def rotation(name):
    """The exact camera -> world rotation that looks along the named axis: right = the next axis, down = view x right."""
    axis, sign = AXES[name]
    d, right = np.zeros(3), np.zeros(3)
    d[axis], right[(axis + 1) % 3] = sign, 1
    return np.stack([right, np.cross(d, right), d], 1)


def pose_of(R, g):
    """The pose with rotation R whose camera centre is G = g in voxel-grid units (g integer: the camera lies on a voxel
    boundary plane on every axis; g = k + 1/2: at the centre of voxel k)."""
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (np.asarray(g, np.float64) - 0.5) * VS
    T = T.astype(F)
    assert np.array_equal(T[:3, 3] / F(VS) + F(0.5), np.asarray(g, F))
    return T


def general_pose(position):
    """Pitched, rolled and yawed by angles that are no round numbers: every entry an inexact float."""
    a, b, c = 0.3137, -0.2291, 0.1713
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = position
    return T.astype(F)


def shifted(model, by):
    return {tuple(int(k + o) for k, o in zip(key, by)): val for key, val in model.items()}


# ---- new models ----
def wall(view, g, lateral=(-3, 3), distance=16, plane=3.25, slope=0.25):
    """A slab of blocks one block deep, facing a camera at G = g (integers, multiples of 8 on the view axis) that looks along
    `view`: its near face `distance` voxels in front of the camera, holding the exact plane sdf = (coordinate - p0) * c on the
    view axis, p0 = `plane` voxels behind the near face, positive towards the camera.  Returns (model, p0)."""
    axis, sign = AXES[view]
    assert g[axis] % 8 == 0 and distance % 8 == 0
    near = g[axis] + sign * distance                          # the face, in grid units; voxel i covers [i, i + 1)
    block = near >> 3 if sign > 0 else (near >> 3) - 1
    p0 = (near + plane) - 0.5 if sign > 0 else (near - plane) - 0.5        # in voxel-centre coordinates
    i = np.arange(512)
    local = (i & 7, (i >> 3) & 7, i >> 6)[axis]
    sdf = ((block * 8 + local - p0) * (-sign * slope)).astype(F)
    model = {}
    o1, o2 = (axis + 1) % 3, (axis + 2) % 3
    for a in range(lateral[0], lateral[1]):
        for b in range(lateral[0], lateral[1]):
            key = [0, 0, 0]
            key[axis], key[o1], key[o2] = block, (g[o1] >> 3) + a, (g[o2] >> 3) + b
            model[tuple(key)] = (sdf.copy(), np.ones(512, F))
    return model, p0


def sparse(keys, seed, share=0.04):
    """Noise that is positive except for a small share of the voxels: most rays walk deep into the cluster before they hit."""
    rng = np.random.RandomState(seed)
    model = {}
    for k in keys:
        mag = rng.uniform(0.05, 1, 512)
        model[k] = (np.where(rng.uniform(size=512) < share, -mag, mag).astype(F), np.ones(512, F))
    return model


FAR_KEY = 1 << 17                                  # voxel coordinate 2^20: G has an ulp of 1/16 voxel there


def far_cluster(seed=31, key=FAR_KEY):
    return mm.uniform_model(mm.cube_keys((key, -1, -1), (key + 3, 2, 2)), seed)


TWO_GAP = 600                                      # blocks between the two clusters: 75 m


def two_clusters(seed=33, gap=TWO_GAP):
    """A near cluster with positive sdf only (no hit) and a noise cluster TWO_GAP blocks behind it along +z, seen through a long
    lens (focal 8192: the 64 x 48 rays stay inside a few blocks at 75 m)."""
    near = {k: (np.abs(s) + F(0.01), w) for k, (s, w) in mm.uniform_model(mm.cube_keys((0, 0, 2), (3, 3, 4)), seed).items()}
    near.update(mm.uniform_model(mm.cube_keys((-1, -1, gap + 4), (4, 4, gap + 6)), seed + 1))
    return near


# ---- cases ----
class Case:
    def __init__(self, name, model, pose, size="64x48", t=(0.1, 0.5), kinds=(), nan=False, why="", tables="a", forms=(2, 1, 0, 3),
                 focal=FOCAL, **facts):
        self.name, self.model, self.pose, self.size, self.t, self.focal = name, model, pose, size, t, focal
        self.kinds, self.nan, self.why, self.tables, self.forms, self.facts = set(kinds), nan, why, tables, forms, facts
        self.W, self.H, self.cx, self.cy = SIZES[size]

    def __repr__(self):
        return self.name


def front_camera(model, view, gap, half=False, lateral=(0, 0)):
    """G of a camera `gap` voxels in front of the model's bounding box, looking along `view` at the box's middle (moved by
    `lateral` voxels on the two other axes); half: at a voxel centre (G = k + 1/2), else on the boundary planes (G = k)."""
    keys = np.array(list(model.keys()))
    lo, hi = keys.min(0) * 8, keys.max(0) * 8 + 8
    axis, sign = AXES[view]
    g = ((lo + hi) // 2).astype(np.float64)
    g[(axis + 1) % 3] += lateral[0]
    g[(axis + 2) % 3] += lateral[1]
    g[axis] = lo[axis] - gap if sign > 0 else hi[axis] + gap
    return g + (0.5 if half else 0.0)


def build_cases():
    cases = []
    add = lambda *a, **k: cases.append(Case(*a, **k))
    views = list(AXES)
    # -- noise: many candidates per ray, straddling pairs, dead voxels; all six exact rotations, both kinds of translation
    noise = mm.every_configuration()
    # (the gap decides how many voxels of a block lie behind a ray's start, and with it how many pairs straddle a face)
    gaps = {"+x": 1, "-x": 0, "+y": 5, "-y": 5, "+z": 5, "-z": 0}
    for i, view in enumerate(views):
        half = bool(i & 1)
        add(f"noise{view}", noise, pose_of(rotation(view), front_camera(noise, view, gaps[view], half, (i - 2, 3 - i))), kinds={"noise", "tie"},
            tables="abcd" if view == "+z" else "ab" if view == "-x" else "a",
            why="candidates in several listed blocks, pairs across block boundaries, weight-0 voxels; camera at a voxel "
                + ("centre" if half else "boundary") + (", the rays enter from outside" if gaps[view] > 2 else ", t_min inside the first block"))
    for view in ("+z", "-x"):
        add(f"noise{view} deep", noise, next(c for c in cases if c.name == f"noise{view}").pose, t=(0.1, 5.0), kinds={"noise", "tie", "deep"}, tables="abcd",
            why="the range 0.1 .. 5 m: at this focal length a patch's beam grows wider than two blocks, the cooperative launch takes "
                "the per-lane walk (on the crowded table its set would overflow as well); the macro-cell level of the beam front end")
    add("noise+z small", noise, pose_of(rotation("+z"), front_camera(noise, "+z", 8, False)), size="40x24", kinds={"noise", "tie"},
        tables="ab", why="15 patches: a workgroup with waves that have no patch, patches partly outside the image")
    add("noise general", noise, general_pose((0.19, 0.17, 0.2)), t=(0.1, 0.3), kinds={"noise"}, tables="ab",
        why="a pitched and rolled pose of inexact floats with the camera inside the model")
    for seed in (0, 1, 2):
        m = mm.holes(seed)
        view = views[seed * 2]
        add(f"holes{seed}{view}", m, pose_of(rotation(view), front_camera(m, view, 6, seed == 1)), kinds={"holes"},
            why="absent blocks between allocated ones: pairs broken at a block's face, normals without a neighbour, "
                "negative coordinates")
    for name, builder, view, nan in (("zeros", mm.zeros, "-z", False), ("subnormals", mm.subnormals, "+y", False),
                                     ("wide_magnitudes", mm.wide_magnitudes, "-y", True), ("non_finite", mm.non_finite, "+x", True),
                                     ("weights", mm.weights, "+z", True), ("zero_gradient", mm.zero_gradient, "+x", False)):
        m = builder()
        add(name, m, pose_of(rotation(view), front_camera(m, view, 5, name in ("zeros", "weights"), (4, -4))), kinds={name}, nan=nan,
            tables="ab" if name in ("zeros", "weights") else "a",
            why={"zeros": "sdf +0 and -0 as the pair's second sample; a cluster across the origin",
                 "subnormals": "subnormal sdf in the interpolation and the gradient",
                 "wide_magnitudes": "|sdf| from 1e-30 to 1e3: the quotient next to 0 and 1, squares that overflow or vanish",
                 "non_finite": "inf and NaN sdf in the hit test, the interpolation, the normal's sqrt and divide",
                 "weights": "weights 0, -1, 1e-45, inf, NaN: only > 0 makes a sample",
                 "zero_gradient": "a gradient of length 0: no normal"}[name])
    origin = mm.uniform_model(mm.cube_keys(-1, 1), 41)
    add("origin-z", origin, pose_of(rotation("-z"), front_camera(origin, "-z", 1, False, (1, -1))), kinds={"noise", "tie"},
        why="keys -1..0: >> 3 and & 7 of negative voxel coordinates")
    # -- walls: exact planes behind 16 voxels of empty space, for the ties on the way and at the block's entry face
    for i, view in enumerate(views):
        for half in (False, True):
            g = np.array([8 * (i - 2), -16, 24]) + (np.array([3, -2, 5]) * (np.arange(3) != AXES[view][0]))
            m, p0 = wall(view, g)
            add(f"wall{view}{'c' if half else 'b'}", m, pose_of(rotation(view), g + (0.5 if half else 0.0)), kinds={"tie", "wall"},
                p0=p0, view=view,
                why="ties of two and three axes in the merge, in dda_advance and at the entry face of a listed block; "
                    "inactive axes; depth known in closed form")
    # -- far from the origin
    m = far_cluster()
    add("far", m, pose_of(rotation("+x"), front_camera(m, "+x", 1, False)), kinds={"noise"}, why="voxel coordinates at 2^20: G and the "
        "crossing times round to 1/16 voxel, the estimate in dda_advance is off by more than a voxel.  Only through the per-lane "
        "walk: the margin of a beam box grows with the coordinates (1e-5 of them: 10 voxels on either side here), so at 2^20 every "
        "box spans three blocks and the cooperative launch falls back whatever the range or the lens; see `far 2^16`")
    m = far_cluster(key=1 << 13)
    add("far 2^16", m, pose_of(rotation("+x"), front_camera(m, "+x", 1, False)), kinds={"noise"}, focal=64.0,
        why="voxel coordinates at 2^16 through a lens of twice the focal length: the farthest the cooperative walk itself gets "
            "(margin 0.7 voxel, most patches keep their boxes within two blocks): coop_entry and dda_advance inside a listed "
            "block with G and the crossing times rounded to 1/256 voxel")
    # -- ranges, on a model most rays walk deep into
    thin = sparse(mm.cube_keys(0, 3), 43)
    g = front_camera(thin, "+z", 8, False)
    for name, t, kind in (("t_min 0", (0.0, 0.5), "range"), ("starts inside", (0.15, 0.5), "starts"),
                          ("t_max inside", (0.1, 0.3), "ends"), ("t_max on a crossing", (0.1, 0.3125), "event")):
        add(f"range {name}", thin, pose_of(rotation("+z"), g), t=t, kinds={"range", kind}, tables="ab" if kind == "starts" else "a",
            why={"range": "t_min = 0: the per-lane walk from the camera", "starts": "the walk starts at voxel level, no entry event",
                 "ends": "t_max inside a block", "event": "t_max equal to a crossing time: that crossing is not taken"}[kind])
    # -- the cooperative form's far-block fall-back
    m = two_clusters()
    add("two clusters", m, pose_of(rotation("+z"), front_camera(m, "+z", 8, False)), t=(0.1, 80.0), kinds={"far_block"}, forms=(2, 1, 3), focal=8192.0,
        why="a listed block more than 511 blocks behind the wave's first: the patch takes the per-lane walk inside the "
            "cooperative launch; several depth windows (form 3 chooses the per-lane walk over this range; form 0 is "
            "the same walk without its front end and would step through 75 m of empty blocks one by one)")
    m = two_clusters(gap=300)
    add("long beam", m, pose_of(rotation("+z"), front_camera(m, "+z", 8, False)), t=(0.1, 40.0), kinds={"overflow"}, forms=(2,), focal=8192.0,
        tables="b", why="(cooperative launch forced: the case is about its fall-back) a thin beam through 320 blocks of depth on the crowded table: more than 256 cells with a set bit, the set overflows "
                        "and the patch takes the per-lane walk inside the cooperative launch; nearly every bit set and the key absent")
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# tables: (a) comfortable, (b) crowded with a prime bucket count, (c) a view table, (d) (a) after deleting a third of the keys
TABLES = {"a": dict(numBuckets=1 << 12, bucketSize=8), "b": dict(numBuckets=13, bucketSize=16),
          "c": dict(numBuckets=509, bucketSize=8), "d": dict(numBuckets=1 << 12, bucketSize=8)}
POOL = 128


def deleted_keys(model, seed=51):
    """About a third of the model's keys, the ones variant (d) deletes."""
    keys = sorted(model)
    rng = np.random.RandomState(seed)
    return [k for k in keys if rng.uniform() < 1 / 3]


def reduced(model):
    gone = set(deleted_keys(model))
    return {k: v for k, v in model.items() if k not in gone}


def reference(case, oracle, model=None):
    """(depth, normals, record) of tests/raycast_ref.py for the case (the inverse pose from the oracle's cofactor inverse)."""
    import raycast_ref
    return raycast_ref.raycast(case.model if model is None else model, VS, case.pose, oracle.invert4x4(case.pose), case.focal, case.focal,
                               case.cx, case.cy, case.W, case.H, *case.t)


def same_image(got, want, nan_rule):
    """The comparison rule: every word bit-equal; in the cases that are meant to produce NaN, NaN in the same places and
    every other word bit-equal (the sign and payload of a made-up NaN are nobody's rule)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    if not nan_rule:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def census_line(case, depth, record):
    f = record["found"]
    hits = max(1, int(f.sum()))
    ties = [int((record[k] > 0).sum()) for k in ("tie_xy", "tie_xz", "tie_yz", "tie_xyz")]
    return (f"{case.name:26s} hits={f.mean():.2f} candidates>=2={(record['candidates'][f] >= 2).sum() / hits:.2f} "
            f"straddles={record['straddles'].sum() / hits:.2f} ties xy/xz/yz/xyz={ties} inactive 1/2={int((record['inactive'] == 1).sum())}/"
            f"{int((record['inactive'] == 2).sum())} starts in={record['starts_in_allocated'].mean():.2f} "
            f"ends in={int((record['ends_in_allocated'] & ~f).sum())} t_max=event={int((record['tmax_equals_event'] & ~f).sum())} "
            f"broken by weight={int((record['broken_by_weight'] > 0).sum())} starved/one-sided normals={int(record['normal_starved'].sum())}/"
            f"{int(record['normal_one_sided'].sum())} NaN depths={int(np.isnan(depth).sum())} most events={int(record['events'].max())}")


# ---- what the cooperative form's beam step lists (for the fall-back cases) ----
def beam_cells(case, num_buckets, model=None):
    """(counts, wide): per 8x8 patch, whether some box spans more than two blocks on an axis (then the patch takes the per-lane
    walk whatever else holds) and the number of distinct blocks with a set bucket bit that the patch's beam touches: the boxes of the
    half-block slabs between t_min and t_max, from the patch's corner rays, with the margin DESIGN.md 4.6 gives them (float64:
    a count, not a bit pattern), tested against the buckets a table of `num_buckets` holding the model has entries in."""
    model = case.model if model is None else model
    set_buckets = set(mm.hash_block(list(model), num_buckets).tolist())
    T = case.pose.astype(np.float64)
    G = T[:3, 3] / VS + 0.5
    t0, t1 = case.t
    dt = 4.0 * VS
    out, wide = [], []
    for pv in range(0, case.H, 8):
        for pu in range(0, case.W, 8):
            corners = [(pu, pv), (pu + 7, pv), (pu, pv + 7), (pu + 7, pv + 7)]
            E = np.array([T[:3, :3] @ np.array([(u - case.cx) / case.focal, (v - case.cy) / case.focal, 1.0]) / VS for u, v in corners])
            lo, hi = E.min(0), E.max(0)
            ta = t0 + dt * np.arange(int(np.ceil((t1 - t0) / dt)))
            ta = ta[ta < t1]
            tA, tB = np.maximum(ta - 1e-4 * dt, 0)[:, None], (ta + 1.0001 * dt)[:, None]
            gl = G + np.minimum(tA * lo, tB * lo)
            gh = G + np.maximum(tA * hi, tB * hi)
            m = 0.02 + 1e-5 * np.maximum(np.abs(gl), np.abs(gh))
            k0, k1 = np.floor(gl - m).astype(np.int64) >> 3, np.floor(gh + m).astype(np.int64) >> 3
            wide.append(bool((k1 - k0 > 1).any()))
            cells = set()
            for a, b in zip(k0.tolist(), k1.tolist()):
                b = [min(q, p + 1) for p, q in zip(a, b)]
                for x in range(a[0], b[0] + 1):
                    for y in range(a[1], b[1] + 1):
                        for z in range(a[2], b[2] + 1):
                            cells.add((x, y, z))
            keys = np.array(sorted(cells))
            out.append(int(np.isin(mm.hash_block(keys, num_buckets), list(set_buckets)).sum()))
    return out, wide
