"""Incoherent depth and loaded tables for the frame path: the inputs of tests/test_gpu_incoherent.py and a CPU census that
says which paths of the claim / walk code a frame reaches (tests/test_incoherent_cases_cpu.py asserts it on the oracle alone).

Every frame the other suites fuse is a smooth surface, where the wave-level de-duplication of vh_alloc.hip leaves a handful
of keys per launch tile.  Three pieces of code exist for the other case only:
  claim_tile_wave   queues a TILE's survivors in waveKeys[..][kWaveQueue = 64] and probes and refills at count + n > 64;
  claim_tile        (band) queues a WAVE's keys in queues[..][kClaimQueue = 128] and drains inside the sample loop;
  flatten_index_tile_to   gives each wave a 512-bucket list for the 8192 buckets it covers, takes further passes beyond 512
                    occupied ones and reads slots 2.. only behind a live slot 1.
The inputs here are the smallest that reach them: a 64x64 image (16 launch tiles, 64 waves) of independent depths.

Everything in this module runs on the CPU, from numpy and the oracle.  The de-duplication rule and the block key are
restated in numpy (block_keys is checked against oracle.world2block by the CPU test)."""
import numpy as np

from voxelhashing_demo_amd import synth

SIZE = 64                        # incoherent64 / duplicates64: 64x64 pixels
Z_LO, Z_HI = 0.5, 3.5            # metres
INVALID_SHARE = 0.01
LARGE = (1024, 640)              # large_patchy: 2560 launch tiles (> 2400: the tile per wave)
SEQ_SEEDS = tuple(range(100, 106))      # the loaded sequences: six frames
PLAIN_SEEDS = (5, 6)                     # plain and band frames (a third frame repeats the first)
SHARD_SEEDS = (200, 201, 202, 203)       # two cameras x two frames
DUP_SEEDS = (5, 6)
PATCHY_SEEDS = (5, 6, 7, 8)               # large_patchy(seed) copies incoherent64(seed)
ALL_SEEDS = tuple(sorted(set(PLAIN_SEEDS + PATCHY_SEEDS + SEQ_SEEDS + SHARD_SEEDS)))
LOADED_KW = dict(numBuckets=2048, bucketSize=5, numVoxelBlocks=12288)
CHAINED_KW = dict(numBuckets=1024, bucketSize=2, numVoxelBlocks=12288, attachedLinkedListSize=8)
WAVE_SPAN = 8192                 # buckets one wave of the occupancy-index walk covers (64 lanes x 4 words x 32 bits)
INDEX_QUEUE = 512                # buckets a wave lists per pass (vh_walk.hip: kIndexQueue)


def k_inv(width=SIZE, height=SIZE):
    return np.linalg.inv(synth.K_matrix(width, height).astype(np.float64)).astype(np.float32)


def incoherent_depth(seed):
    """float32 [64, 64] camera z, independent per pixel, uniform in 0.5 .. 3.5 m; about 1 % of the pixels 0 (invalid)."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(Z_LO, Z_HI, (SIZE, SIZE)).astype(np.float32)
    z[rng.uniform(size=(SIZE, SIZE)) < INVALID_SHARE] = 0.0
    return z


def incoherent64(seed):
    """The vertex-map form."""
    return synth.verts_from_depth(incoherent_depth(seed), SIZE, SIZE)


def incoherent64_u16(seed):
    """The sensor form (5000 per metre) of the same depths, for integrate_depth; the oracle's side takes
    oracle.preprocess(d16, k_inv())."""
    return np.round(incoherent_depth(seed) * 5000.0).clip(0, 65535).astype(np.uint16)


def duplicates64(seed):
    """The same size with depths from only 8 values per 16x16 tile (each tile's 8 out of a pool of 12, so that tiles share
    keys too), laid out as value[(a x + b y + c) mod 8] with a odd and b not a multiple of 8: no pixel's depth equals its
    left or upper neighbour's inside a tile, so next to nothing is collapsed inside a wave (two of the eight depths may share
    a block), and one key is demanded by many lanes and waves."""
    rng = np.random.RandomState(seed)
    pool = rng.uniform(Z_LO, Z_HI, 12).astype(np.float32)
    z = np.zeros((SIZE, SIZE), np.float32)
    y, x = np.mgrid[0:16, 0:16]
    for ty in range(SIZE // 16):
        for tx in range(SIZE // 16):
            vals = pool[rng.permutation(12)[:8]]
            a, b, c = rng.choice([1, 3, 5, 7]), rng.choice([1, 2, 3, 5, 6, 7]), rng.randint(8)
            z[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = vals[(a * x + b * y + c) % 8]
    z[rng.uniform(size=(SIZE, SIZE)) < INVALID_SHARE] = 0.0
    return synth.verts_from_depth(z, SIZE, SIZE)


def large_patchy(seed):
    """1024x640 vertex map, invalid except for patches of incoherent64(seed)'s vertices (a vertex need not agree with its
    pixel: allocation follows the vertex, the TSDF update reads z at the projection, on both sides):
      - a 32x32 patch on a tile boundary in the image's first rows (four whole launch tiles),
      - a 32x16 patch in the last two launch tiles (2558, 2559: the last claim workgroup's last waves),
      - a 16x16 patch off the tile grid (four tiles, each partly covered),
      - a 3x2 and a 1x1 patch alone in their tiles (a wave with one lane, a tile with six survivors at most).
    The positions of all but the second move with the seed."""
    W, H = LARGE
    rng = np.random.RandomState(seed + 7919)
    src = incoherent64(seed)
    out = np.zeros((H, W, 4), np.float32)
    out[..., 3] = 1.0

    def put(x0, y0, w, h, sx, sy):
        out[y0:y0 + h, x0:x0 + w] = src[sy:sy + h, sx:sx + w]

    put(16 * rng.randint(0, 60), 16 * rng.randint(0, 3), 32, 32, 0, 0)
    put(W - 32, H - 16, 32, 16, 32, 0)
    put(16 * rng.randint(4, 58) + rng.randint(1, 15), 16 * rng.randint(8, 30) + rng.randint(1, 15), 16, 16, 0, 32)
    put(16 * rng.randint(0, 60) + rng.randint(0, 13), 16 * rng.randint(32, 36) + rng.randint(0, 14), 3, 2, 40, 40)
    put(16 * rng.randint(0, 60) + rng.randint(0, 16), 16 * 37 + rng.randint(0, 16), 1, 1, 50, 50)
    return out


def sequence_pose(s):
    """The loaded sequences' camera: a few degrees per frame."""
    return synth.yaw_pose(3.0 * s, (0.01 * s, 0.0, 0.02 * s))


def sequence(seeds=SEQ_SEEDS):
    """[(pose, verts)]: frames of incoherent64, a new seed each."""
    return [(sequence_pose(s), incoherent64(seed)) for s, seed in enumerate(seeds)]


# ---- the census ----
def _rz(x):
    """float -> int32 as v_cvt_i32_f32: toward zero, saturating, NaN -> 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.where(x >= np.float32(2147483648.0), np.int64(2147483647),
                     np.where(x <= np.float32(-2147483648.0), np.int64(-2147483648),
                              np.trunc(np.where(np.isfinite(x), x, np.float32(0.0))).astype(np.int64)))
    return np.where(np.isnan(x), 0, r).astype(np.int32)


def block_keys(pose, verts, voxel_size=0.02):
    """int32 [H, W, 3]: the block every pixel's vertex falls into -- global_transform * v with each row summed left to right,
    world2Voxel's true divide and round half away from zero, voxel2Block's floor division by 8 -- in float32 / wrapping int32
    as the oracle does it (oracle/vh_oracle.c: vho_mat4_mul_vec4, vho_world2block)."""
    T = np.asarray(pose, np.float32).reshape(4, 4)
    v = np.asarray(verts, np.float32)
    vs = np.float32(voxel_size)
    out = np.empty(v.shape[:-1] + (3,), np.int32)
    with np.errstate(all="ignore"):
        for r in range(3):
            g = ((T[r, 0] * v[..., 0] + T[r, 1] * v[..., 1]) + T[r, 2] * v[..., 2]) + T[r, 3] * v[..., 3]
            q = (g / vs).astype(np.float32)
            half = _rz(np.copysign(np.float32(1.0), q)).astype(np.float32) * np.float32(0.5)
            c = _rz(q + half)
            c = np.where(c < 0, (c.astype(np.int64) - 7 + 2 ** 31) % 2 ** 32 - 2 ** 31, c).astype(np.int32)      # wrapping c - 7
            out[..., r] = (np.abs(c.astype(np.int64)) // 8 * np.sign(c)).astype(np.int32)                        # C's c / 8
    return out


def survivors(pose, verts):
    """(per_wave, per_tile) counts of the keys that survive the wave-level collapse, before the frustum test -- what
    claim_tile_wave queues.  A wave is a 16x4 patch of a 16x16 launch tile; a lane is silent when its left or upper
    neighbour IN THE WAVE is valid and has the same block.  per_wave[4 * tile + w], tiles x-fastest (launch order)."""
    v = np.asarray(verts, np.float32)
    H, W = v.shape[:2]
    keys = block_keys(pose, v)
    valid = v[..., 2] != 0.0
    y, x = np.mgrid[0:H, 0:W]
    same_left = np.zeros((H, W), bool)
    same_left[:, 1:] = valid[:, :-1] & np.all(keys[:, 1:] == keys[:, :-1], axis=-1)
    same_up = np.zeros((H, W), bool)
    same_up[1:] = valid[:-1] & np.all(keys[1:] == keys[:-1], axis=-1)
    alive = valid & ~(same_left & ((x & 15) != 0)) & ~(same_up & ((y & 3) != 0))
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    wave = ((y >> 4) * tiles_x + (x >> 4)) * 4 + ((y & 15) >> 2)
    per_wave = np.bincount(wave[alive], minlength=tiles_x * tiles_y * 4)
    return per_wave, per_wave.reshape(-1, 4).sum(axis=1)


def band_keys_per_wave(oracle, pose, verts, band, mode, normals=None, sem=1, capacity=1 << 19):
    """Keys per wave under an allocation band, from OracleTable.generate_keys on an empty table (one shard): a record's rank
    field is launch rank << 6 | sample, launch rank = tile << 8 | lane, so rank >> 12 is the wave.  A LOWER bound on what the
    wave queues: the GPU queues a key before the frustum test, generate_keys records it after (and collapses runs along an
    image row only, across the tile's edge too).  VH_BAND_NORMAL_DDA: generate_keys walks the same pixel_keys() as the frame
    and reads the table's normal map, which set_normals() hands it -- exact, nothing restated.
    Returns (per_wave, total)."""
    v = np.ascontiguousarray(verts, np.float32)
    H, W = v.shape[:2]
    ot = oracle.OracleTable(oracle.default_params(numBuckets=1 << 12, numVoxelBlocks=16), W, H, sem)
    ot.set_alloc_band(band, mode)
    if normals is not None:
        ot.set_normals(normals)
    ot.set_pose(pose)
    bins, _ = ot.generate_keys(v, 0, 1, capacity)
    n = int(bins[0, 0, 0])
    ranks = bins[0, 1:1 + n, 3].astype(np.int64) & 0x7FFFFFF
    per_wave = np.bincount(ranks >> 12, minlength=((W + 15) // 16) * ((H + 15) // 16) * 4)
    ot.close()
    return per_wave, n


def table_census(ot):
    """After a frame on an oracle table: entries per bucket, occupied buckets per aligned span of 8192 (one wave of the
    index walk; more than 512 means further passes), chain links, load, and the frame's last_stats."""
    tab = ot.hash_table()
    bs = ot.params.bucketSize
    per_bucket = (tab["ptr"] != -1).reshape(-1, bs).sum(axis=1)
    occ = per_bucket > 0
    spans = [int(occ[s:s + WAVE_SPAN].sum()) for s in range(0, len(occ), WAVE_SPAN)]
    return dict(per_bucket=per_bucket, occupied_per_span=spans, passes=[-(-s // INDEX_QUEUE) for s in spans],
                buckets_3plus=int((per_bucket >= 3).sum()), buckets_full=int((per_bucket == bs).sum()),
                links=int((tab["offset"] != 0).sum()), load=float(per_bucket.sum()) / len(tab), entries=int(per_bucket.sum()),
                stats=dict(ot.last_stats) if ot.last_stats else None)


def launch_ranks(width, height):
    """int64 [H, W]: a pixel's position in the launch order (16x16 tiles x-fastest, lanes x-fastest inside a tile)."""
    y, x = np.mgrid[0:height, 0:width]
    return (((y >> 4) * ((width + 15) // 16) + (x >> 4)) << 8) + ((y & 15) << 4) + (x & 15)


def winners_by_definition(ot, oracle, pose, verts):
    """The keys a frame inserts into `ot` in its plain form (no band, no overflow list), by the rule itself and not by the
    oracle's loop (oracle/vh_oracle.c: insert_entry against VoxelUtils.cu:418-456): among the frame's valid pixels whose block
    passes the frustum test and is not in the table, per bucket the one of lowest launch rank wins; it is inserted if the
    bucket has a free slot and the heap a block.  `ot` must have the frame's pose set (set_pose); it is not changed.
    Returns the set of inserted keys; the heap must hold a block for each (asserted), so that none is refused."""
    v = np.asarray(verts, np.float32)
    H, W = v.shape[:2]
    keys = block_keys(pose, v).reshape(-1, 3)
    valid = (v[..., 2] != 0.0).reshape(-1)
    rank = launch_ranks(W, H).reshape(-1)
    tab = ot.hash_table()
    live = tab["ptr"] != -1
    present = set(map(tuple, tab["pos"][live].tolist()))
    free = ot.params.bucketSize - live.reshape(-1, ot.params.bucketSize).sum(axis=1)
    nb = ot.params.numBuckets
    best = {}                                       # bucket -> (rank, key)
    seen = {}                                       # key -> (in frustum, bucket)
    for i in np.nonzero(valid)[0][np.argsort(rank[valid], kind="stable")]:
        k = tuple(int(c) for c in keys[i])
        if k not in seen:
            seen[k] = (ot.block_in_frustum(k), oracle.hash_block(*k, nb))
        ok, h = seen[k]
        if ok and k not in present and h not in best:
            best[h] = k
    out = {k for h, k in best.items() if free[h] > 0}
    assert len(out) <= ot.heap_counter() + 1, "the heap would run dry: which winners are refused is not part of the rule"
    return out
