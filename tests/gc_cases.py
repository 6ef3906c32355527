"""Crafted buckets, chains and voxels for block deletion and collection (vh_delete_blocks, vh_garbage_collect; vh_gc.hip),
shared by tests/test_gc_cases_cpu.py (the oracle against the definition, and the coverage of the cases) and
tests/test_gpu_gc_crafted.py.

A CASE is one table and one call.  Every table is a state the library's own insertion produces: the oracle's insert_blocks over
the case's keys in the case's order (with the overflow list where chains are wanted); the voxels are written through the
oracle's sdf_blocks() view.  No link is forged.  A GPU context receives the state slot for slot as a snapshot.

Family P, PLAIN BUCKETS (bucketSize 5, no list): for every n = 1..5 and every mask of n bits one bucket of n entries whose doomed
        subset is the mask -- 62 buckets of a 64-bucket table, one call; the same with a shuffled list, keys twice, absent keys.
Family C, ONE CHAIN: bucketSize 2, list size 6: slot 0, the head and 5 chained entries (offsets 9 -> 7 -> 5 -> 3 -> 1 from the
        head, slot 0 of the five buckets behind); every one of the 128 subsets, 64 groups a table.  And bucketSize 4, list size 4.
Family I, INTERLEAVED CHAINS: homes h and h+1 with 4 entries each, their chained entries alternating in slot 0 of h+2 .. h+5, whose
        last slots hold an entry of their own; 16 x 16 subsets x (hosts' own entries deleted / kept), 64 groups a table.
Family W, WRAP: C's chain on the last bucket of a table and of a shard (a bucket range that starts above 0); one table a mask.
Family V, VOXELS THAT DECIDE: blocks kept or deleted by exactly one voxel, special weights, sdf values and thresholds.

check_after states what a deletion must leave, from the definition; expected_plain is the compaction without the list."""
import itertools

import numpy as np

import mesh_models as mm

F = np.float32
ENTRY, VOXEL = mm.ENTRY, mm.VOXEL
NAN, INF = float("nan"), float("inf")
T = F(0.05)                                            # the threshold of family V
FAR = F(0.5)
GROUP = 6                                              # buckets of one group of the families C and I
GROUPS = 64                                            # groups a table


BACK = np.eye(4, dtype=F)                              # the camera of the delete_blocks families: 100 blocks behind the origin,
BACK[2, 3] = -16.0                                     # so that every key with small x, y >= 0 and any z >= 0 is in its frustum


def up(v):
    return F(np.nextafter(F(v), F(np.inf)))


def dn(v):
    return F(np.nextafter(F(v), F(-np.inf)))


def search_keys(num_buckets, want):
    """{bucket: [keys]} with want[bucket] keys each, from a search over small x, y, z >= 0 (any bucket count)."""
    r = np.arange(64)
    cand = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)[:, ::-1]
    bucket = mm.hash_block(cand, num_buckets)
    out = {}
    for b, n in want.items():
        at = np.nonzero(bucket == b)[0][:n]
        assert len(at) == n, f"bucket {b}: {len(at)} of {n} keys found"
        out[b] = [tuple(int(c) for c in cand[i]) for i in at]
    return out


def bucket_keys(num_buckets, want):
    """{bucket: [keys]}: mesh_models.key_for_bucket for a power-of-two table, the search otherwise."""
    if num_buckets & (num_buckets - 1):
        return search_keys(num_buckets, want)
    return {b: [mm.key_for_bucket(3 + i, 7 + (b % 5), b, num_buckets) for i in range(n)] for b, n in want.items()}


class Case:
    """table: the parameters; overflow; bucket_range (None: the whole table); insert: the keys in the order the oracle places
    them; fill(key, i) -> (sdf[512], weight[512]) of the i-th placed key; then ONE call: `keys` (delete_blocks' list, with
    whatever absent, foreign and repeated keys the case wants) or `threshold` (garbage_collect behind a flatten at `pose`)."""

    W, H, sem = 64, 48, 1

    def __init__(self, name, family, table, insert, overflow=False, bucket_range=None, keys=None, threshold=None, fill=None,
                 pose=None, **facts):
        self.name, self.family, self.table, self.overflow = name, family, dict(table), overflow
        self.bucket_range, self.insert, self.keys, self.threshold = bucket_range, list(insert), keys, threshold
        self.fill = fill or pattern_block
        self.pose = (np.eye(4, dtype=F) if family == "V" else BACK) if pose is None else pose
        self.facts = facts                             # what the generator aimed at
        if keys is not None and "back" not in facts:   # the calls that put the doomed keys back: one, where any order places them all
            self.facts["back"] = [sorted(facts["doomed"])] if facts["doomed"] else []

    def params(self, module):
        return module.default_params(**self.table)

    @property
    def shape(self):
        lo, hi = self.bucket_range or (0, self.table["numBuckets"])
        return dict(numBuckets=self.table["numBuckets"], bucketSize=self.table["bucketSize"],
                    listSize=self.table.get("attachedLinkedListSize", 0), overflow=self.overflow, lo=lo, hi=hi)

    def proj(self):
        return np.array((2, 0, self.W / 2, 0, 2, self.H / 2, 0, 0, 1), F)

    def key_list(self):
        k = np.zeros((len(self.keys), 4), np.int32)
        k[:, :3] = np.asarray(self.keys, np.int32).reshape(-1, 3)
        return k


def pattern_block(key, i):
    """A block that holds no zero word and differs from every other: both fields of every voxel are non-zero."""
    v = np.arange(512, dtype=F)
    return (v + F(1)) * F(0.001) + F(i), np.full(512, F(1 + i % 7))


def load_oracle(oracle, c):
    """The oracle's table of the case: inserted in order, filled, nothing deleted yet."""
    ot = oracle.OracleTable(c.params(oracle), c.W, c.H, c.sem, bucket_range=c.bucket_range)
    ot.set_projection(c.proj())
    if c.overflow:
        ot.set_overflow(True)
    placed = ot.insert_blocks(c.insert)
    lo, hi = c.shape["lo"], c.shape["hi"]
    mine = [k for k in c.insert if lo <= mm.hash_block([k], c.table["numBuckets"])[0] < hi]
    assert placed == len(mine) == len(set(mine)), f"{c.name}: {placed} of {len(mine)} keys placed"
    tab, vol = ot.hash_table(), ot.sdf_blocks()
    where = {tuple(e["pos"].tolist()): int(e["ptr"]) for e in tab[tab["ptr"] != -1]}
    for i, k in enumerate(mine):
        s, w = c.fill(k, i)
        vol["sdf"][where[k]:where[k] + 512], vol["weight"][where[k]:where[k] + 512] = s, w
    return ot


def state_of(ot):
    """A copy of an oracle table's state, in the form of test_gpu_deintegrate.snapshot."""
    return dict(table=ot.hash_table().copy(), heap=ot.heap().copy(), vox=ot.sdf_blocks().copy(), heap_counter=ot.heap_counter())


def oracle_call(c, ot):
    """The case's call on the oracle; returns what it freed."""
    if c.keys is not None:
        return ot.delete_blocks(c.keys)
    ot.set_pose(c.pose)
    assert ot.flatten() == len(c.insert)
    return ot.garbage_collect(float(c.threshold))


def _void(pos):
    return np.ascontiguousarray(np.asarray(pos, "<i4").reshape(-1, 3)).view(np.dtype((np.void, 12))).ravel()


def holds(pos, keys):
    """[N] bool: which rows of pos [N, 3] are in the key set."""
    if not len(keys):
        return np.zeros(len(pos), bool)
    return np.isin(_void(pos), _void(sorted(keys)))


def key_set(table):
    return set(map(tuple, table["pos"][table["ptr"] != -1].tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------------
def lookup(table, key, s):
    """The lookup restated: the slots of the home bucket (without the list: up to the first free one), then the chain from the
    last slot, at most list-size steps.  Entry index or None."""
    h = int(mm.hash_block([key], s["numBuckets"])[0])
    if not s["lo"] <= h < s["hi"]:
        return None
    bs = s["bucketSize"]
    start = (h - s["lo"]) * bs
    for i in range(start, start + bs):
        e = table[i]
        if e["ptr"] == -1:
            if not s["overflow"]:
                return None
            continue
        if tuple(e["pos"].tolist()) == tuple(key):
            return i
    if not s["overflow"]:
        return None
    last, i = start + bs - 1, start + bs - 1
    for _ in range(s["listSize"]):
        e = table[i]
        if e["ptr"] != -1 and tuple(e["pos"].tolist()) == tuple(key):
            return i
        if e["offset"] == 0:
            return None
        i = (last + int(e["offset"])) % len(table)
    return None


def chains(table, s):
    """{home bucket: [entry indices of its chained entries, in chain order]} (with the list)."""
    bs, out = s["bucketSize"], {}
    for b in range(len(table) // bs):
        last = b * bs + bs - 1
        if table[last]["ptr"] == -1:
            assert table[last]["offset"] == 0, f"bucket {b}: a free last slot with a chain behind it"
            continue
        i, seen = last, []
        for _ in range(s["listSize"]):
            if table[i]["offset"] == 0:
                break
            i = (last + int(table[i]["offset"])) % len(table)
            seen.append(i)
        else:
            assert table[i]["offset"] == 0 or len(seen) < s["listSize"], f"bucket {b}: the chain does not end"
        if seen:
            out[b] = seen
    return out


def check_after(pre, post, doomed, s, freed=None):
    """What deleting the key set `doomed` from the state `pre` must leave in `post` (both dicts: table, heap, heap_counter, vox),
    for the table shape `s` (Case.shape), written from the definition of the calls.  freed: (last_freed, freed_total before,
    freed_total after) where the caller has them.  Returns the number of blocks freed."""
    a, b = pre["table"], post["table"]
    bs = s["bucketSize"]
    ua, ub = a["ptr"] != -1, b["ptr"] != -1
    ka, kb = key_set(a), key_set(b)
    gone = ka & set(doomed)
    assert kb == ka - set(doomed), "keys after != keys before - doomed"
    assert ub.sum() == len(kb), "a key is held twice"
    # survivors: ptr and voxel bits
    where_a = dict(zip(map(tuple, a["pos"][ua].tolist()), a["ptr"][ua].tolist()))
    pos_b, ptr_b = b["pos"][ub], b["ptr"][ub]
    assert np.array_equal(ptr_b, np.array([where_a[k] for k in map(tuple, pos_b.tolist())], np.int64)), "a survivor changed its block"
    va, vb = pre["vox"].view(np.uint32).reshape(-1, 1024), post["vox"].view(np.uint32).reshape(-1, 1024)
    assert np.array_equal(va[ptr_b // 512], vb[ptr_b // 512]), "a survivor's voxels changed"
    # every survivor is found
    at = np.nonzero(ub)[0]
    if not s["overflow"]:                              # (all of them at once: each sits in the bucket of its key; the prefix is below)
        assert np.array_equal(mm.hash_block(b["pos"][at], s["numBuckets"]) - s["lo"], at // bs), "an entry outside its home bucket"
        at = at if len(at) <= 8192 else at[::16]       # the lookup itself, entry by entry: a sample where the table is large
    for i in at:
        assert lookup(b, b["pos"][i].tolist(), s) == i, f"entry {i} {b['pos'][i].tolist()} is not found by the lookup"
    free = b[~ub]
    assert (free["offset"] == 0).all(), "a free slot with an offset"
    if not s["overflow"]:
        rows = ub.reshape(-1, bs)
        assert (rows[:, :-1] >= rows[:, 1:]).all(), "entries are no prefix of their bucket"
        assert (b["offset"] == 0).all()
        # old order: the survivors of every bucket, read in slot order, are the old bucket's with the doomed left out
        keep = ua & ~holds(a["pos"], gone)
        bucket_a, bucket_b = np.nonzero(keep)[0] // bs, np.nonzero(ub)[0] // bs
        assert np.array_equal(bucket_a, bucket_b) and np.array_equal(a["pos"][keep], b["pos"][ub]), "the old order is lost"
    else:
        reach = chains(b, s)
        seen = [i for c in reach.values() for i in c]
        assert len(seen) == len(set(seen)), "an entry is reachable from two chains"
        for home, c in reach.items():
            for i in c:
                assert b["ptr"][i] != -1 and i % bs != bs - 1, f"chain of bucket {home}: slot {i}"
                assert int(mm.hash_block([b["pos"][i].tolist()], s["numBuckets"])[0]) - s["lo"] == home
        away = [int(i) for i in np.nonzero(ub)[0] if int(mm.hash_block([b["pos"][i].tolist()], s["numBuckets"])[0]) - s["lo"] != i // bs]
        assert sorted(away) == sorted(seen), "entries outside their home bucket != the entries on chains"
    # the heap: the new part, as a set, is the freed block ids; freed blocks are zero; the old part stands
    c0, c1 = pre["heap_counter"], post["heap_counter"]
    ids = sorted(where_a[k] // 512 for k in gone)
    assert c1 - c0 == len(gone)
    assert sorted(post["heap"][c0 + 1:c1 + 1].tolist()) == ids, "the pushed block ids are not the freed ones"
    assert np.array_equal(post["heap"][:c0 + 1], pre["heap"][:c0 + 1])
    assert not vb[ids].any(), "a freed block is not zero"
    live = sorted((ptr_b // 512).tolist() + post["heap"][:c1 + 1].tolist())
    assert live == list(range(len(vb))), "entries and free list do not partition the pool"
    if freed is not None:
        last, before, after = freed
        assert last == len(gone) and after - before == len(gone), (freed, len(gone))
    return len(gone)


def expected_plain(table_pre, doomed, bucket_size):
    """Without the list: every bucket's surviving entries moved down in order, the rest of its slots free."""
    out = table_pre.copy().reshape(-1, bucket_size)
    hit = (holds(table_pre["pos"], doomed) & (table_pre["ptr"] != -1)).reshape(-1, bucket_size)
    free = np.zeros((), ENTRY)
    free["pos"], free["ptr"] = 0x7FFFFFFF, -1
    for r in np.nonzero(hit.any(1))[0]:
        keep = out[r][(out[r]["ptr"] != -1) & ~hit[r]]
        out[r] = free
        out[r][:len(keep)] = keep
    return out.reshape(-1)


def collect_rule(sdf, weight, threshold):
    """garbage_collect's decision for one block, from the header: deleted iff its max weight is 0 (no voxel has weight > 0:
    the max is floored at 0, a NaN weight is no weight) or the min |sdf| over the voxels with weight > 0 (a NaN sdf is no
    sample; none at all: +inf) is >= threshold.  A NaN threshold compares false: only the unobserved blocks go."""
    with np.errstate(invalid="ignore"):
        seen = np.asarray(weight, F) > 0
        if not seen.any():
            return True
        a = np.abs(np.asarray(sdf, F)[seen])
        a = a[~np.isnan(a)]
        m = F(a.min()) if len(a) else F(np.inf)
        return bool(m >= F(threshold))


# ---------------------------------------------------------------------------------------------------------------------------------
# family P
# ---------------------------------------------------------------------------------------------------------------------------------
P_TABLE = dict(numBuckets=64, bucketSize=5, numVoxelBlocks=512)


def p_layout():
    """[(bucket, n, mask)] over n = 1..5 and every mask of n bits, and {bucket: keys}."""
    plan = [(n, m) for n in range(1, 6) for m in range(1 << n)]
    plan = [(b, n, m) for b, (n, m) in enumerate(plan)]
    return plan, bucket_keys(64, {b: n for b, n, _ in plan})


def p_case(shuffled):
    plan, keys = p_layout()
    insert = [k for b, n, _ in plan for k in keys[b]]
    doomed = [keys[b][i] for b, n, m in plan for i in range(n) if m >> i & 1]
    patterns = {(n, m) for _, n, m in plan}
    assert len(plan) == 62 and len(patterns) == 2 + 4 + 8 + 16 + 32
    call, absent = list(doomed), []
    if shuffled:
        twice = [keys[b][i] for b, n, m in plan[::3] for i in range(n) if m >> i & 1]
        listed = next(b for b, n, m in plan if m and n < 5)
        absent = [mm.key_for_bucket(40, 41, listed, 64), mm.key_for_bucket(40, 42, 63, 64)]      # a listed and an empty bucket
        assert not set(absent) & set(insert) and len(twice) > 20
        call = doomed + twice + absent
        call = [call[i] for i in np.random.RandomState(5).permutation(len(call))]
    return Case("P-shuffled" if shuffled else "P-plain", "P", P_TABLE, insert, keys=call, doomed=set(doomed), plan=plan,
                bucket_keys=keys, absent=absent)


# ---------------------------------------------------------------------------------------------------------------------------------
# families C, I and W
# ---------------------------------------------------------------------------------------------------------------------------------
C_TABLE = dict(numBuckets=GROUP * GROUPS, bucketSize=2, numVoxelBlocks=1024, attachedLinkedListSize=6)
C4_TABLE = dict(numBuckets=256, bucketSize=4, numVoxelBlocks=1024, attachedLinkedListSize=4)


def c_case(part):
    """Groups g = 64 * part .. +63: home bucket 6 * (g % 64) with 7 colliding keys, mask g."""
    keys = bucket_keys(C_TABLE["numBuckets"], {GROUP * j: 7 for j in range(GROUPS)})
    insert = [k for j in range(GROUPS) for k in keys[GROUP * j]]
    masks = [GROUPS * part + j for j in range(GROUPS)]
    doomed = [keys[GROUP * j][i] for j, m in enumerate(masks) for i in range(7) if m >> i & 1]
    return Case(f"C-{part}", "C", C_TABLE, insert, overflow=True, keys=doomed, doomed=set(doomed), masks=masks,
                homes=[GROUP * j for j in range(GROUPS)], per_home=7)


def c4_case():
    """bucketSize 4, list size 4: 4 slots and 3 chained entries (all in the bucket behind), 128 groups of 2 buckets, mask g."""
    keys = bucket_keys(256, {2 * g: 7 for g in range(128)})
    insert = [k for g in range(128) for k in keys[2 * g]]
    doomed = [keys[2 * g][i] for g in range(128) for i in range(7) if g >> i & 1]
    return Case("C-bucket4", "C", C4_TABLE, insert, overflow=True, keys=doomed, doomed=set(doomed), masks=list(range(128)),
                homes=[2 * g for g in range(128)], per_home=7)


I_TABLE = dict(numBuckets=GROUP * GROUPS, bucketSize=2, numVoxelBlocks=1024, attachedLinkedListSize=6)


def i_case(part):
    """Groups g = 64 * part .. +63 of 512: homes h = 6 * (g % 64) and h + 1 with 4 keys each, inserted in turn (a1 a2 b1 b2 a3
    b3 a4 b4), then one key of its own for each of h+2 .. h+5 (slot 0 is taken: it lands in the last slot).  Mask of home a =
    g & 15, of home b = g >> 4 & 15, the hosts' own entries are deleted iff g >> 8."""
    want = {}
    for j in range(GROUPS):
        want.update({GROUP * j: 4, GROUP * j + 1: 4, **{GROUP * j + 2 + k: 1 for k in range(4)}})
    keys = bucket_keys(I_TABLE["numBuckets"], want)
    insert, doomed, combos, roles, owns = [], [], [], [], []
    for j in range(GROUPS):
        g, h = GROUPS * part + j, GROUP * j
        a, b = keys[h], keys[h + 1]
        own = [keys[h + 2 + k][0] for k in range(4)]
        insert += [a[0], a[1], b[0], b[1], a[2], b[2], a[3], b[3]] + own
        ma, mb, host = g & 15, g >> 4 & 15, g >> 8
        doomed += [a[i] for i in range(4) if ma >> i & 1] + [b[i] for i in range(4) if mb >> i & 1] + (own if host else [])
        combos.append((ma, mb, host))
        roles.append([b[0], b[1], a[0], a[1], a[2], b[2], a[3], b[3]])
        owns += own
    # the way back: one key a group a call, b's home slots first (a's chain may not settle there), the hosts' own keys last
    back = [[r[i] for r in roles if r[i] in set(doomed)] for i in range(8)] + [[k for k in owns if k in set(doomed)]]
    return Case(f"I-{part}", "I", I_TABLE, insert, overflow=True, keys=doomed, doomed=set(doomed), combos=combos,
                homes=[GROUP * j for j in range(GROUPS)], back=[b for b in back if b])


W_TABLE = dict(numBuckets=8, bucketSize=2, numVoxelBlocks=16, attachedLinkedListSize=6)
W_SHARD = dict(numBuckets=16, bucketSize=2, numVoxelBlocks=16, attachedLinkedListSize=6)
W_RANGE = (5, 13)


def w_case(mask, shard):
    """C's chain on the last bucket: of the table (8 buckets), or of a shard that owns buckets 5 .. 12 of 16 -- there the list
    also names two keys of the other shard, one of them a key the other shard could hold in `bucket 12 + 1`."""
    table, rng = (W_SHARD, W_RANGE) if shard else (W_TABLE, None)
    home = rng[1] - 1 if shard else 7
    keys = bucket_keys(table["numBuckets"], {home: 7})[home]
    doomed = [keys[i] for i in range(7) if mask >> i & 1]
    foreign = [mm.key_for_bucket(50, 51, 13, 16), mm.key_for_bucket(50, 52, 2, 16)] if shard else []
    return Case(f"W-{'shard' if shard else 'table'}-{mask}", "W", table, keys, overflow=True, bucket_range=rng,
                keys=foreign[:1] + doomed + foreign[1:], doomed=set(doomed), home=home, foreign=foreign)


def permutations_of(c, count=24, seed=0):
    """`count` orders of the case's key list: as given, reversed, and seeded shuffles."""
    rng = np.random.RandomState(seed)
    out = [list(c.keys), list(c.keys)[::-1]]
    while len(out) < count:
        out.append([c.keys[i] for i in rng.permutation(len(c.keys))])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family V
# ---------------------------------------------------------------------------------------------------------------------------------
V_TABLE = dict(numBuckets=256, bucketSize=8, numVoxelBlocks=2048)
V_BIG_TABLE = dict(numBuckets=512, bucketSize=8, numVoxelBlocks=4096)
THRESHOLDS = {"T": float(T), "zero": 0.0, "minus-one": -1.0, "inf": INF, "nan": NAN}
SUB = F(1e-45)                                          # the smallest subnormal


def far_block():
    return np.full(512, FAR), np.ones(512, F)


def one_voxel(i, sdf, weight=1.0):
    """Every voxel observed and far, voxel i alone holds (sdf, weight)."""
    s, w = far_block()
    s[i], w[i] = sdf, weight
    return s, w


def v_blocks(big=False):
    """[(tag, sdf[512], weight[512])]: the crafted blocks of family V in the order they are dealt to the keys."""
    out = []
    for i in range(512):                               # decided by voxel i alone: kept, and its twin without it: deleted
        out.append((f"near-{i}", *one_voxel(i, dn(T) if i & 1 else -dn(T))))
        out.append((f"far-{i}", *one_voxel(i, F(0.5) + F(i) * F(0.001))))
    for name, v in (("at", T), ("above", up(T)), ("below", dn(T))):
        for sign in (+1, -1):
            out.append((f"boundary-{name}{'+' if sign > 0 else '-'}", *one_voxel(77 + 128 * (sign > 0), F(sign) * v)))
    assert np.array_equal(mm.WEIGHTS, np.array([0.0, -1.0, 1e-45, INF, NAN, 1.0], F), equal_nan=True)
    for j, name in enumerate(("zero", "minus-one", "subnormal", "inf", "nan", "one")):     # the deciding voxel is near; does its weight count?
        out.append((f"weight-{name}", *one_voxel(300 + j, dn(T), mm.WEIGHTS[j])))
    for name, ws in (("zero", (0.0,)), ("minus-one", (-1.0,)), ("nan", (NAN,)), ("zero-and-minus-one", (0.0, -1.0))):
        w = np.array([ws[i % len(ws)] for i in range(512)], F)
        out.append((f"weights-all-{name}", np.full(512, F(0.01)), w))
    for name, v in (("+0", 0.0), ("-0", -0.0), ("+sub", SUB), ("-sub", -SUB), ("+inf", INF), ("-inf", -INF), ("nan", NAN)):
        out.append((f"sdf-{name}", *one_voxel(450, v)))
    out.append(("sdf-all-nan", np.full(512, F(NAN)), np.ones(512, F)))
    out.append(("sdf-all-inf", np.full(512, F(INF)), np.ones(512, F)))
    if big:                                            # filler, then decisions in the last 300 of the list
        head, tail = out[:-300], out[-300:]
        filler = [(f"filler-{i}", *one_voxel(i % 512, F(0.02) if i % 3 else FAR)) for i in range(2100 - len(out))]
        out = head + filler + tail
    return out


def frustum_keys(oracle, c, count):
    """`count` block keys the frustum test of the case's pose accepts, nearest first."""
    ot = oracle.OracleTable(c.params(oracle), c.W, c.H, c.sem)
    ot.set_projection(c.proj())
    ot.set_pose(c.pose)
    cand = sorted(itertools.product(range(-12, 12), range(-10, 10), range(2, 22)), key=lambda k: (k[2], abs(k[0]) + abs(k[1])))
    room = np.full(c.table["numBuckets"], c.table["bucketSize"])           # (a cuboid of keys crowds the hash: skip full buckets)
    keys = []
    for k, b in zip(cand, mm.hash_block(cand, c.table["numBuckets"]).tolist()):
        if len(keys) < count and room[b] and ot.block_in_frustum(k):
            room[b] -= 1
            keys.append(k)
    ot.close()
    assert len(keys) == count, f"{len(keys)} of {count} keys in the frustum"
    return keys


def v_case(oracle, threshold="T", big=False):
    """The blocks of v_blocks dealt to keys inside the frustum in TABLE order (the compact list's order), so that the blocks kept
    and deleted by voxel i follow each other in the list."""
    blocks = v_blocks(big)
    table = V_BIG_TABLE if big else V_TABLE
    c = Case(f"V-{'big-' if big else ''}{threshold}", "V", table, [], threshold=THRESHOLDS[threshold])
    keys = frustum_keys(oracle, c, len(blocks))
    bucket = mm.hash_block(keys, table["numBuckets"])
    assert np.bincount(bucket).max() <= table["bucketSize"], "the crafted keys crowd a bucket"
    order = np.argsort(bucket, kind="stable")          # insertion in order fills a bucket's slots in order: table order
    c.insert = [keys[i] for i in order]
    by_key = {k: blocks[n] for n, k in enumerate(c.insert)}
    c.fill = lambda key, i: by_key[key][1:]
    c.facts.update(blocks=by_key, doomed={k for k, (_, s, w) in by_key.items() if collect_rule(s, w, c.threshold)})
    return c


def deciding_voxels(c):
    """{tag: (key, voxel)} of the blocks of a V case whose decision (at threshold T) hangs on one voxel: flipping that voxel to
    far, or to near, flips collect_rule."""
    out = {}
    for k, (tag, s, w) in c.facts["blocks"].items():
        if not tag.startswith(("near-", "far-")):
            continue
        i = int(tag.split("-")[1])
        s2 = s.copy()
        s2[i] = FAR if tag.startswith("near") else dn(T)
        if collect_rule(s, w, T) != collect_rule(s2, w, T):
            out[tag] = (k, i)
    return out
