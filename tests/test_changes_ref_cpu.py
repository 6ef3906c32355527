"""tests/changes_ref.py, the rule of vh_changes in numpy, checked on its own: the digest's known answers and its guarantee, the
halo sets against what a block's mesh reads, region growth at the ends of int32, and removed / re-keyed / re-slotted blocks on
hand-written tables.  No GPU."""
import itertools

import numpy as np
import pytest

import changes_ref as R

ENTRY = np.dtype([("pos", "<i4", (3,)), ("ptr", "<i4"), ("offset", "<i4")])
VOXEL = np.dtype([("sdf", "<f4"), ("weight", "<f4")])
EDGE = (1 << 28) - 1


def fixed_block():
    """sdf bits 3 i + 1, weight bits 0x3f800000 + i, colour words 7 i + 5."""
    i = np.arange(512, dtype=np.uint32)
    return 3 * i + 1, np.uint32(0x3F800000) + i, 7 * i + 5


def plain_digest(sdf, weight, colors, what):
    """The header's formulas with Python ints, term by term."""
    h0 = h1 = 0
    for i in range(512):
        m = R.mix_int(((int(weight[i]) << 32) | int(sdf[i])) + (i + 1) * R.G + what)
        h0, h1 = (h0 + m) & R.MASK, (h1 + m * (2 * i + 1)) & R.MASK
    if what & R.COLOR:
        for i in range(512):
            c = 0 if colors is None else int(colors[i])
            m = R.mix_int(c + (i + 513) * R.G + what)
            h0, h1 = (h0 + m) & R.MASK, (h1 + m * (2 * (i + 512) + 1)) & R.MASK
    return h0, h1


def test_mix_known_answers():
    # splitmix64's finaliser: the first outputs of the generator seeded with 0 are mix(G), mix(2 G) (Vigna's reference values)
    assert R.mix_int(R.G) == 0xE220A8397B1DCDAF
    assert R.mix_int(2 * R.G) == 0x6E789E6AA1B965F4
    assert [int(v) for v in R.mix(np.array([R.G, (2 * R.G) & R.MASK], np.uint64))] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    assert R.mix_int(0) == 0


@pytest.mark.parametrize("what", [R.VOXELS, R.VOXELS | R.COLOR])
def test_digest_is_the_formula_and_a_sum(what):
    sdf, weight, colors = fixed_block()
    want = plain_digest(sdf, weight, colors, what)
    assert R.digest(sdf, weight, colors, what) == want
    n = 1024 if what & R.COLOR else 512
    rng = np.random.RandomState(1)
    for _ in range(3):
        assert R.digest(sdf, weight, colors, what, order=rng.permutation(n)) == want
    assert R.digest(sdf, weight, colors, what, order=np.arange(n)[::-1]) == want
    # no colour volume: every word 0
    assert R.digest(sdf, weight, None, what) == plain_digest(sdf, weight, None, what)


def test_what_separates_the_digests():
    sdf, weight, colors = fixed_block()
    a, b = R.digest(sdf, weight, colors, R.VOXELS), R.digest(sdf, weight, colors, R.VOXELS | R.COLOR)
    assert a != b
    # and not just by the colour terms: the voxel terms alone differ
    m1, _ = R.terms(sdf, weight, colors, R.VOXELS)
    m3, _ = R.terms(sdf, weight, colors, R.VOXELS | R.COLOR)
    assert (m1 != m3[:512]).all()


@pytest.mark.parametrize("voxel", [0, 255, 511])
def test_every_single_bit_flip_is_detected(voxel):
    sdf, weight, colors = fixed_block()
    what = R.VOXELS | R.COLOR
    base = R.digest(sdf, weight, colors, what)
    seen = {base}
    for field in range(3):
        for bit in range(32):
            parts = [sdf.copy(), weight.copy(), colors.copy()]
            parts[field][voxel] ^= np.uint32(1 << bit)
            d = R.digest(parts[0], parts[1], parts[2], what)
            assert d[0] != base[0] and d != base, (field, bit)      # mix is a bijection: h0 moves by m' - m != 0
            seen.add(d)
    assert len(seen) == 97
    # a colour flip is invisible to a digest of the voxels alone, as specified
    flipped = colors.copy()
    flipped[voxel] ^= np.uint32(1)
    assert R.digest(sdf, weight, flipped, R.VOXELS) == R.digest(sdf, weight, colors, R.VOXELS)


def test_signed_zero_and_nan_payloads_are_changes():
    sdf, weight, _ = fixed_block()
    a, b = sdf.copy(), sdf.copy()
    a[7], b[7] = np.float32(0.0).view(np.uint32), np.float32(-0.0).view(np.uint32)
    assert R.digest(a, weight) != R.digest(b, weight)
    a[7], b[7] = 0x7FC00000, 0x7FC00001
    assert R.digest(a, weight) != R.digest(b, weight)


@pytest.mark.parametrize("halo", [R.HALO_NONE, R.HALO_MESH, R.HALO_NORMALS])
def test_halo_offsets_are_what_the_mesh_reads(halo):
    assert sorted(R.halo_offsets(halo)) == sorted(R.halo_offsets_brute(halo))
    assert len(R.halo_offsets(halo)) == {R.HALO_NONE: 0, R.HALO_MESH: 7, R.HALO_NORMALS: 26}[halo]


def table_of(keys_ptrs, size=None):
    t = np.zeros(size or len(keys_ptrs), ENTRY)
    t["ptr"] = -1
    for i, (k, ptr) in enumerate(keys_ptrs):
        if k is not None:
            t[i] = (k, ptr, 0)
    return t


def noise(pool, seed=0):
    rng = np.random.RandomState(seed)
    v = np.zeros(pool * 512, VOXEL)
    v["sdf"], v["weight"] = rng.standard_normal(pool * 512), rng.randint(1, 9, pool * 512)
    return v


@pytest.mark.parametrize("centre", [(0, 0, 0), (-5, 7, -1), (EDGE - 1, -EDGE + 1, EDGE - 1), (-EDGE + 1, -EDGE + 1, -EDGE + 1)])
@pytest.mark.parametrize("halo", [R.HALO_MESH, R.HALO_NORMALS])
def test_halo_sets_against_brute_force(centre, halo):
    """A 3x3x3 cluster with holes around a centre (negative keys, keys at +-(2^28 - 1)); one block changes."""
    rng = np.random.RandomState(abs(hash(centre)) % 1000)
    keys = [tuple(c + o for c, o in zip(centre, d)) for d in itertools.product((-1, 0, 1), repeat=3)
            if d == (0, 0, 0) or rng.uniform() < 0.6]
    assert all(abs(c) <= EDGE for k in keys for c in k)
    table = table_of([(k, 512 * i) for i, k in enumerate(keys)])
    vox = noise(len(keys))
    st = R.State(len(keys))
    ch, rm, ok = R.changes(table, vox, None, st, halo=halo)
    assert ok and len(ch) == len(keys) and (ch[:, 3] & R.SELF).all() and len(rm) == 0
    vox["sdf"][512 * keys.index(centre) + 255] += 1.0
    ch, rm, ok = R.changes(table, vox, None, st, halo=halo)
    got = {tuple(r[:3]): int(r[3]) for r in ch.tolist()}
    reads = (0, 1) if halo == R.HALO_MESH else (-1, 0, 1)
    want = {centre: R.SELF}
    for j in keys:                                  # brute force: block j is halo iff one of the blocks its mesh reads is the centre
        if j != centre and any(tuple(a + b for a, b in zip(j, d)) == centre for d in itertools.product(reads, repeat=3)):
            want[j] = R.HALO
    assert got == want and len(want) > 1
    assert [tuple(r[:3]) for r in ch.tolist()] == [k for k in keys if k in want]      # entry order


def test_region_growth_saturates():
    assert R.grow(None) == ((R.INT32_MIN,) * 3, (R.INT32_MAX,) * 3)
    assert R.grow(((R.INT32_MIN, -3, 0), (4, R.INT32_MAX, 1))) == ((R.INT32_MIN, -4, -1), (5, R.INT32_MAX, 2))
    assert R.grow(((R.INT32_MIN + 1, 0, 0), (R.INT32_MAX - 1, 1, 1))) == ((R.INT32_MIN, -1, -1), (R.INT32_MAX, 2, 2))
    # a region up to the end of int32 lists its blocks and their halo, and nothing wraps round
    keys = [(EDGE, 0, 0), (EDGE - 1, 0, 0), (-EDGE, 0, 0)]
    table = table_of([(k, 512 * i) for i, k in enumerate(keys)])
    st = R.State(3)
    ch, _, _ = R.changes(table, noise(3), None, st, region=((EDGE, R.INT32_MIN, R.INT32_MIN), (R.INT32_MAX,) * 3))
    assert {tuple(r[:3]): r[3] for r in ch.tolist()} == {(EDGE, 0, 0): R.SELF, (EDGE - 1, 0, 0): R.HALO}


def test_removed_rekeyed_and_reslotted():
    K1, K2, K3, FAR = (0, 0, 0), (9, 9, 9), (1, 0, 0), (40, 0, 0)
    vox = noise(4, seed=3)
    before = table_of([(K1, 0), (K3, 512), (FAR, 1024), (None, -1)])
    st = R.State(4)
    ch, rm, _ = R.changes(before, vox, None, st, halo=R.HALO_NONE)
    assert len(ch) == 3 and len(rm) == 0 and st.epoch == 1 and st.slots["live"].tolist() == [1, 1, 1, 0]

    # removed: K1 leaves, nothing takes its slot.  K3 = K1 + (1, 0, 0) is no MESH halo of K1 (it does not read K1) ...
    s = st.copy()
    ch, rm, _ = R.changes(table_of([(None, -1), (K3, 512), (FAR, 1024), (None, -1)]), vox, None, s, halo=R.HALO_MESH)
    assert rm.tolist() == [[0, 0, 0, 0]] and len(ch) == 0 and not s.slots[0]["live"]
    # ... but it is a NORMALS halo
    s = st.copy()
    ch, rm, _ = R.changes(table_of([(None, -1), (K3, 512), (FAR, 1024), (None, -1)]), vox, None, s, halo=R.HALO_NORMALS)
    assert rm.tolist() == [[0, 0, 0, 0]] and ch.tolist() == [[1, 0, 0, R.HALO]]

    # re-keyed: K2 takes K1's pool slot with K1's very bits -- K1 removed, K2 self-changed, one slot
    s = st.copy()
    ch, rm, _ = R.changes(table_of([(K2, 0), (K3, 512), (FAR, 1024), (None, -1)]), vox, None, s, halo=R.HALO_NONE)
    assert rm.tolist() == [[0, 0, 0, 0]] and ch.tolist() == [[9, 9, 9, R.SELF]]
    assert s.slots[0]["live"] and s.slots[0]["key"].tolist() == [9, 9, 9]
    assert R.block_digest(vox, None, 0, R.VOXELS) == (int(s.slots[0]["h0"]), int(s.slots[0]["h1"]))

    # re-slotted: K1 comes back under another pool slot with the same bits -- not removed, self-changed at the new slot
    moved = vox.copy()
    moved[1536:2048] = vox[0:512]
    s = st.copy()
    ch, rm, _ = R.changes(table_of([(None, -1), (K3, 512), (FAR, 1024), (K1, 1536)]), moved, None, s, halo=R.HALO_NONE)
    assert len(rm) == 0 and ch.tolist() == [[0, 0, 0, R.SELF]]
    assert not s.slots[0]["live"] and s.slots[3]["live"] and s.slots[3]["key"].tolist() == [0, 0, 0]
    assert (s.slots[3]["h0"], s.slots[3]["h1"]) == (st.slots[0]["h0"], st.slots[0]["h1"])      # the digest does not hold the slot

    # a capacity one short: counts, no commit
    s = st.copy()
    ch, rm, ok = R.changes(table_of([(K2, 0), (K3, 512), (FAR, 1024), (None, -1)]), vox, None, s, halo=R.HALO_NONE,
                           capacity_changed=1, capacity_removed=0)
    assert not ok and len(ch) == 1 and len(rm) == 1 and s.tobytes() == st.tobytes()
    assert R.State.frombytes(st.tobytes()).tobytes() == st.tobytes()

    # a region: what lies outside is neither reported nor consumed
    s = st.copy()
    changed = vox.copy()
    changed["sdf"][1024] += 1.0
    changed["sdf"][0] += 1.0
    ch, rm, _ = R.changes(before, changed, None, s, region=((-1, -1, -1), (2, 2, 2)), halo=R.HALO_NONE)
    assert ch.tolist() == [[0, 0, 0, R.SELF]]
    ch, rm, _ = R.changes(before, changed, None, s, halo=R.HALO_NONE)
    assert ch.tolist() == [[40, 0, 0, R.SELF]]


@pytest.mark.parametrize("halo", [R.HALO_MESH, R.HALO_NORMALS])
def test_the_mesh_cache_sequences_have_partial_updates(oracle, halo):
    """The seeds of tests/test_gpu_mesh_cache.py, on the shadow model alone: after some model-changing step the rule lists fewer
    blocks than the model holds (a cache that re-meshed everything would otherwise pass there), and blocks are removed."""
    import lifecycle_cases as LC
    import mesh_cache_cases as MC
    for seed in MC.SEEDS:
        seq = LC.Sequence(oracle, MC.VARIANT, MC.SEM, seed)
        sh = seq.shadow
        state = R.State(sh.params.numVoxelBlocks)
        partial, removed, ops = [], 0, []
        for n, step in MC.changing_steps(seq):
            if not MC.changes_model(step):
                continue
            ch, rm, ok = R.changes(sh.table(), sh.ot.sdf_blocks(), None, state, halo=halo)
            live = len(sh.live())
            assert ok and len(ch) <= live
            ops.append(step["op"])
            removed += len(rm)
            if len(ch) < live:
                partial.append((n, step["op"], len(ch), live))
        print(f"seed {seed}: steps={ops} partial={partial} removed={removed}")
        assert len(partial) >= 3 and removed > 0 and len(set(ops)) >= 6
        seq.close()
