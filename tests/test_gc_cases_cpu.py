"""Pins the crafted deletion cases (tests/gc_cases.py) without a GPU: the oracle's delete_blocks / garbage_collect over every
case passes the state check written from the definition, the chain families give one outcome whatever the order of the key list
(the property the kernels' one-lane-per-home-bucket design rests on), expected_plain equals the oracle on the plain buckets, and
every case reaches what it aims at."""
import numpy as np
import pytest

import gc_cases as GC
import mesh_models as mm

PLAIN = ["P-plain", "P-shuffled"]
CHAINS = [f"C-{p}" for p in range(2)] + ["C-bucket4"] + [f"I-{p}" for p in range(8)]
MASKS = list(range(128))


def case(name):
    if name.startswith("P"):
        return GC.p_case(name == "P-shuffled")
    if name == "C-bucket4":
        return GC.c4_case()
    return (GC.c_case if name[0] == "C" else GC.i_case)(int(name[2:]))


def run(oracle, c, keys=None):
    """(pre, post, freed) of the case's call on the oracle, optionally with another key list."""
    ot = GC.load_oracle(oracle, c)
    pre = GC.state_of(ot)
    if keys is not None:
        freed = ot.delete_blocks(keys)
    else:
        freed = GC.oracle_call(c, ot)
    post = GC.state_of(ot)
    ot.close()
    return pre, post, freed


def same_outcome(a, b):
    return np.array_equal(a["table"], b["table"]) and np.array_equal(a["vox"].view(np.uint32), b["vox"].view(np.uint32)) and \
        a["heap_counter"] == b["heap_counter"]


# ---- 1. the oracle passes the state check ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN + CHAINS)
def test_oracle_passes_the_state_check(oracle, name):
    c = case(name)
    pre, post, freed = run(oracle, c)
    assert GC.check_after(pre, post, c.facts["doomed"], c.shape) == freed == len(c.facts["doomed"])


@pytest.mark.parametrize("shard", [False, True], ids=["table", "shard"])
def test_oracle_passes_the_state_check_on_the_wrapped_chain(oracle, shard):
    for mask in MASKS:
        c = GC.w_case(mask, shard)
        pre, post, freed = run(oracle, c)
        assert GC.check_after(pre, post, c.facts["doomed"], c.shape) == freed == bin(mask).count("1")
        assert GC.key_set(pre["table"]) == set(c.insert)


@pytest.mark.parametrize("threshold", list(GC.THRESHOLDS))
def test_oracle_collects_by_the_rule(oracle, threshold):
    c = GC.v_case(oracle, threshold)
    pre, post, freed = run(oracle, c)
    assert GC.check_after(pre, post, c.facts["doomed"], c.shape) == freed
    tags = {c.facts["blocks"][k][0] for k in c.facts["doomed"]}
    none_seen = {"weights-all-zero", "weights-all-minus-one", "weights-all-nan", "weights-all-zero-and-minus-one"}
    if threshold == "nan":                             # the decision: a block without an observed voxel goes, whatever the threshold
        assert tags == none_seen
    if threshold == "inf":
        assert tags == none_seen | {"sdf-all-nan", "sdf-all-inf"}
    if threshold in ("zero", "minus-one"):
        assert len(tags) == len(c.insert)
    if threshold == "T":
        kept = {c.facts["blocks"][k][0] for k in set(c.insert) - c.facts["doomed"]}
        assert {t for t in kept if not t.startswith("near-")} == {
            "boundary-below+", "boundary-below-", "weight-subnormal", "weight-inf", "weight-one", "sdf-+0", "sdf--0", "sdf-+sub", "sdf--sub"}
        assert len([t for t in kept if t.startswith("near-")]) == 512 == len([t for t in tags if t.startswith("far-")])
        assert {"boundary-at+", "boundary-at-", "boundary-above+", "boundary-above-"} <= tags


def test_oracle_collects_the_long_list(oracle):
    c = GC.v_case(oracle, "T", big=True)
    pre, post, freed = run(oracle, c)
    assert GC.check_after(pre, post, c.facts["doomed"], c.shape) == freed
    listed = [tuple(p) for p in pre["table"]["pos"][pre["table"]["ptr"] != -1].tolist()]      # table order = list order
    assert listed == c.insert and len(listed) >= 2049
    tail = [c.facts["blocks"][k][0] for k in listed[-300:]]
    assert not any(t.startswith("filler") for t in tail)
    verdicts = {k in c.facts["doomed"] for k in listed[-300:]}
    assert verdicts == {True, False}
    decided = GC.deciding_voxels(c)
    assert sum(1 for t in tail if t in decided) > 100


@pytest.mark.parametrize("name", PLAIN + CHAINS)
def test_the_doomed_keys_can_all_come_back(oracle, name):
    """... in the calls the GPU test streams them in with; the survivors' frustum is the whole table."""
    c = case(name)
    ot = GC.load_oracle(oracle, c)
    GC.oracle_call(c, ot)
    ot.set_pose(c.pose)
    assert ot.flatten() == len(c.insert) - len(c.facts["doomed"])
    back = [k for call in c.facts["back"] for k in call]
    assert sorted(back) == sorted(c.facts["doomed"])
    assert ot.insert_blocks(back) == len(back)
    assert ot.flatten() == len(c.insert)
    ot.close()


# ---- 2. the order of the key list does not matter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
def test_chains_give_one_outcome_in_every_order(oracle, name):
    c = case(name)
    _, first, _ = run(oracle, c)
    orders = GC.permutations_of(c)
    assert len(orders) >= 24
    for keys in orders[1:]:
        assert same_outcome(first, run(oracle, c, keys)[1])


@pytest.mark.parametrize("shard", [False, True], ids=["table", "shard"])
def test_the_wrapped_chain_gives_one_outcome_in_every_order(oracle, shard):
    for mask in MASKS:
        c = GC.w_case(mask, shard)
        _, first, _ = run(oracle, c)
        for keys in GC.permutations_of(c, seed=mask)[1:]:
            assert same_outcome(first, run(oracle, c, keys)[1]), mask


# ---- 3. expected_plain ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN)
def test_expected_plain_is_the_oracle_on_plain_buckets(oracle, name):
    c = case(name)
    pre, post, _ = run(oracle, c)
    assert np.array_equal(GC.expected_plain(pre["table"], c.facts["doomed"], 5), post["table"])
    assert not np.array_equal(pre["table"], post["table"])


# ---- 4. the cases reach what they aim at -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN)
def test_plain_buckets_hold_every_pattern(oracle, name):
    c = case(name)
    pre, post, _ = run(oracle, c)
    rows = pre["table"].reshape(-1, 5)
    patterns = set()
    for b, n, m in c.facts["plan"]:
        assert (rows[b]["ptr"] != -1).tolist() == [True] * n + [False] * (5 - n)
        assert [tuple(p) for p in rows[b]["pos"][:n].tolist()] == c.facts["bucket_keys"][b]
        patterns.add((n, sum(1 << i for i in range(n) if c.facts["bucket_keys"][b][i] in c.facts["doomed"])))
    assert len(patterns) == 62 == 2 + 4 + 8 + 16 + 32
    assert (rows[62:]["ptr"] == -1).all()
    if name == "P-shuffled":
        assert len(c.keys) > len(set(c.keys)) > len(c.facts["doomed"])
        home = mm.hash_block(c.facts["absent"], 64).tolist()
        listed = {b for b, n, m in c.facts["plan"] if m}
        assert home[0] in listed and home[1] == 63 and not set(c.facts["absent"]) & GC.key_set(pre["table"])
    moved = (pre["table"]["ptr"] != post["table"]["ptr"]) & (post["table"]["ptr"] != -1)
    assert moved.sum() > 50                            # entries that moved down


@pytest.mark.parametrize("name", ["C-0", "C-1", "C-bucket4"])
def test_one_chain_is_laid_out_as_said(oracle, name):
    c = case(name)
    pre, post, _ = run(oracle, c)
    tab, bs = pre["table"], c.table["bucketSize"]
    reach = GC.chains(tab, c.shape)
    assert sorted(reach) == c.facts["homes"]
    for g, h in enumerate(c.facts["homes"]):
        last = h * bs + bs - 1
        offsets = [int(tab["offset"][i]) for i in [last] + reach[h]]
        if bs == 2:
            assert offsets == [9, 7, 5, 3, 1, 0] and reach[h] == [last + o for o in (9, 7, 5, 3, 1)]
            assert all(i % 2 == 0 for i in reach[h])                       # slot 0 of the five buckets behind
        else:
            assert offsets == [3, 2, 1, 0] and reach[h] == [last + 3, last + 2, last + 1]
    assert len(set(c.facts["masks"])) == len(c.facts["homes"])
    # heads that were deleted with followers, heads that were kept with unlinked followers, chains that went entirely
    heads = [h * bs + bs - 1 for h in c.facts["homes"]]
    refilled = sum(1 for i in heads if post["table"]["ptr"][i] != -1 and post["table"]["ptr"][i] != tab["ptr"][i])
    emptied = sum(1 for i in heads if post["table"]["ptr"][i] == -1)
    assert refilled > 10 and emptied == sum(1 for m in c.facts["masks"] if m >> (bs - 1) == (1 << (8 - bs)) - 1)


def test_one_chain_covers_all_128_subsets():
    assert sorted(m for p in range(2) for m in GC.c_case(p).facts["masks"]) == list(range(128))
    assert GC.c4_case().facts["masks"] == list(range(128))


def test_interleaved_chains_interleave(oracle):
    combos, ends = [], set()
    for part in range(8):
        c = case(f"I-{part}")
        pre, post, _ = run(oracle, c)
        tab = pre["table"]
        reach = GC.chains(tab, c.shape)
        for h in c.facts["homes"]:
            assert [i // 2 for i in reach[h]] == [h + 4, h + 2] and [i // 2 for i in reach[h + 1]] == [h + 5, h + 3]
            for host in range(h + 2, h + 6):                               # a foreign entry in slot 0, its own in the last slot
                own = tab[2 * host + 1]
                assert own["ptr"] != -1 and mm.hash_block([own["pos"].tolist()], 384)[0] == host and tab["ptr"][2 * host] != -1
                after = post["table"][2 * host:2 * host + 2]
                foreign, mine = after["ptr"][0] != -1, after["ptr"][1] != -1
                ends.add((bool(foreign), bool(mine)))
        combos += c.facts["combos"]
    assert len(set(combos)) == 512 == 16 * 16 * 2
    assert ends == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("shard", [False, True], ids=["table", "shard"])
def test_the_wrapped_chain_wraps(oracle, shard):
    c = GC.w_case(127, shard)
    pre, post, _ = run(oracle, c)
    tab = pre["table"]
    reach = GC.chains(tab, c.shape)
    home = c.facts["home"] - c.shape["lo"]
    assert list(reach) == [home] and home == len(tab) // 2 - 1
    assert sorted(reach[home]) == [0, 2, 4, 6, 8]                          # slot 0 of the first five buckets
    assert (post["table"]["ptr"] == -1).all()
    if shard:
        assert all(not c.shape["lo"] <= b < c.shape["hi"] for b in mm.hash_block(c.facts["foreign"], 16))
        assert c.shape["lo"] > 0


def test_deciding_voxels_lie_everywhere(oracle):
    c = GC.v_case(oracle, "T")
    d = GC.deciding_voxels(c)
    near = sorted(v for t, (_, v) in d.items() if t.startswith("near"))
    far = sorted(v for t, (_, v) in d.items() if t.startswith("far"))
    assert near == far == list(range(512))                                 # every quarter of 128 voxels, both voxels of a lane's pair
    assert {v // 128 for v in near} == {0, 1, 2, 3} and {v & 1 for v in near} == {0, 1}
    order = [c.facts["blocks"][k][0] for k in c.insert]
    assert order[:4] == ["near-0", "far-0", "near-1", "far-1"]             # kept and deleted follow each other in the list
    assert len(c.insert) == 2 * 512 + 6 + 6 + 4 + 7 + 2


@pytest.mark.parametrize("big", [False, True], ids=["V", "V-big"])
def test_the_pose_lists_every_block_and_changes_none(oracle, big):
    c = GC.v_case(oracle, "T", big)
    ot = GC.load_oracle(oracle, c)
    pre = GC.state_of(ot)
    ot.set_pose(c.pose)
    assert ot.flatten() == len(c.insert)
    assert set(map(tuple, ot.compact()["pos"].tolist())) == set(c.insert)
    ot.integrate(c.pose, np.zeros((c.H, c.W, 4), np.float32))               # an all-invalid vertex map
    assert ot.last_stats["pixels_valid"] == 0 and ot.compact_count() == len(c.insert)
    assert set(map(tuple, ot.compact()["pos"].tolist())) == set(c.insert)
    post = GC.state_of(ot)
    assert np.array_equal(pre["table"], post["table"])
    a, b = pre["vox"].view(np.uint32), post["vox"].view(np.uint32)
    assert np.array_equal(a, b)
    ot.close()
