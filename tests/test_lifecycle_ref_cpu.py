"""The plans of tests/lifecycle_cases.py replayed on the shadow alone (tests/lifecycle_ref.py): the conditions on the INPUTS that keep
tests/test_gpu_lifecycle.py from being vacuous -- the roomy variant never meets a full bucket, the crowded one has chains and
takes entries out of them, every step kind and every adjacent pair the GPU test is about occurs, no step is empty, a freed block
is handed out again under colour -- and the two pieces the shadow adds to the repository's rules: the oracle's insertion call and
the checker of a downloaded table's structure."""
import numpy as np
import pytest

import lifecycle_cases as LC
import lifecycle_ref as LR
import merge_color_cases as CC
import stream_ref as S

CASES = [(v, sem) for v in ("A", "B") for sem in (0, 1)]

_RUNS = {}


def replay(oracle, variant, sem, seed):
    """One sequence on the shadow: the steps (with what the shadow expects of them) and what was seen of the table on the way."""
    key = (variant, sem, seed)
    if key not in _RUNS:
        seq = LC.Sequence(oracle, variant, sem, seed)
        sh = seq.shadow
        bs = sh.params.bucketSize
        seen = dict(full=False, min_heap=sh.ot.heap_counter(), chains=False, steps=[])

        def look():
            tab = sh.table()
            seen["full"] |= bool((tab["ptr"].reshape(-1, bs) != -1).all(1).any())
            seen["min_heap"] = min(seen["min_heap"], sh.ot.heap_counter())
            seen["chains"] |= bool((tab["offset"] != 0).any())

        look()
        for step in seq.steps():
            look()
            LR.table_invariants(LR.oracle_snapshot(sh), sh.params, sh.overflow)
            seen["steps"].append({k: v for k, v in step.items() if k in ("op", "expect", "pending", "fused", "piped", "in_flight", "chunk")})
        seen.update(log=list(seq.log), dropped=list(seq.dropped), refused=sh.refused, reuse=sh.reuse_coloured, live=len(sh.live()))
        seq.close()
        _RUNS[key] = seen
    return _RUNS[key]


@pytest.mark.parametrize("seed", LC.SEEDS)
@pytest.mark.parametrize("variant,sem", CASES)
def test_no_step_is_empty(oracle, variant, sem, seed):
    run = replay(oracle, variant, sem, seed)
    print(f"{variant} sem {sem} seed {seed}: {len(run['log'])} steps, {run['live']} blocks at the end; {run['log']}")
    print("steps the plan could not place:", run["dropped"])
    assert len(run["dropped"]) <= 2                                       # (what must occur is asserted by kind and by pair below)
    assert 30 <= len(run["log"]) <= 50
    if variant == "A":
        assert not run["full"] and run["min_heap"] >= 16
    else:
        assert run["min_heap"] >= 0 and run["refused"] == 0
    for i, step in enumerate(run["steps"]):
        op, ex = step["op"], step["expect"]
        where = (i, op, run["log"][:i + 1])
        if op in ("delete_blocks", "stream_out") or (op == "garbage_collect" and ex["listed"] > 0):
            assert ex["freed"] >= 1 and ex["live"] >= 8, where
        if op == "garbage_collect" and ex["listed"] == 0:                 # directly after a stream-in: the list is empty by the rule
            assert ex["freed"] == 0 and run["log"][i - 1] == "stream_in", where
        if op == "stream_in":
            assert ex["placed"] >= 1, where
        if op in LC.DEINT + ["reintegrate_depth", "deintegrate_depth_color", "reintegrate_depth_color"]:
            assert ex["voxels"] >= 100, where
        if op in ("merge", "merge_color"):
            assert ex["stats"]["allocated"] >= 1 and ex["stats"]["updated"] >= 1, where
        if op in LC.COLOUR + ["integrate_depth_color", "deintegrate_depth_color", "reintegrate_depth_color"]:
            assert ex["words"] >= 100, where


@pytest.mark.parametrize("variant,sem", CASES)
def test_every_kind_and_every_pair_occurs(oracle, variant, sem):
    runs = [replay(oracle, variant, sem, seed) for seed in LC.SEEDS]
    ops = [s["op"] for r in runs for s in r["steps"]]
    for kind in LC.KINDS:
        assert ops.count(kind) >= 3, (kind, ops.count(kind))

    def adjacent(*names):
        """Some run has steps of these kinds next to each other; a name ending in "!" is a plain frame left pending, "fused" a
        frame in the fused form."""
        def fits(step, name):
            if name == "frame!":
                return step["op"] in ("integrate_depth", "integrate") and step.get("in_flight")
            if name == "fused":
                return step["op"] in LC.FRAMES and step.get("fused")
            if name == "deintegrate":
                return step["op"] in LC.DEINT
            if name == "colour frame":
                return step["op"] in ("integrate_color", "integrate_color_map", "integrate_depth_color")
            return step["op"] == name
        return any(all(fits(r["steps"][i + j], n) for j, n in enumerate(names))
                   for r in runs for i in range(len(r["steps"]) - len(names) + 1))

    pairs = [("stream_in", "garbage_collect"), ("stream_in", "stream_in"), ("merge", "stream_out"),
             ("stream_out", "extract_mesh", "stream_out"), ("garbage_collect", "stream_in"), ("deintegrate", "garbage_collect"),
             ("reload", "colour frame")] + [("frame!", x) for x in LC.PENDING_BEFORE]
    if variant == "A":
        pairs += [("stream_in", "fused"), ("merge", "fused")]
    missing = [p for p in pairs if not adjacent(*p)]
    assert not missing, missing
    # a stream-in with PRESENT records and a duplicate record; block reuse under colour; chains, and a removal out of one
    ins = [s for r in runs for s in r["steps"] if s["op"] == "stream_in"]
    assert any(s["expect"]["present"] >= 2 and len(np.unique(s["chunk"]["keys"], axis=0)) < len(s["chunk"]["keys"]) for s in ins)
    assert any(s["chunk"]["colors"] is None for s in ins) and any(s["chunk"]["colors"] is not None for s in ins)
    assert any(r["reuse"] for r in runs)
    if variant == "B":
        assert all(r["chains"] for r in runs)
        assert sum(s["expect"].get("unchained", 0) for r in runs for s in r["steps"]) >= 1


# ---- the insertion call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A", "B"])
def test_insert_blocks_against_with_new_blocks(oracle, variant):
    seq = LC.Sequence(oracle, variant, 1, 0)
    sh = seq.shadow
    steps = seq.steps()
    for _ in range(3):
        next(steps)
    before = sh.model()
    counter = sh.ot.heap_counter()
    held = sorted(before)[:5]
    far = (np.random.RandomState(5).randint(-3000, 3000, (200, 3)) + (9000, 0, 0)).astype(np.int64)
    used = (sh.table()["ptr"] != -1).reshape(-1, sh.params.bucketSize).sum(1)
    home = np.asarray(LR.MM.hash_block(far, sh.params.numBuckets))
    far = far[[i for i, h in enumerate(home.tolist()) if used[h] < sh.params.bucketSize and h not in home[:i].tolist()]]     # (a free slot each)
    new = [tuple(k) for k in far[:12].tolist()]
    assert len(new) == 12
    keys = new[:6] + held + new[6:] + new[:2]                                # absent keys, present keys, and two a second time
    assert sh.ot.insert_blocks(keys) == len(new)
    want = CC.with_new_blocks(before, keys)
    S.same_models(sh.model(), want)
    assert sh.ot.heap_counter() == counter - len(new) and sh.ot.compact_count() == 0
    LR.table_invariants(LR.oracle_snapshot(sh), sh.params, sh.overflow)
    assert sh.ot.insert_blocks(keys) == 0                                    # all present now
    assert sh.ot.delete_blocks(new) == len(new)
    S.same_models(sh.model(), before)
    seq.close()


def test_insert_blocks_chains_and_refuses(oracle):
    """One bucket filled beyond its slots: with the list the next keys go on its chain (at most attachedLinkedListSize - 1),
    without it they are refused; an empty heap refuses everything."""
    for overflow in (False, True):
        p = oracle.default_params(numBuckets=257, bucketSize=4, numVoxelBlocks=64)
        ot = oracle.OracleTable(p, 64, 48, 1)
        ot.set_overflow(overflow)
        target, keys, x = S.hash_block((3, -2, 7), 257), [], -4000
        while len(keys) < 9:
            if S.hash_block((x, -2, 7), 257) == target:
                keys.append((x, -2, 7))
            x += 1
        placed = ot.insert_blocks(keys)
        assert placed == (4 + p.attachedLinkedListSize - 1 if overflow else 4)
        tab = ot.hash_table()
        assert (tab["ptr"] != -1).sum() == placed and bool((tab["offset"] != 0).any()) == overflow
        snap = dict(table=tab.copy(), heap=ot.heap().copy(), counters=dict(heap_counter=ot.heap_counter()), compact=None)
        LR.table_invariants(snap, p, overflow)
        assert ot.delete_blocks(keys) == placed and ot.heap_counter() == 63
        ot.close()
    ot = oracle.OracleTable(oracle.default_params(numBuckets=257, bucketSize=4, numVoxelBlocks=3), 64, 48, 1)
    assert ot.insert_blocks([(i, 0, 0) for i in range(5)]) == 3 and ot.heap_counter() == -1
    ot.close()


# ---- the invariants checker --------------------------------------------------------------------------------------------------------
def broken(snap, how, params):
    tab, heap = snap["table"].copy(), snap["heap"].copy()
    c = dict(snap["counters"])
    bs = params.bucketSize
    live = np.nonzero(tab["ptr"] != -1)[0]
    if how == "duplicate key":                                   # a second entry of a held key in its own bucket, with a block of the heap
        full = [i for i in live if tab["ptr"][i - i % bs + bs - 1] == -1 and i % bs == 0 and tab["ptr"][i + 1] == -1]
        i = full[0]
        tab[i + 1] = tab[i]
        tab["ptr"][i + 1] = int(heap[c["heap_counter"]]) * 512
        c["heap_counter"] -= 1
    elif how == "hole":                                          # a bucket's only entry moved from its first slot to its second
        i = [i for i in live if i % bs == 0 and tab["ptr"][i + 1] == -1][0]
        tab[[i, i + 1]] = tab[[i + 1, i]]
    elif how == "free and referenced":
        heap[c["heap_counter"]] = tab["ptr"][live[0]] // 512
    elif how == "in neither":
        c["heap_counter"] -= 1                                   # the block on top of the heap is no longer on it
    elif how == "link to a free slot":
        heads = [i for i in np.nonzero(tab["offset"] != 0)[0] if i % bs == bs - 1]
        i = heads[0]
        at = (i + int(tab["offset"][i])) % len(tab)
        heap[c["heap_counter"] + 1] = tab["ptr"][at] // 512
        c["heap_counter"] += 1
        tab["ptr"][at], tab["pos"][at], tab["offset"][at] = -1, LR.SENTINEL, 0
    return dict(table=tab, heap=heap, counters=c, compact=None)


@pytest.mark.parametrize("how,variant,says", [("duplicate key", "A", "twice"), ("hole", "A", "hole"),
                                               ("free and referenced", "A", "both free and referenced"),
                                               ("in neither", "A", "neither"), ("link to a free slot", "B", "links to a free slot")])
def test_invariants_checker_fails_on_hand_broken_tables(oracle, how, variant, says):
    seq = LC.Sequence(oracle, variant, 1, 0)
    steps = seq.steps()
    for _ in range(3):
        next(steps)
    sh = seq.shadow
    snap = LR.oracle_snapshot(sh)
    LR.table_invariants(snap, sh.params, sh.overflow)
    with pytest.raises(AssertionError, match=says):
        LR.table_invariants(broken(snap, how, sh.params), sh.params, sh.overflow)
    seq.close()
