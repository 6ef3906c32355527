"""The rule of vh_components in executable form (tests/components_ref.py) pinned without a GPU: by hand on the offsets, by the
textbook union-find on small models, by scipy.ndimage.label on dense copies where scipy is installed, and on its removal."""
import numpy as np
import pytest

import components_cases as cc
import components_ref as cr
import mesh_models as mm

BOTH = [(t, c) for t in (cr.INSIDE, cr.OUTSIDE) for c in (6, 14)]
MODELS = {
    "serpentine": cc.serpentine,
    "sparse30": lambda: cc.sparse(0.30),
    "sparse16": lambda: cc.sparse(0.16),
    "holes": lambda: mm.holes(0),
    "zeros": mm.zeros,
    "non_finite": mm.non_finite,
    "weights": mm.weights,
    "every_configuration": mm.every_configuration,
}


def component_of(lab, g):
    return lab.index[lab.rank[tuple(c >> 3 for c in g)]][cc.index(*g)]


@pytest.mark.parametrize("outside", (False, True))
def test_offsets_by_hand(outside):
    model, pairs = cc.offsets(outside)
    target = cr.OUTSIDE if outside else cr.INSIDE
    assert len(pairs) == 62 and sum(bool(p["cross"]) for p in pairs) == 49
    corner = [p for p in pairs if p["o"] == (1, 1, 1) and len(p["cross"]) == 3]
    assert len(corner) == 1 and sum(1 for k in model if all(abs(a - b) <= 1 for a, b in zip(k, (c >> 3 for c in corner[0]["A"])))) == 2
    for conn in (6, 14):
        lab = cr.label(model, None, target, conn)
        joined = 0
        for p in pairs:
            a, b = component_of(lab, p["A"]), component_of(lab, p["B"])
            assert a != cr.NONE and b != cr.NONE
            assert (a == b) == p[f"joined{conn}"], (p, conn)
            joined += int(a == b)
        assert joined == {6: 6, 14: 26}[conn]                        # axis pairs under both, the other four offsets under 14 only
        assert lab.stats["nodes"] == 124 and lab.stats["components"] == 124 - joined and lab.stats["largest"] == 2
        assert not any(p["joined14"] for p in pairs if p["o"] in cc.ANTI)
        # the sea is one piece per block pair: the other target sees no pair at all
        other = cr.label(model, None, 1 - target, conn)
        assert other.stats["nodes"] == len(model) * 512 - 124


def test_identity_and_order():
    """id = rank * 512 + voxel index: the first block of the order holds the first root, and a reversed order reverses it."""
    model = {(0, 0, 0): (np.full(512, -1.0, np.float32), np.ones(512, np.float32)),
             (5, 0, 0): (np.full(512, -1.0, np.float32), np.ones(512, np.float32))}
    model[(0, 0, 0)][1][:7] = 0                                      # voxels 0..6 are not valid: the root is voxel 7
    a = cr.label(model, [(0, 0, 0), (5, 0, 0)])
    b = cr.label(model, [(5, 0, 0), (0, 0, 0)])
    assert a.records["voxel"].tolist() == [[7, 0, 0], [40, 0, 0]] and a.records["size"].tolist() == [505, 512]
    assert b.records["voxel"].tolist() == [[40, 0, 0], [7, 0, 0]] and b.records["size"].tolist() == [512, 505]
    assert a.labels((6, 0, 0), (3, 1, 1)).tolist() == [[[cr.NONE, 0, cr.NONE]]]
    assert cr.label(model, None, region=((1, 0, 0), (9, 1, 1))).records["voxel"].tolist() == [[40, 0, 0]]
    with pytest.raises(ValueError):
        cr.label(model, None, connectivity=26)
    with pytest.raises(ValueError):
        cr.label(model, None, target=2)


def test_figures_of_the_crafted_models():
    s = cc.serpentine()
    for conn in (6, 14):
        lab = cr.label(s, None, cr.INSIDE, conn)
        assert lab.stats["components"] == 1 and lab.stats["nodes"] == 609 and lab.blocks_of().tolist() == [36]
    sea = cr.label(s, None, cr.OUTSIDE, 6)
    assert sea.stats["components"] == 1 and sea.stats["nodes"] == 17823
    swapped = cr.label(cc.serpentine(True), None, cr.OUTSIDE, 6)
    assert swapped.stats["components"] == 1 and swapped.stats["nodes"] == 609
    for p, conn in ((0.30, 6), (0.16, 14)):
        lab = cr.label(cc.sparse(p), None, cr.INSIDE, conn)
        print(p, conn, lab.stats, int((lab.blocks_of() > 1).sum()))
        assert lab.stats["components"] >= 400 and (lab.blocks_of() > 1).sum() >= 50
        assert lab.stats["largest"] <= 0.2 * lab.stats["nodes"]
    e = mm.every_configuration()
    assert cr.label(e, None, cr.INSIDE, 6).stats["components"] >= 205
    lab = cr.label(e, None, cr.INSIDE, 14)
    assert lab.stats["components"] >= 2 and lab.blocks_of().max() == 27


@pytest.mark.parametrize("name", list(MODELS))
def test_against_the_textbook_union_find(name):
    model = MODELS[name]()
    order = list(model)[::-1]
    for t, c in BOTH:
        lab = cr.label(model, order, t, c)
        assert np.array_equal(lab.records, cr.label_plain(model, order, t, c)), (t, c)
        assert lab.stats["nodes"] == lab.records["size"].sum() and lab.stats["components"] == len(lab.records)


@pytest.mark.parametrize("name", list(MODELS))
def test_against_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    model = MODELS[name]()
    d = mm.Dense(model)
    six = ndimage.generate_binary_structure(3, 1)
    fourteen = np.zeros((3, 3, 3), bool)
    fourteen[1, 1, 1] = True
    for o in cc.OFFSETS:                                             # [z, y, x]: +-o for o in {0,1}^3 minus 0
        fourteen[1 + o[2], 1 + o[1], 1 + o[0]] = fourteen[1 - o[2], 1 - o[1], 1 - o[0]] = True
    assert fourteen.sum() == 15
    for t, c in BOTH:
        mask = d.valid & (d.inside if t == cr.INSIDE else ~d.inside)
        labels, n = ndimage.label(mask, six if c == 6 else fourteen)
        lab = cr.label(model, None, t, c)
        assert n == lab.stats["components"]
        assert sorted(np.bincount(labels[mask])[1:].tolist()) == sorted(lab.records["size"].tolist())
        g, first = lab.canonical()                                   # the same partition, node by node
        theirs = labels[tuple((g - d.origin + 1).T[::-1])]
        assert (theirs > 0).all()
        _, a = np.unique(theirs, return_inverse=True)
        _, b = np.unique(first, return_inverse=True)
        pairs = np.unique(np.stack([a, b], 1), axis=0)
        assert len(pairs) == n


@pytest.mark.parametrize("min_size", (0, 1, 2, 8, 10**9))
def test_removal(min_size):
    model = cc.sparse(0.30)
    lone = np.zeros(512, np.float32), np.zeros(512, np.float32)
    lone[0][77], lone[1][77] = -1.0, 1.0
    model[(9, 9, 9)] = lone                                          # a block that holds only a floater
    model[(12, 9, 9)] = (np.zeros(512, np.float32), np.zeros(512, np.float32))     # a block that is empty already
    for t, c in BOTH:
        before = cr.label(model, None, t, c)
        out, stats, cleared, freed = cr.remove(model, min_size, None, t, c)
        small = before.records["size"] < min_size
        assert stats["removed_components"] == small.sum() and stats["removed_voxels"] == before.records["size"][small].sum()
        assert (12, 9, 9) in out
        if min_size <= 1:
            assert not cleared and not freed and stats["removed_voxels"] == 0
        if t == cr.INSIDE:
            assert ((9, 9, 9) in freed) == (min_size >= 2) and ((9, 9, 9) in out) == (min_size < 2)
        after = cr.label(out, [k for k in model if k in out], t, c)
        assert after.stats["components"] == stats["components"] - stats["removed_components"]
        assert len(after.records) == 0 or after.records["size"].min() >= min_size      # whole components went: nothing split
        assert np.array_equal(np.sort(after.records["size"]), np.sort(before.records["size"][~small]))
        again, stats2, cleared2, freed2 = cr.remove(out, min_size, None, t, c)         # idempotent
        assert stats2["removed_voxels"] == 0 and not cleared2 and not freed2
        for k in out:                                                                  # the other class keeps its bits
            keep = ~cr.node_mask(model[k][0], model[k][1], t)
            for i in (0, 1):
                assert np.array_equal(out[k][i][keep].view(np.uint32), np.asarray(model[k][i], np.float32)[keep].view(np.uint32))
            gone = cleared.get(k, np.zeros(512, bool))
            assert not out[k][0][gone].any() and not out[k][1][gone].any()
