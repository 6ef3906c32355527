"""The label rule without a GPU: properties of tests/labels_ref.py (include/voxelhash.h, "the model with labels") on crafted
words and on the oracle's model of the small room scenes (tests/deintegrate_cases.py)."""
import numpy as np
import pytest

import deintegrate_cases as DC
import deintegrate_ref as R
import labels_cases as LC
import labels_ref as LR

F = np.float32
U = np.uint32
VS = DC.KW["voxelSize"]
BAND = 1.5 * VS


# ---- the vote table ----------------------------------------------------------------------------------------------------------
def one(word, pixel, vote_max):
    out, kind = LR.vote(np.array([word], U), np.array([pixel], U), vote_max)
    return int(out[0]), LR.TRANSITIONS[int(kind[0])]


def test_every_transition_of_the_vote_table():
    P = lambda l, n: int(LR.pack(l, n))
    assert one(0, 5, 3) == (P(5, 1), "fresh")
    assert one(P(5, 1), 5, 3) == (P(5, 2), "increment")
    assert one(P(5, 2), 5, 3) == (P(5, 3), "increment")
    assert one(P(5, 3), 5, 3) == (P(5, 3), "held")
    assert one(P(5, 3), 6, 3) == (P(5, 2), "decrement")
    assert one(P(5, 2), 6, 3) == (P(5, 1), "decrement")
    assert one(P(5, 1), 6, 3) == (0, "reset")
    assert one(0, 6, 3) == (P(6, 1), "fresh")
    # the ends of both fields
    assert one(0, 65535, 65535) == (P(65535, 1), "fresh")
    assert one(P(65535, 65534), 65535, 65535) == (P(65535, 65535), "increment")
    assert one(P(65535, 65535), 65535, 65535) == (P(65535, 65535), "held")
    assert one(P(65535, 65535), 1, 65535) == (P(65535, 65534), "decrement")
    assert one(P(1, 1), 65535, 65535) == (0, "reset")
    # vote_max 1: a voxel changes its mind in two votes
    assert one(0, 4, 1) == (P(4, 1), "fresh")
    assert one(P(4, 1), 4, 1) == (P(4, 1), "held")
    assert one(P(4, 1), 9, 1) == (0, "reset")
    # a word above a smaller cap (an earlier call had a larger one) comes down to the cap
    assert one(P(4, 9), 4, 3)[0] == P(4, 3)
    assert one(P(4, 9), 5, 3) == (P(4, 8), "decrement")


def test_the_cap_bounds_the_votes_it_takes_to_change_a_label():
    for cap in (1, 2, 7):
        word = np.zeros(1, U)
        for _ in range(50):
            word, _ = LR.vote(word, 3, cap)
        assert int(word[0]) == int(LR.pack(3, cap))
        for k in range(cap):
            assert int(LR.label_of(word)[0]) == 3
            word, _ = LR.vote(word, 8, cap)
        assert int(word[0]) == 0
        word, _ = LR.vote(word, 8, cap)
        assert int(word[0]) == int(LR.pack(8, 1))


def test_a_strict_majority_ends_as_the_stored_label():
    rng = np.random.default_rng(11)
    n, length = 500, 41
    major = rng.integers(1, 1000, n)
    seq = rng.integers(1, 1000, (n, length))
    for row in range(n):                                                  # 21 of the 41 votes, anywhere in the sequence
        seq[row, rng.permutation(length)[:21]] = major[row]
    seq[seq == 0] = 1
    word = np.zeros(n, U)
    for t in range(length):
        word, _ = LR.vote(word, seq[:, t].astype(U), 65535)               # (the cap out of reach)
    assert np.array_equal(LR.label_of(word), major.astype(U))
    assert (LR.votes_of(word) >= 1).all()


# ---- fusing over the oracle's model -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle):
    """The oracle's model of the three frames (PINHOLE), its table, volume and the compact set of frame 1's pose."""
    ot = DC.oracle_table(oracle, 1)
    frames = DC.frames(oracle)
    for pose, _, verts in frames:
        ot.integrate(pose, verts)
    pose, d16, verts = frames[1]
    proj, inv = DC.projection(1), oracle.invert4x4(pose)
    tab, vox = ot.hash_table().copy(), ot.sdf_blocks().copy()
    entries = tab[R.visible_entries(tab, ot.params, 1, proj, pose, inv, DC.W, DC.H)]
    out = dict(params=ot.params, proj=proj, inv=inv, tab=tab, vox=vox, entries=entries, src=(d16, DC.k_inv()), pose=pose)
    yield out
    ot.close()


def fuse(sc, labels, image, band, vote_max, vox=None):
    return LR.integrate(labels, sc["vox"] if vox is None else vox, sc["entries"], sc["params"], 1, sc["proj"], sc["inv"], sc["src"],
                        image, band, vote_max)


def test_a_uniform_image_gives_one_word(scene):
    empty = np.zeros(len(scene["vox"]), U)
    image = np.full((DC.H, DC.W), 12, np.uint16)
    once, stats = fuse(scene, empty, image, BAND, 3)
    assert stats["fresh"] > 1000 and stats["voted"] == stats["fresh"] and stats["rejected"] > 0
    assert set(np.unique(once).tolist()) == {0, int(LR.pack(12, 1))}
    twice, _ = fuse(scene, once, image, BAND, 3)
    assert set(np.unique(twice).tolist()) == {0, int(LR.pack(12, 2))}
    # voxels that hold nothing never get a label, blocks off the list are untouched
    assert not once[~(scene["vox"]["weight"] > 0)].any()
    listed = np.zeros(len(once), bool)
    listed[(scene["entries"]["ptr"].astype(np.int64)[:, None] + np.arange(512)).ravel()] = True
    assert (~listed).any()
    marked = np.where(listed, once, LR.pack(7, 7))
    again, _ = fuse(scene, marked, image, BAND, 3)
    assert (again[~listed] == LR.pack(7, 7)).all()


def test_label_zero_pixels_and_vote_max_zero_change_nothing(scene):
    empty = np.zeros(len(scene["vox"]), U)
    once, _ = fuse(scene, empty, LC.image(0), BAND, 3)
    assert once.any()
    same, stats = fuse(scene, once, np.zeros((DC.H, DC.W), np.uint16), BAND, 3)
    assert np.array_equal(same, once) and stats["voted"] == 0 and stats["unlabelled"] > 1000
    same, stats = fuse(scene, once, LC.image(1), BAND, 0)
    assert np.array_equal(same, once) and stats["voted"] == 0 and stats["swept"] == 0


def test_a_wider_band_labels_a_superset(scene):
    empty = np.zeros(len(scene["vox"]), U)
    thin, st = fuse(scene, empty, LC.image(2), 0.5 * VS, 3)
    wide, sw = fuse(scene, empty, LC.image(2), 3.0 * VS, 3)
    assert 0 < st["voted"] < sw["voted"]
    assert not ((thin != 0) & (wide == 0)).any()
    assert np.array_equal(wide[thin != 0], thin[thin != 0])


def test_the_sweep_clears_what_holds_nothing(scene):
    empty = np.zeros(len(scene["vox"]), U)
    once, _ = fuse(scene, empty, LC.image(3), 3.0 * VS, 3)
    vox = scene["vox"].copy()
    at = int(scene["entries"]["ptr"][0])
    labelled = np.nonzero(once[at:at + 512])[0]
    assert len(labelled) > 0
    vox["weight"][at + labelled[0]] = 0.0                                  # as a de-integration leaves it
    swept, stats = fuse(scene, once, LC.image(4), 3.0 * VS, 0, vox)
    assert stats["swept"] == 1 and stats["voted"] == 0
    want = once.copy()
    want[at + labelled[0]] = 0
    assert np.array_equal(swept, want)


def model_of(tab, vox, labels, colour=None):
    out = {}
    for e in tab[tab["ptr"] != -1]:
        p = int(e["ptr"])
        v = (vox["sdf"][p:p + 512], vox["weight"][p:p + 512], labels[p:p + 512])
        out[tuple(e["pos"].tolist())] = v + ((colour[p:p + 512],) if colour is not None else ())
    return out


def test_the_bins_sum_to_the_valid_voxels(scene):
    labels = np.zeros(len(scene["vox"]), U)
    for i in range(3):
        labels, _ = fuse(scene, labels, LC.image(i) * np.uint16(5), BAND, 3)        # labels 5, 10, 15
    model = model_of(scene["tab"], scene["vox"], labels)
    valid = sum(int(LR.valid_mask(v[0], v[1]).sum()) for v in model.values())
    present = set(np.unique(LR.label_of(labels)).tolist()) - {0}
    assert present == {5, 10, 15} and valid > 1000
    full = LR.counts(model, 65536)
    assert full.sum() == valid and {int(i) for i in np.nonzero(full[1:])[0] + 1} == present
    for n_bins in (1, 6, 11, 15, 16):                                      # 15: one below the largest label present
        c = LR.counts(model, n_bins)
        assert len(c) == n_bins and c.sum() == valid
        assert np.array_equal(c[1:], full[1:n_bins])
        assert c[0] == full[0] + full[n_bins:].sum()
    strict = LR.counts(model, 16, min_votes=2)
    assert strict.sum() == valid and strict[0] > full[0] and (strict[1:] <= full[1:16]).all()
    keys = np.array(list(model))
    region = (keys.min(0), ((keys.min(0) + keys.max(0)) // 2 + 1))
    inside = {k: v for k, v in model.items() if LR.in_region(k, region)}
    assert 0 < len(inside) < len(model)
    assert np.array_equal(LR.counts(model, 16, region=region), LR.counts(inside, 16))


# ---- removal ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band, frees", [(10.0, True), (1.5 * VS, False)])
def test_removing_a_label_frees_blocks_only_when_the_band_covers_the_truncation(oracle, band, frees):
    ot = DC.oracle_table(oracle, 1)
    pose, d16, verts = DC.frames(oracle)[1]
    ot.integrate(pose, verts)
    proj, inv = DC.projection(1), oracle.invert4x4(pose)
    tab, vox = ot.hash_table().copy(), ot.sdf_blocks().copy()
    entries = tab[R.visible_entries(tab, ot.params, 1, proj, pose, inv, DC.W, DC.H)]
    labels, _ = LR.integrate(np.zeros(len(vox), U), vox, entries, ot.params, 1, proj, inv, (d16, DC.k_inv()), LC.halves(), band, 3)
    colour = np.where(labels != 0, U(0x01112233), U(0))
    model = model_of(tab, vox, labels, colour)
    ot.close()
    after, stats, freed = LR.remove(model, 7)
    touched = [k for k, v in model.items() if (LR.label_of(v[2]) == 7).any()]
    kept = [k for k in touched if k in after]
    print(f"band {band}: touched {len(touched)}, freed {len(freed)}, kept {len(kept)}")
    assert len(touched) > 0 and stats["blocks"] == len(model) and stats["freed_blocks"] == len(freed)
    assert stats["removed_voxels"] == int((LR.label_of(labels) == 7).sum())
    if frees:
        assert len(freed) > 0 and len(kept) > 0
    else:
        assert len(freed) == 0
    for k, v in after.items():
        assert not (LR.label_of(v[2]) == 7).any()
        gone = LR.label_of(model[k][2]) == 7
        assert not v[1][gone].any() and not v[0][gone].any() and not v[3][gone].any()
        for a, b in zip(v, model[k]):                                      # everything else keeps its bits
            assert np.array_equal(np.asarray(a)[~gone].view(U), np.asarray(b)[~gone].view(U))
    assert set(after) | set(freed) == set(model) and not set(after) & set(freed)
    # label 9 is still there, and removing 7 again removes nothing
    assert any((LR.label_of(v[2]) == 9).any() for v in after.values())
    assert LR.remove(after, 7)[1]["removed_voxels"] == 0
