"""tests/merge_ref.py, the executable form of vh_merge's rule, on ball shells (tests/merge_cases.py): the identity copy, the
candidate box as a superset of what can receive a sample for every transform and voxel-size pair the GPU tests use, the
over-allocation it costs, and both branches of the update with the cap."""
import numpy as np
import pytest

import merge_cases as MC
import merge_ref as R
import sample_ref as S

F = np.float32
U = np.uint32
BIG = 1e9


def inverse(T):
    """(the GPU tests use the library's cofactor inverse; here any inverse of a rigid transform serves the properties checked)"""
    return np.linalg.inv(np.asarray(T, np.float64)).astype(F)


@pytest.fixture(scope="module")
def ball():
    model = MC.shell()
    assert 30 <= len(model) <= 80, len(model)
    return model


def test_nearest_identity_is_an_exact_copy(ball):
    vs = F(2.0 ** -5)
    keys, records = R.candidates(ball.keys(), MC.IDENTITY, vs, vs)
    assert keys == set(ball) and records == len(ball)
    out, stats = R.apply(MC.with_new_blocks({}, keys), ball, keys, MC.IDENTITY, vs, vs, BIG, 255.0, R.NEAREST)
    copied = 0
    for k, (s, w) in ball.items():
        valid = w > 0
        assert np.array_equal(out[k][0][valid].view(U), s[valid].view(U)) and np.array_equal(out[k][1][valid].view(U), w[valid].view(U))
        assert not out[k][0][~valid].view(U).any() and not out[k][1][~valid].view(U).any()        # a dead voxel gives nothing
        copied += int(valid.sum())
    assert stats["fresh"] == copied and stats["combined"] == 0 and stats["empty_blocks"] == 0
    # a voxel size that is no power of two: the source's blocks, and now and then k + 1, which stays empty
    keys4, _ = R.candidates(ball.keys(), MC.IDENTITY, MC.VS, MC.VS)
    assert keys4 >= set(ball)
    extra = keys4 - set(ball)
    s, _ = R.samples(ball, sorted(extra), MC.IDENTITY, MC.VS, MC.VS, R.NEAREST) if extra else (np.zeros((0, 512), F), None)
    assert np.isnan(s).all()


PAIRS = [("identity", MC.IDENTITY, 1.0), ("oblique", MC.OBLIQUE, 1.0), ("steep", MC.STEEP, 1.0), ("half-shift", MC.HALF_SHIFT, 1.0),
         ("oblique", MC.OBLIQUE, 0.5), ("oblique", MC.OBLIQUE, 2.0)]


@pytest.mark.parametrize("name,T,ratio", PAIRS, ids=[f"{n}-{r}" for n, _, r in PAIRS])
def test_no_sample_outside_the_candidates(ball, name, T, ratio):
    vs_s, vs_d = F(MC.VS), F(MC.VS * ratio)
    keys, records = R.candidates(ball.keys(), T, vs_s, vs_d)
    assert R.skipped(ball.keys(), T, vs_s, vs_d) == 0 and records >= len(keys)
    outside = sorted(MC.dilation(keys) - keys)
    assert outside
    Tinv = inverse(T)
    for mode in (R.NEAREST, R.TRILINEAR):
        s, w = R.samples(ball, outside, Tinv, vs_s, vs_d, mode)
        assert not (s == s).any() and not (w > 0).any(), (name, ratio, mode, int((s == s).sum()))
    # inside, the rule finds something: the test above is not vacuous
    s, _ = R.samples(ball, sorted(keys), Tinv, vs_s, vs_d, R.NEAREST)
    assert (s == s).sum() > 1000
    print(f"{name} x{ratio}: {len(ball)} source blocks, {len(keys)} candidates, {records} records, "
          f"{int((~(s == s).any(1)).sum())} candidates without a nearest sample")


def test_the_oblique_case_over_allocates(ball):
    vs = F(MC.VS)
    keys, _ = R.candidates(ball.keys(), MC.OBLIQUE, vs, vs)
    assert len(keys) > len(ball)
    out, stats = R.apply(MC.with_new_blocks({}, keys), ball, keys, inverse(MC.OBLIQUE), vs, vs, BIG, 255.0, R.TRILINEAR)
    assert 0 < stats["empty_blocks"] < len(keys) and stats["blocks"] == len(keys)       # something for the collection to free
    assert stats["fresh"] > 0


def test_both_branches_and_the_cap(ball):
    vs = F(MC.VS)
    Tinv = inverse(MC.HALF_SHIFT)
    keys, _ = R.candidates(ball.keys(), MC.HALF_SHIFT, vs, vs)
    # dst: the same shell with every other block missing, weights 1; the cap at 1.5 is below 1 + 1
    dst = {k: v for i, (k, v) in enumerate(sorted(ball.items())) if i % 2 == 0}
    before = MC.with_new_blocks(dst, keys)
    out, stats = R.apply(before, ball, keys, Tinv, vs, vs, 3.0, 1.5, R.TRILINEAR)
    assert stats["fresh"] > 0 and stats["combined"] > 0 and stats["capped"] > 0 and stats["untouched"] > 0, stats
    worst_w = max(float(w.max()) for _, w in out.values())
    assert worst_w == 1.5
    assert max(float(np.abs(s[w > 0]).max()) for s, w in out.values() if (w > 0).any()) <= max(3.0, max(float(np.abs(s).max()) for s, _ in dst.values()))
    # a block outside `keys` is never touched, and neither is the caller's model
    k0 = sorted(dst)[0]
    out2, _ = R.apply(before, ball, [k for k in keys if k != k0], Tinv, vs, vs, 3.0, 1.5, R.TRILINEAR)
    assert np.array_equal(out2[k0][0].view(U), before[k0][0].view(U)) and np.array_equal(out2[k0][1].view(U), before[k0][1].view(U))


def test_a_block_outside_the_domain_is_skipped():
    far = [(0, 0, 0), ((1 << 27), 0, 0)]                     # 8 * 2^27 = 2^30 source voxels: outside at equal voxel sizes
    vs = F(MC.VS)
    assert R.skipped(far, MC.IDENTITY, vs, vs) == 1
    keys, records = R.candidates(far, MC.IDENTITY, vs, vs)
    assert (0, 0, 0) in keys and all(abs(k[0]) < 4 for k in keys) and records == len(keys)
