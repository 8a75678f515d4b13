"""CPU: the one ranking order of the cosine scorer ("One ranking order") as the oracle states it, and the proof
that the exact problems of tests/util.py are exact -- the licence for tests/test_gpu_score_contract.py to demand equal indices
and bit-equal values with no exemption."""
import numpy as np
import pytest

from oracle import sert_oracle as O
from tests import util as U

POS_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
NEG_NAN = np.array([0xffc00000], dtype=np.uint32).view(np.float32)[0]
INF = np.float32(np.inf)


def f32(*xs):
    return np.array(xs, dtype=np.float32)


def test_the_two_nan_patterns_are_what_they_claim():
    assert np.isnan(POS_NAN) and not np.signbit(POS_NAN)
    assert np.isnan(NEG_NAN) and np.signbit(NEG_NAN)


@pytest.mark.parametrize('values,expect', [
    (f32(0.25, 1.0, -1.0, 0.5), [1, 3, 0, 2]),                               # descending
    (f32(0.5, 0.25, 0.5, 0.25, 0.5), [0, 2, 4, 1, 3]),                       # ties: lowest index
    (f32(-0.0, 0.0, 0.0, -0.0), [0, 1, 2, 3]),                               # +0 and -0 are one value
    (f32(0.0, -0.0, 1e-45, -1e-45), [2, 0, 1, 3]),                           # ... between the two smallest denormals
    (f32(-INF, 3e38, INF, -3e38, INF), [2, 4, 1, 3, 0]),                     # infinities are numbers
    (f32(POS_NAN, 1.0, NEG_NAN, -INF), [1, 3, 0, 2]),                        # NaN of either sign after -inf, by index
    (f32(NEG_NAN, POS_NAN, -1.0, POS_NAN, NEG_NAN), [2, 0, 1, 3, 4]),
    (f32(POS_NAN, NEG_NAN, NEG_NAN, POS_NAN), [0, 1, 2, 3]),                 # all NaN: 0, 1, 2, ...
    (f32(0.125, 0.125, 0.125), [0, 1, 2]),                                   # all equal
    (f32(7.0), [0]),
])
def test_rank_order_hand_written_cases(values, expect):
    assert O.rank_order(values).tolist() == expect
    for top in range(1, len(expect) + 2):
        got = O.rank_order(values, top)
        assert got.tolist() == expect[:top]                 # every top-k is the head of the full ranking
        assert got.dtype == np.int64
    assert O.rank_order(values.astype(np.float64)).tolist() == expect


def test_the_device_key_restated_in_numpy_sorts_like_rank_order():
    """score_key (csrc/common.h), restated in tests/util.py: ascending (key, index) is the contract's order, the key of a NaN
    is the last one and decodes to a NaN, the two zeros share a key."""
    rng = np.random.RandomState(3)
    v = np.concatenate([f32(0.0, -0.0, INF, -INF, POS_NAN, NEG_NAN, 1e-45, -1e-45, 1.0, -1.0, 0.5, 0.5, NEG_NAN, -0.0),
                        rng.randn(200).astype(np.float32), np.round(rng.randn(200) * 4).astype(np.float32) / 16])
    v = v[rng.permutation(v.size)]
    key = U.score_key(v)
    by_key = np.lexsort((np.arange(v.size), key))
    assert np.array_equal(by_key, O.rank_order(v))
    assert np.all(key[np.isnan(v)] == 0xffffffff) and np.all(key[~np.isnan(v)] < 0xffffffff)
    assert len(set(key[v == 0].tolist())) == 1


def test_score_map_is_not_injective_below_one_half():
    """Why the COSINE is ordered and the score applied afterwards: (cos + 1)/2 rounds pairs of cosines below 0.5 to one
    score, and both zeros to 0.5."""
    c = np.float32(0.25)
    c2 = np.nextafter(c, np.float32(1))
    assert c2 > c and (c + np.float32(1)) / np.float32(2) == (c2 + np.float32(1)) / np.float32(2)
    assert (np.float32(-0.0) + np.float32(1)) / np.float32(2) == np.float32(0.5)


# ---- the exact problems -------------------------------------------------------------------------------------------------

def _bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def _unit_rows_f32(X):
    X = X.astype(np.float32)
    ss = np.zeros(X.shape[0], dtype=np.float32)
    for c in range(X.shape[1]):
        ss = ss + X[:, c] * X[:, c]
    return X / np.sqrt(ss)[:, None]


def _cos_f32(Pn, En, order):
    """float32 cosines with the products summed in float32 in the given column order (one rounding per addition)."""
    acc = np.zeros((Pn.shape[0], En.shape[0]), dtype=np.float32)
    for c in order:
        acc = acc + Pn[:, c, None] * En[None, :, c]
    return acc


def _cos_f32_pairwise(Pn, En):
    terms = [Pn[:, c, None] * En[None, :, c] for c in range(Pn.shape[1])]
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


@pytest.mark.parametrize('name', sorted(U.EXACT_SHAPES))
def test_exact_problems_are_exact_in_fp32_in_any_order_and_in_bf16(name):
    p = U.exact_score_problem(name)
    seed, V, d, Q, mix = U.EXACT_SHAPES[name]
    assert p['E'].shape == (V, d) and p['P'].shape == (Q, d)
    for X in (p['Ei'], p['Pi']):
        assert set(np.unique(X).tolist()) <= {-1, 0, 1}
        assert set(np.unique((X != 0).sum(axis=1)).tolist()) <= set(U.EXACT_NNZ)
    assert set(np.unique((p['Ei'] != 0).sum(axis=1)).tolist()) == set(U.EXACT_NNZ)      # every kind of row is there
    c16 = U.exact_cos16(p['Pi'], p['Ei'])
    assert c16.min() >= -16 and c16.max() <= 16
    want = (c16.astype(np.float64) / 16.0).astype(np.float32)
    assert np.array_equal(want.astype(np.float64) * 16.0, c16)                          # a multiple of 1/16 IS a float32
    Pn, En = _unit_rows_f32(p['P']), _unit_rows_f32(p['E'])
    assert set(np.unique(np.abs(En)).tolist()) <= {0.0, 0.25, 0.5, 1.0}
    cols = list(range(d))
    for got in (_cos_f32(Pn, En, cols), _cos_f32(Pn, En, cols[::-1]), _cos_f32_pairwise(Pn, En),
                _cos_f32(_bf16_round(Pn), _bf16_round(En), cols)):
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32) & 0x7fffffff, want.view(np.uint32) & 0x7fffffff)   # (a zero of either sign)
        assert np.array_equal(got, want)
    assert np.array_equal(_bf16_round(En), En) and np.array_equal(_bf16_round(Pn), Pn)
    # the emitted score is exact as well, and the expected ranking has the ties the tests are after
    idx, val = U.exact_expected(c16, min(V, 100))
    assert np.array_equal(val.astype(np.float64) * 32.0, np.take_along_axis(c16, idx.astype(np.int64), axis=1) + 16)
    assert any(len(set(row.tolist())) < len(row) for row in val)
    for q in range(Q):
        assert len(set(idx[q].tolist())) == idx.shape[1]


def test_exact_expected_marks_directionless_rows():
    p = U.exact_score_problem('tiny')
    c16 = U.exact_cos16(p['Pi'], p['Ei'])
    idx, val = U.exact_expected(c16, 50, nan_entities=(0, 17), nan_queries=(2,))
    for q in range(idx.shape[0]):
        assert sorted(idx[q].tolist()) == list(range(50))
        if q == 2:
            assert idx[q].tolist() == list(range(50)) and np.isnan(val[q]).all()
        else:
            assert idx[q][-2:].tolist() == [0, 17] and np.isnan(val[q][-2:]).all() and not np.isnan(val[q][:-2]).any()
    assert U.same_bits(val, val.copy()) and not U.same_bits(val, np.nan_to_num(val))


def test_threshold_bin_load_reaches_both_selection_kernels_of_topk_rows():
    """topk_rows (csrc/kernels_score.h) sorts the threshold bin of an 11-bit key histogram in a 2048-entry list and falls
    back to a radix select when the bin holds more: the shapes meant for either side are on that side."""
    assert max(U.threshold_bin_load('mid', 100)) <= 2048
    assert max(U.threshold_bin_load('unaligned_rows', 100)) <= 2048
    assert max(U.threshold_bin_load('radix_fallback', 400)) > 2048


def test_gaussian_tables_have_equal_scores_of_different_cosines():
    """The shape of the prefix test's non-vacuity assertion, on the float32 oracle: among the first 1024 of 40 000 Gaussian
    entities at d = 16, some query has two entities with one emitted score and two cosines."""
    E, P = U.gaussian_score_problem(40000, 16, 100)
    assert U.count_score_collisions(U.oracle_cosines_f32(E, P), 1024) > 0
