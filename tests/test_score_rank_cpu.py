"""No GPU: the inputs of tests/test_gpu_score_rank.py have the properties that test relies on -- so that its exact
comparison of the device ranking (sert_scorer_rank) with oracle.rank_order says something."""
import numpy as np
import pytest

from oracle import sert_oracle as O
from tests import score_rank_cases as K
from tests import util as U


@pytest.mark.parametrize('V', K.SPECIAL_V)
def test_special_rows_hold_what_they_are_there_for(V):
    rows = K.special_rows(V)
    assert rows.shape == (K.SPECIAL_Q, V) and rows.dtype == np.float32
    r, bits = rows[0], rows[0].view(np.uint32)
    assert np.any(bits == 0) and np.any(bits == 0x80000000)                               # both zeros
    assert np.any(np.isnan(r) & (bits >> 31 == 0)) and np.any(np.isnan(r) & (bits >> 31 == 1))   # NaNs of both signs
    assert np.any(r == np.inf) and np.any(r == -np.inf)
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert np.any((r != 0) & (np.abs(r) < tiny))                                          # denormals
    numbers = r[~np.isnan(r)]
    assert np.unique(numbers).size < numbers.size                                         # duplicates
    assert np.isnan(rows[1]).all() and len(set((rows[1].view(np.uint32) >> 31).tolist())) == 2
    assert np.count_nonzero(rows[2] == 0) > V // 2
    assert np.unique(rows[3][~np.isnan(rows[3])]).size <= 7


@pytest.mark.parametrize('V', K.SPECIAL_V)
def test_rank_order_on_the_special_rows(V):
    """NaNs last and by index, the two zeros tied (index decides), the permutation complete, every prefix its head."""
    rows = K.special_rows(V)
    for q, row in enumerate(rows):
        order = O.rank_order(row)
        assert np.array_equal(np.sort(order), np.arange(V)), q
        ranked = row[order]
        nnan = int(np.isnan(row).sum())
        assert not np.isnan(ranked[:V - nnan]).any() and np.isnan(ranked[V - nnan:]).all(), q
        assert np.all(np.diff(order[V - nnan:]) > 0), q                                   # the NaNs by index, whatever their sign
        nums = ranked[:V - nnan]
        assert np.all(nums[1:] <= nums[:-1]), q                                           # descending (+0 == -0 here)
        same = nums[1:] == nums[:-1]
        assert np.all(np.diff(order[:V - nnan])[same] > 0), q                             # ties by lowest index
        zeros = order[:V - nnan][nums == 0]
        if q in (0, 2):
            signs = np.signbit(row[zeros])
            assert signs.any() and not signs.all() and np.any(signs[:-1] & ~signs[1:]), q  # a -0 ranked before a +0
        for k in (1, 100, 1500):
            assert np.array_equal(O.rank_order(row, k), order[:k])
    assert np.array_equal(O.rank_order(rows[1]), np.arange(V))                            # all NaN: 0, 1, 2, ...
    idx, val = K.expected(rows, 1500)
    assert idx.shape == (K.SPECIAL_Q, min(V, 1500)) and np.isnan(val[1]).all()
    full = K.expected(rows)[1]
    assert np.any(full[0] == np.inf) and np.any(full[0] == -np.inf)          # (inf + 1)/2 and (-inf + 1)/2 stay what they are


@pytest.mark.parametrize('V', K.SPECIAL_V)
def test_score_and_cosine_part_inside_the_ranked_depth(V):
    """Two entities with one emitted score (cos + 1)/2 and two cosines among the first entities of row 0: a kernel that
    ordered the score instead of the cosine would rank them by index -- the comparison on the GPU is not vacuous."""
    rows = K.special_rows(V)
    assert U.count_score_collisions(rows[:1], min(V, 1500)) == 1
    order = O.rank_order(rows[0])
    a, b = int(np.nonzero(order == V - 1)[0][0]), int(np.nonzero(order == 1)[0][0])
    assert a < b, 'the larger cosine sits at the higher index: ordering by score and then by index would swap the two'
    sc = (rows[0] + np.float32(1)) / np.float32(2)
    assert sc[1] == sc[V - 1] and rows[0][1] != rows[0][V - 1]


def test_the_tie_heavy_table_is_tie_heavy():
    """'radix_fallback' (V 6000, the stability case of the LDS sort) and 'prefix' (V 40000, of the counting-sort passes):
    thousands of entities per query share a cosine, so the order inside a level is the index order or the sort is not
    stable; rank_order gives a complete permutation with the levels in index order."""
    for name, floor in (('radix_fallback', 2000), ('prefix', 10000)):
        p = U.exact_score_problem(name)
        cos = U.exact_cos16(p['Pi'], p['Ei']).astype(np.float32) / np.float32(16)
        for q, row in enumerate(cos):
            order = O.rank_order(row)
            assert np.array_equal(np.sort(order), np.arange(row.size))
            ranked = row[order]
            assert np.all(ranked[1:] <= ranked[:-1])
            same = ranked[1:] == ranked[:-1]
            assert np.all(np.diff(order)[same] > 0)
            levels, counts = np.unique(row, return_counts=True)
            assert counts.max() >= floor and levels.size <= 33, (name, q, counts.max(), levels.size)


def test_path_and_footprint_restatement():
    """The shapes of the GPU test reach the path they are named for, and a budget of chunk_bytes(.., 2) holds two queries."""
    assert K.rank_path(50, None) == (K.PATH_TOPK, 50) and K.rank_path(300, 2000) == (K.PATH_TOPK, 300)
    assert K.rank_path(1024, None)[0] == K.PATH_TOPK and K.rank_path(1025, None) == (K.PATH_LDS, 1025)
    assert K.rank_path(8192, 1025) == (K.PATH_LDS, 1025) and K.rank_path(8193, None) == (K.PATH_CSORT, 8193)
    assert K.rank_path(40000, 1024) == (K.PATH_TOPK, 1024) and K.rank_path(40000, 1500) == (K.PATH_CSORT, 1500)
    for V in (300, 1025, 8193):
        assert K.chunk_bytes(V, None, 2) < K.chunk_bytes(V, None, 3)
    assert K.chunk_bytes(8193, None, 2048) < (2 << 30)        # the 2048-query cap, not the default budget, cuts Q = 2049
