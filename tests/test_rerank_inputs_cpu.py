"""CPU: the surface and the inputs of the re-ranking calls (sert_scorer_pairs, sert_scorer_rank_candidates) -- the symbols, the
case builders of tests/rerank_cases.py, the wrapper's CSR helper, bin/query.py's load_candidates and the loglinear callback's
filter.  tests/test_gpu_rerank.py runs the cases on the device."""
import logging
import os
import re
import sys
import types

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import scoring
from tests import rerank_cases as R
from tests import util as U

NEW_SYMBOLS = ('sert_scorer_pairs', 'sert_scorer_rank_candidates', 'sert_debug_scorer_rerank_counts')


def _declared(header):
    src = open(os.path.join(U.ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\b(sert_[a-z_0-9]+)\s*\(', src))


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(C.EXPORTS)
    assert set(NEW_SYMBOLS[:2]) <= _declared('sert_hip.h') and NEW_SYMBOLS[2] in _declared('sert_hip_debug.h')
    assert NEW_SYMBOLS[2] not in _declared('sert_hip.h')
    for name in ('score_pairs', 'rank_candidates', 'debug_rerank_counts'):
        assert callable(getattr(C.Scorer, name))


@pytest.mark.parametrize('name', R.EXACT_NAMES)
def test_exact_lists_follow_the_ladder_and_hold_ties(name):
    case = R.exact_case(name)
    V = case['E'].shape[0]
    steps = R.ladder(V)
    assert steps == (1, 2, 3, 33, 257, V // 2, V)
    lengths = [len(lst) for lst in case['lists']]
    assert lengths == case['lengths'] and lengths[-1] == 0 and len(lengths) == case['P'].shape[0] >= 8
    assert lengths[:-1] == [min(steps[i % 7], V) for i in range(len(lengths) - 1)] and set(min(s, V) for s in steps) <= set(lengths)
    assert (max(lengths) > R.LDS_MAX) == (name == 'fused_smallest')            # the slab path: the prefiltered problem
    for lst, c16, (ents, val) in zip(case['lists'], case['c16'], case['want']):
        assert lst.dtype == np.int32 and np.all(np.diff(lst) > 0) and (lst.size == 0 or (0 <= lst[0] and lst[-1] < V))
        assert np.all(np.abs(c16) <= 16)
        if len(lst) > 33:                       # 33 levels, more candidates: the tie-break is exercised
            assert len(np.unique(c16)) < len(lst)
        assert ents.dtype == np.int32 and val.dtype == np.float32 and sorted(ents.tolist()) == lst.tolist()
        # the ranking restated: 16 cos descending, equal values by entity
        pos = np.searchsorted(lst, ents)
        keys = list(zip((-c16[pos]).tolist(), ents.tolist()))
        assert keys == sorted(keys)
        assert np.array_equal(val, ((c16[pos] + 16) / 32.0).astype(np.float32))


def test_form_prefilter_width_and_k_cases():
    E, P, lists = R.form_case()
    assert E.shape == (9000, 16) and P.shape[0] == 9
    assert [len(x) for x in lists] == [1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 9000]
    assert sum(len(x) <= R.LDS_MAX for x in lists) == 7
    E, P, lists = R.prefilter_case()
    assert E.shape == (40000, 16) and sorted(set(len(x) for x in lists)) == [100, 9000, 40000]
    assert np.array_equal(lists[2], np.arange(40000))
    for d in R.WIDTHS:
        E, P, lists, cos = R.width_case(d)
        assert E.shape == (500, d) and P.shape == (4, d) and all(len(x) == 200 for x in lists)
        assert all(c.dtype == np.float64 and np.all(np.abs(c) <= 1 + 1e-12) for c in cos)
        assert R.width_bound(d) == (2 * d + 8) * 2.0 ** -24
    assert [d % 4 for d in R.WIDTHS].count(2) == 1
    E, P, lists = R.k_case()
    lengths = [len(x) for x in lists]
    assert lengths.count(0) == 2 and max(lengths) > R.LDS_MAX and max(R.K_VALUES) > max(lengths)
    assert R.K_VALUES[:3] == (1, 5, 1500)
    for lst in lists:
        assert np.all(np.diff(lst) > 0)


def test_chunk_case_is_cut_into_two_chunks_of_several_queries():
    """The planner's arithmetic restated with kRankLdsMax = 8192, kSortMaxBins = 2048 and kSortTile = 2048: the budgets of
    CHUNK_BUDGETS cut CHUNK_LENGTHS at queries [0, 4) and [4, 9) -- and so does every budget from 800 000 to 1 100 000 for the
    whole lists, so that 1 000 000 sits mid-range.  tests/test_gpu_rerank.py asserts the device's chunk count against this."""
    assert (R.LDS_MAX, R.SORT_MAX_BINS, R.SORT_TILE) == (8192, 2048, 2048)
    E, P, lists = R.chunk_case()
    assert E.shape == (9000, 16) and P.shape == (9, 16)
    assert tuple(len(x) for x in lists) == R.CHUNK_LENGTHS == (8200, 300, 8300, 5, 8250, 1100, 0, 8193, 2000)
    for lst in lists:
        assert lst.dtype == np.int32 and np.all(np.diff(lst) > 0)
    assert R.CHUNK_BUDGETS == {None: 1000000, 7: 600000} and R.CHUNK_BOUNDS == [0, 4, 9]
    for k, budget in R.CHUNK_BUDGETS.items():
        assert R.plan_chunks(R.CHUNK_LENGTHS, k, budget) == R.CHUNK_BOUNDS, (k, budget)
    for budget in range(800000, 1100001, 10000):
        assert R.plan_chunks(R.CHUNK_LENGTHS, None, budget) == R.CHUNK_BOUNDS, budget
    # the plan's other ends: everything in one chunk, one query per chunk
    assert R.plan_chunks(R.CHUNK_LENGTHS, None, 2 << 30) == [0, 9]
    assert R.plan_chunks(R.CHUNK_LENGTHS, None, 1) == list(range(10))
    # what the second chunk holds: two slab rows of unequal length, two lists of the 2048-entry LDS kernel (the first chunk's
    # two are of the 1024-entry one), an empty list
    second = R.CHUNK_LENGTHS[4:]
    slab = [n for n in second if n > R.LDS_MAX]
    assert len(slab) == 2 and slab[0] != slab[1] and 0 in second
    assert sorted(n for n in second if 0 < n <= R.LDS_MAX) == [1100, 2000] and sorted(n for n in R.CHUNK_LENGTHS[:4] if n <= R.LDS_MAX) == [5, 300]
    assert sum(0 < n <= R.LDS_MAX for n in R.CHUNK_LENGTHS) == 4 and sum(n > R.LDS_MAX for n in R.CHUNK_LENGTHS) == 4


@pytest.mark.parametrize('V', [1100, 8300])
def test_special_expectations_put_nans_last_by_entity(V):
    E, P, lists = R.special_case(V)
    zero = list(R.ZERO_ROWS(V))
    want = R.special_expected(E, P, lists)
    assert all(len(x) > R.LDS_MAX for x in lists) == (V == 8300)
    for q, (lst, (ents, val)) in enumerate(zip(lists, want)):
        assert set(zero) <= set(lst.tolist())
        if q in R.NAN_QUERIES:
            assert np.array_equal(ents, lst) and np.isnan(val).all()
        else:
            assert ents[-3:].tolist() == zero and np.isnan(val[-3:]).all() and not np.isnan(val[:-3]).any()
            assert np.all(np.diff(val[:-3]) <= 0)


def test_csr_helper_of_the_wrapper():
    lists = [[5, 2, 9, 2], [], np.array([7], dtype=np.int64), [3, 1, 3, 3, 0]]
    indptr, ents = C.candidates_csr(lists)
    assert indptr.dtype == np.int64 and ents.dtype == np.int32
    assert indptr.tolist() == [0, 4, 4, 5, 10] and ents.tolist() == [5, 2, 9, 2, 7, 3, 1, 3, 3, 0]       # order and duplicates kept
    indptr, ents = C.candidates_csr(lists, unique=True)
    assert indptr.tolist() == [0, 3, 3, 4, 7] and ents.tolist() == [2, 5, 9, 7, 0, 1, 3]
    assert C.ranked_indptr(indptr).tolist() == [0, 3, 3, 4, 7]
    assert C.ranked_indptr(indptr, 1).tolist() == [0, 1, 1, 2, 3]
    assert C.ranked_indptr(indptr, 2).tolist() == [0, 2, 2, 3, 5]
    assert C.ranked_indptr(indptr, 100).tolist() == [0, 3, 3, 4, 7] and C.ranked_indptr(indptr, 100).dtype == np.int64
    e_indptr, e_ents = C.candidates_csr([])
    assert e_indptr.tolist() == [0] and e_ents.size == 0
    with pytest.raises(C.SertError):
        C.candidates_csr([[0.5, 1.0]])


def _query_cli():
    sys.path.insert(0, os.path.join(U.ROOT, 'bin'))
    try:
        import query
    finally:
        sys.path.pop(0)
    return query


def test_load_candidates(tmp_path, caplog):
    inv = {i: 'E%03d' % i for i in range(12)}
    a, b = tmp_path / 'first_stage_a', tmp_path / 'first_stage_b'
    a.write_text(u't1 Q0 E007 1 0.9 run\nt1 Q0 E002 2 0.8 run\nt1 Q0 E007 3 0.7 run\nt2 Q0 E999 1 0.5 run\n'
                 u't3 Q0 E011 1 0.5 run\n')
    b.write_text(u't1 Q0 E000 1 0.9 other\nt1 Q0 NOPE 2 0.8 other\nt3 Q0 E001 1 0.4 other\nt3 Q0 E011 2 0.3 other\n')
    with caplog.at_level(logging.WARNING):
        got = _query_cli().load_candidates([str(a), str(b)], inv)
    assert sorted(got) == ['t1', 't3']                                  # t2 has nothing left: absent
    assert got['t1'].tolist() == [0, 2, 7] and got['t3'].tolist() == [1, 11]
    assert all(v.dtype == np.int32 for v in got.values())
    dropped = [r.getMessage() for r in caplog.records if 'Dropped' in r.getMessage()]
    assert len(dropped) == 1 and '2' in dropped[0]


def test_loglinear_callback_filters_the_full_ranking():
    rng = np.random.RandomState(3)
    dist = rng.rand(3, 40) + 0.01
    dist[1, ::7] = 0.0                          # (zeros are skipped by the product)
    dist /= dist.sum(axis=1)[:, None]
    seen = {}

    def collect(topic, idx, score):
        seen[topic] = (np.array(idx), np.array(score))

    args = (types.SimpleNamespace(top=None), types.SimpleNamespace(), {}, None, collect)
    scoring.LogLinearCallback(*args).process([1, 2, 3], dist.copy(), 'full')
    cand = {'t': np.array([31, 4, 17, 4, 0], dtype=np.int32), 'none': np.zeros(0, dtype=np.int32)}
    cb = scoring.LogLinearCallback(*args, candidates=cand)
    cb.process([1, 2, 3], dist.copy(), 't')
    cb.process([1, 2, 3], dist.copy(), 'none')
    cb.process([1, 2, 3], dist.copy(), 'unlisted')
    idx, score = seen['full']
    assert idx.shape == (40,)
    keep = np.isin(idx, cand['t'])
    assert keep.sum() == 4
    assert np.array_equal(seen['t'][0], idx[keep]) and np.array_equal(seen['t'][1], score[keep])       # same order, same scores
    assert seen['none'][0].size == 0 and seen['unlisted'][0].size == 0

    # the device-ranked batch goes through the same filter
    ranking = types.SimpleNamespace(status=[0], idx=[idx], score=[score], k=None, joint_entropy=[0.5], token_entropy=[[0.5] * 3])
    cb2 = scoring.LogLinearCallback(*args, candidates=cand)
    cb2.process_batch([[1, 2, 3]], ranking, [{'topic_id': 't'}])
    assert np.array_equal(seen['t'][0], idx[keep]) and np.array_equal(seen['t'][1], score[keep])
