"""CPU: the surface and the inputs of the loglinear re-ranking call (sert_ll_rank_candidates) -- the symbols, the case
builders of tests/ll_rerank_cases.py and their expectation.  tests/test_gpu_ll_rerank.py runs the cases on the device."""
import os
import re

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import inference, models, scoring
from tests import ll_rerank_cases as L
from tests import util as U

NEW_SYMBOLS = ('sert_ll_rank_candidates', 'sert_debug_ll_rank_candidates_distributions', 'sert_debug_ll_rerank_counts')


def _declared(header):
    src = open(os.path.join(U.ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\b(sert_[a-z_0-9]+)\s*\(', src))


def test_symbols_are_declared_and_bound():
    assert set(NEW_SYMBOLS) <= set(C.EXPORTS)
    assert NEW_SYMBOLS[0] in _declared('sert_hip.h') and set(NEW_SYMBOLS[1:]) <= _declared('sert_hip_debug.h')
    assert not set(NEW_SYMBOLS[1:]) & _declared('sert_hip.h')
    assert callable(C.Engine.ll_rank_candidates)
    assert callable(C.debug_ll_rank_candidates_distributions) and callable(C.debug_ll_rerank_counts)
    assert callable(scoring.LogLinearCallback.candidate_lists)
    import inspect
    assert 'candidates' in inspect.signature(models.LogLinearPredictFn.rank_queries).parameters
    r = inference.QueryRanking([], [], [], [], [])
    assert r.candidates is False


def _check_lists(lists, V):
    for lst in lists:
        assert lst.dtype == np.int32 and np.all(np.diff(lst) > 0)
        assert lst.size == 0 or (0 <= lst[0] and lst[-1] < V)


def test_every_list_is_strictly_ascending_and_in_range():
    _check_lists(L.golden_lists(25), 25)
    assert [len(x) for x in L.golden_lists(25)] == [25, 1, 13, 0]
    for V in L.TIED_LENGTHS:
        P, offsets, lists = L.tied_case(V)
        assert P.shape == (offsets[-1], V) and P.dtype == np.float32 and len(lists) == len(offsets) - 1
        _check_lists(lists, V)
    for name, Ve in (('small', 715), ('slab', 9000)):
        case = L.engine_case(name)
        assert case['W'].shape[1] == Ve and len(case['lists']) == len(case['queries'])
        assert all(1 <= len(q) <= 6 for q in case['queries'])
        _check_lists([np.unique(x).astype(np.int32) for x in case['lists']], Ve)       # (as the wrapper hands them over)
    small = L.engine_case('small')
    assert len(small['queries']) == 50 and len(small['lists'][0]) == 0 and len(small['lists'][1]) == 715
    assert np.any(np.diff(small['lists'][5]) < 0) and len(np.unique(small['lists'][5])) < len(small['lists'][5])
    slab = L.engine_case('slab')
    assert len(slab['queries']) == 12 and sum(len(x) > L.LDS_MAX for x in slab['lists']) == 1
    host = L.host_case()
    _check_lists(host['lists'], 4096)
    assert [len(q) for q in host['queries']] == [3, 60, 2]


def test_tied_lengths_cover_every_kernel_edge():
    assert sorted(len(x) for x in L.tied_case(8200)[2]) == [0, 1, 2, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 8200]
    assert set(len(x) for x in L.tied_case(8200)[2]) == {0, 1, 2, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 8200}
    assert [len(x) for x in L.tied_case(300)[2]] == [1, 2, 150, 300]
    assert max(k for k in L.K_VALUES if k) < 8192 and L.K_VALUES == (None, 1, 10, 5000)


def test_tied_inputs_follow_the_full_ranking_test():
    from tests import test_gpu_ll_rank as T
    assert np.array_equal(L.TIE_LEVELS, T.TIE_LEVELS)
    assert np.array_equal(L.tied_distributions(300, T.TIE_OFFSETS), T._tied_distributions(300))


@pytest.mark.parametrize('V', sorted(L.TIED_LENGTHS))
def test_tied_lists_hold_ties(V):
    P, offsets, lists = L.tied_case(V)
    assert set(np.diff(offsets).tolist()) == {1, 2}
    assert np.all(P > 0)
    for q, lst in enumerate(lists):
        joint = L.log_joint64(P[offsets[q]:offsets[q + 1]])
        assert len(np.unique(joint)) <= 25            # five levels per token, at most two tokens
        if len(lst) >= 64:
            assert L.in_tie_runs(joint[lst.astype(np.int64)]) >= len(lst) / 2.0, (q, len(lst))


def test_filter_full_ranking_against_a_brute_force_sort():
    rng = np.random.RandomState(5)
    V, Q = 40, 4
    score = rng.randint(0, 6, (Q, V)).astype(np.float64) / 8.0         # (few levels: ties)
    idx_full = np.stack([np.lexsort((np.arange(V), -row)) for row in score])
    score_full = np.take_along_axis(score, idx_full, axis=1)
    lists = [L.draw_list(rng, V, n) for n in (40, 1, 17, 0)]
    for k in (None, 1, 5, 100):
        got = L.filter_full_ranking(idx_full, score_full, lists, k)
        for q, lst in enumerate(lists):
            brute = sorted(lst.tolist(), key=lambda e: (-score[q, e], e))[:k]
            assert got[q][0].tolist() == brute
            assert np.array_equal(got[q][1], score[q, brute] if brute else np.zeros(0))
    at = np.array([0, 2, 2, 5])
    parts = L.split(at, np.arange(5), np.arange(5) * 0.5)
    assert [p[0].tolist() for p in parts] == [[0, 1], [], [2, 3, 4]]


def test_reversed_queries():
    P, offsets, lists = L.tied_case(300)
    Pr, offs_r, lists_r = L.reversed_queries(P, offsets, lists)
    Q = len(lists)
    for q in range(Q):
        r = Q - 1 - q
        assert np.array_equal(Pr[offs_r[r]:offs_r[r + 1]], P[offsets[q]:offsets[q + 1]]) and lists_r[r] is lists[q]


def test_callback_names_the_lists_and_reports_a_candidate_ranking_as_it_is():
    import types
    seen = []
    args = (types.SimpleNamespace(top=None), types.SimpleNamespace(), {}, None, lambda t, i, s: seen.append((t, i, s)))
    assert scoring.LogLinearCallback(*args).candidate_lists([{'topic_id': 'a'}]) is None
    cand = {'a': np.array([7, 3], dtype=np.int32)}
    cb = scoring.LogLinearCallback(*args, candidates=cand)
    got = cb.candidate_lists([{'topic_id': 'a'}, {'topic_id': 'b'}])
    assert got[0].tolist() == [7, 3] and got[1].size == 0
    idx, score = [np.array([7, 3]), np.zeros(0, np.int64)], [np.array([0.5, 0.25], np.float32), np.zeros(0, np.float32)]
    ranking = inference.QueryRanking(idx, score, [0.5, 0.5], [[0.5], [0.5]], [0, 0], k=None, candidates=True)
    cb.process_batch([[1], [2]], ranking, [{'topic_id': 'a'}, {'topic_id': 'b'}])
    assert [t for t, _, _ in seen] == ['a', 'b'] and seen[0][1] is idx[0] and seen[0][2] is score[0] and seen[1][1].size == 0
    assert cb.topic_projections['a'].tolist() == [0.5, 0.25]
