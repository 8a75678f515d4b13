"""-m gpu: the cosine scorer's bf16 prefilter on tables that sit AT its rounding-error bound (tests/score_bf16_cases.py;
tests/test_score_bf16_inputs_cpu.py proves what is claimed of them here).

`cut` rows: the exact top k lies between 1.08 and 2 bf16_delta below the k-th largest bf16 score, and no row of the call
is flagged -- so it is the cut `s^_(k) - 2 delta` of topk_from_groups_rescore itself that keeps them.  `flag` rows: the
exact top k never enters a candidate list and delta <= s^_(k) - T < 2 delta -- only the flag `s^_(k) - delta >= T + delta`
saves them.  A kernel that cuts at one delta, compares with T alone or uses half the delta fails here and passes every
Gaussian and every bf16-exact table.  Indices are compared for equality (the CPU proof shows the gaps), scores with the
1e-6 of check_topk_against_oracle, against the float64 oracle; the path a row took is read from sert_debug_scorer_counts."""
import functools

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import score_bf16_cases as B
from tests import test_gpu_score_contract as SC
from tests import util as U

pytestmark = pytest.mark.gpu

FUSED_CALLS, BF16_CALLS, CHUNKS, FLAGGED, DIRECT_ROWS, DEMOTED = range(6)


@functools.lru_cache(maxsize=None)
def _oracle(name, planting, k):
    """(idx, score) of the float64 oracle for the 4 adversarial queries of a planting, computed once."""
    case = B.build(name)
    E64 = case['E'].astype(np.float64)
    P64 = case['P_adv'][B.NUM_ADV * planting:B.NUM_ADV * (planting + 1)].astype(np.float64)
    ranked = [O.vectorspace_rank(p, E64, top=k) for p in P64]
    return np.stack([r[0] for r in ranked]), np.stack([r[1] for r in ranked])


def _check_call(name, planting, k, idx, val):
    """One call on B.queries(case, planting): the adversarial rows EQUAL the oracle's indices (which are the planted
    entities in their order), scores within 1e-6; the ordinary rows through check_topk_against_oracle."""
    case = B.build(name)
    want_idx, want_val = _oracle(name, planting, k)
    for j in range(B.NUM_ADV):
        pl = case['plant'][B.NUM_ADV * planting + j]
        assert np.array_equal(want_idx[j], pl['top']), (name, j, 'the oracle does not rank the planted set first')
        err = float(np.abs(val[j].astype(np.float64) - want_val[j]).max())
        lost = sorted(set(pl['top'].tolist()) - set(idx[j].tolist()))
        print(name, 'k', k, 'row', j, 'planted entities lost', len(lost), 'of them decoys instead',
              int(np.isin(idx[j], pl['decoys']).sum()), 'score err %.1e' % err)
        assert np.array_equal(idx[j], want_idx[j]), (name, k, 'row', j, 'lost', lost[:8], 'got', idx[j][:12].tolist(),
                                                     'want', want_idx[j][:12].tolist())
        assert err < 1e-6, (name, k, j, err)
    P = B.queries(case, planting)
    U.check_topk_against_oracle(case['E'], P[B.NUM_ADV:], idx[B.NUM_ADV:], val[B.NUM_ADV:], k)


def _k(name, planting=0):
    return B.CASES[name][1][planting][1]


@pytest.mark.parametrize('name', B.CUT_CASES)
def test_the_two_delta_cut_keeps_the_exact_top_k(hip_lib, name):
    """cut_d64 / cut_d36 (kp = 64, half a K chunk of padding) / cut_d300 (the pattern over all five K chunks of kp = 320),
    k = 10 and 100: one fused bf16 call, no row flagged, nothing demoted -- the cut alone produced the answer."""
    case, k = B.build(name), _k(name)
    sc = C.Scorer(case['E'])
    idx, val = [a.copy() for a in sc.topk(B.queries(case), k)]
    counts = sc.debug_path_counts()
    sc.close()
    print(name, 'path counts', counts)
    _check_call(name, 0, k, idx, val)
    assert counts[FUSED_CALLS] == 1 and counts[BF16_CALLS] == 1, counts
    assert counts[FLAGGED] == 0, counts
    assert counts[DIRECT_ROWS] == 0 and counts[DEMOTED] == 0, counts


@pytest.mark.parametrize('name', B.FLAG_CASES)
def test_a_row_without_the_two_delta_gap_is_flagged(hip_lib, name):
    """flag_d64 / flag_d300, k = 10: the sampled threshold is a decoy's score less than 2 delta (more than one delta) below
    s^_(k), the true top k is below it in bf16: every adversarial row must go to the materialising path."""
    case, k = B.build(name), _k(name)
    sc = C.Scorer(case['E'])
    idx, val = [a.copy() for a in sc.topk(B.queries(case), k)]
    counts = sc.debug_path_counts()
    sc.close()
    print(name, 'path counts', counts)
    assert counts[FUSED_CALLS] == 1 and counts[BF16_CALLS] == 1, counts
    _check_call(name, 0, k, idx, val)
    assert counts[FLAGGED] >= B.NUM_ADV, counts


def test_a_table_demoted_by_gapless_rows_answers_as_a_fresh_scorer(hip_lib):
    """demote_d64: 64 rows of the flag construction (the 4 flag queries, 16 times) -- more than a quarter flagged, the table
    loses its bf16 prefilter -- then the cut queries on the same scorer, now through the fp32 filter and rescore_topk_rows.
    Both calls answer as a fresh scorer does, bit for bit, and as the oracle."""
    name = 'demote_d64'
    case = B.build(name)
    (kind0, k), (kind1, k1) = B.CASES[name][1]
    assert (kind0, kind1) == ('flag', 'cut') and k == k1
    P_flag = np.tile(B.queries(case, 0)[:B.NUM_ADV], (16, 1))
    P_cut = B.queries(case, 1)
    sc = C.Scorer(case['E'])
    idx0, val0 = [a.copy() for a in sc.topk(P_flag, k)]
    counts = sc.debug_path_counts()
    print(name, 'after the flag block', counts)
    assert counts[DEMOTED] == 1 and counts[BF16_CALLS] == 1 and counts[FLAGGED] == 64, counts
    idx1, val1 = [a.copy() for a in sc.topk(P_cut, k)]
    counts = sc.debug_path_counts()
    print(name, 'after the cut block', counts)
    assert counts[FUSED_CALLS] == 2 and counts[BF16_CALLS] == 1 and counts[DEMOTED] == 1, counts      # (filtered in fp32)
    sc.close()
    want_idx, want_val = _oracle(name, 0, k)
    for j in range(B.NUM_ADV):
        assert np.array_equal(want_idx[j], case['plant'][j]['top'])
    for rep in range(16):
        rows = slice(B.NUM_ADV * rep, B.NUM_ADV * (rep + 1))
        assert np.array_equal(idx0[rows], want_idx), rep
        assert np.abs(val0[rows].astype(np.float64) - want_val).max() < 1e-6
    _check_call(name, 1, k, idx1, val1)
    for P, (idx, val) in ((P_flag, (idx0, val0)), (P_cut, (idx1, val1))):
        fresh = C.Scorer(case['E'])
        fidx, fval = fresh.topk(P, k)
        assert np.array_equal(idx, fidx) and U.same_bits(val, fval)
        fresh.close()


@functools.lru_cache(maxsize=None)
def _host_call(name):
    """The host-array call of a case on a fresh scorer: what the other routes must equal bit for bit."""
    case, k = B.build(name), _k(name)
    sc = C.Scorer(case['E'])
    idx, val = [a.copy() for a in sc.topk(B.queries(case), k)]
    sc.close()
    return idx, val


@pytest.mark.parametrize('name', ['cut_d64_k10', 'cut_d64_k100'])
def test_rank_at_a_depth_up_to_1024_is_the_same_call(hip_lib, name):
    """Scorer.rank(P, k) and sert_scorer_rank itself at k <= 1024 (RANK_TOPK: the fused bf16 path chunk by chunk)."""
    case, k = B.build(name), _k(name)
    P = np.ascontiguousarray(B.queries(case))
    idx, val = _host_call(name)
    _check_call(name, 0, k, idx, val)
    sc = C.Scorer(case['E'])
    ridx, rval = [a.copy() for a in sc.rank(P, k)]
    assert np.array_equal(ridx, idx) and U.same_bits(rval, val)
    lidx, lval = np.empty((P.shape[0], k), dtype=np.int32), np.empty((P.shape[0], k), dtype=np.float32)
    C.check(sc._lib.sert_scorer_rank(sc._h, P.ctypes.data, P.shape[0], k, lidx.ctypes.data, lval.ctypes.data))
    counts, rank_counts = sc.debug_path_counts(), sc.debug_rank_counts()
    sc.close()
    print(name, 'path counts', counts, 'rank counts', rank_counts)
    assert np.array_equal(lidx, idx) and U.same_bits(lval, val)
    assert rank_counts[0] == 1 and rank_counts[2] == P.shape[0], rank_counts
    assert counts[FUSED_CALLS] == 2 and counts[BF16_CALLS] == 2 and counts[FLAGGED] == 0, counts


def test_device_arrays_take_the_same_path_as_host_arrays(hip_lib):
    """scorer_topk_io(dev = true), as sert_reval_run feeds it: a vectorspace engine whose entity table is cut_d64_k10's, one
    token per topic, word row atanh(query), W = 1, b = 0 -- its projection tanh(atanh(p)) is the query to a few ulp, far
    inside what keeps the rounding pattern (2^-12).  The ranking the evaluator computes on device-resident projections
    equals, bit for bit, the host-array call on the same projections, and the adversarial rows are the planted sets."""
    name = 'cut_d64_k10'
    case, k = B.build(name), _k(name)
    d = case['d']
    Pn = B.normalize32(B.queries(case))
    p = dict(Rw=np.arctanh(Pn.astype(np.float64)).astype(np.float32), Re=case['E'], W=np.eye(d, dtype=np.float32),
             b=np.zeros(d, dtype=np.float32), X=np.zeros((1, 1), dtype=np.uint8))
    eng = U.vs_engine(p, Pn.shape[0], 1, 1, 0.0)
    lists = [[t] for t in range(Pn.shape[0])]
    none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    ev = C.RetrievalEval(eng, lists, [none] * len(lists), [1.0] * len(lists), [0] * len(lists), k)
    _, status, idx, val = ev.run(return_ranking=True)
    ev.close()
    proj = eng.predict_project(p['Rw'])
    eng.close()
    assert np.all(status == C.LL_STATUS_DEVICE)
    assert np.abs(B.normalize32(proj).astype(np.float64) - Pn).max() <= 8 * 2.0 ** -24, 'the projection is not the query'
    sc = C.Scorer(case['E'])
    hidx, hval = [a.copy() for a in sc.topk(proj, k)]
    counts = sc.debug_path_counts()
    sc.close()
    assert counts[FUSED_CALLS] == 1 and counts[BF16_CALLS] == 1 and counts[FLAGGED] == 0, counts
    assert np.array_equal(idx, hidx) and U.same_bits(val, hval)
    for j in range(B.NUM_ADV):
        assert np.array_equal(idx[j], case['plant'][j]['top']), j
    fidx, fval = _host_call(name)            # the queries themselves: the same entities, scores a few ulp apart
    assert np.array_equal(idx[:B.NUM_ADV], fidx[:B.NUM_ADV]) and np.abs(val - fval).max() < 1e-6


def test_the_materialising_path_returns_the_same_bits(hip_lib):
    """SERT_SCORE_MATERIALISE=1 in a child process (the knob is read once per process): cut_d64 at k = 10 and k = 100."""
    names = ['cut_d64_k10', 'cut_d64_k100']
    jobs = [(B.build(n)['E'], [(B.queries(B.build(n)), _k(n))]) for n in names]
    for n, (((ridx, rval),), (rcounts,)) in zip(names, SC.run_jobs_under('materialise', jobs)):
        assert rcounts[FUSED_CALLS] == 0 and rcounts[DIRECT_ROWS] == 2 * B.NUM_ADV, rcounts
        idx, val = _host_call(n)
        assert np.array_equal(idx, ridx) and U.same_bits(val, rval), n
        _check_call(n, 0, _k(n), ridx, rval)
