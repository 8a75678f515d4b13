"""GPU: the batched loglinear ranking (sert_ll_rank_queries, LogLinearPredictFn.rank_queries,
LogLinearCallback.process_batch, the BatchedWordRanker front end and bin/query.py's default loglinear path) against the
reference's recorded outputs and against today's host path (WordBatcher + predict_fn + LogLinearCallback.process).

Comparison rule (check_ranking): device scores s_d in device order against reference scores s_h indexed by entity --
idx_d is a permutation of V_e (or k distinct indices), |s_d - s_h| <= rtol max(s_d, s_h) + atol for every ranked entity,
and s_h[idx_d] is non-increasing within that tolerance.  The order must therefore agree wherever two reference scores
differ by more than the tolerance; exact ties (runs of zeros included) may come in any order.  The tolerances are derived:
  rtol = 4 (T + 2) max(1, max_e |L_e|) 2^-24   (a few ulp per log / exp, T half-ulps of |L| in the T-term sum, about 2 ulp
                                                from the normalisation sum; factor 4 = margin)
  atol = 4 2^-149 / S                           (a joint among the denormals keeps about one denormal ulp, divided by S)
  entropies: rtol = 1e-5                        (values in [0, 1], each of the V_e terms within 2 ulp)
"""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import inference, models, scoring

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_vectors.npz')


def tolerances(T, L, S):
    """(rtol, atol) of the comparison rule for a query of T tokens with log-joint L (V_e,) and joint sum S."""
    rtol = 4.0 * (T + 2) * max(1.0, float(np.max(np.abs(L)))) * 2.0 ** -24
    atol = 4.0 * 2.0 ** -149 / S
    return rtol, atol


def check_ranking(idx_d, s_d, s_h, rtol, atol, k=None):
    """The comparison rule; with k, also: the device's i-th score matches the reference's i-th best."""
    idx_d = np.asarray(idx_d, dtype=np.int64)
    s_d = np.asarray(s_d, dtype=np.float64)
    s_h = np.asarray(s_h, dtype=np.float64)
    V = s_h.size
    if k is None:
        assert np.array_equal(np.sort(idx_d), np.arange(V))
    else:
        assert idx_d.size == min(k, V) and np.unique(idx_d).size == idx_d.size and idx_d.min() >= 0 and idx_d.max() < V
    at = s_h[idx_d]
    err = np.abs(s_d - at) - (rtol * np.maximum(s_d, at) + atol)
    assert err.max() <= 0, (err.max(), int(err.argmax()))
    step = at[1:] - at[:-1] - (rtol * np.maximum(at[1:], at[:-1]) + atol)
    assert step.size == 0 or step.max() <= 0, (step.max(), int(step.argmax()))
    if k is not None:
        best = np.sort(s_h)[::-1][:idx_d.size]
        gap = np.abs(s_d - best) - (rtol * np.maximum(s_d, best) + atol)
        assert gap.max() <= 0, (gap.max(), int(gap.argmax()))


def host_log_joint(dist):
    """L_e = sum_t log p_te with log 0 -> 0 (inference.py:174), float64; and S = sum_e exp(L_e)."""
    d = np.asarray(dist, dtype=np.float64)
    L = np.where(d > 0, np.log(np.where(d > 0, d, 1.0)), 0.0).sum(axis=0)
    return L, float(np.exp(L).sum())


def test_pinned_to_the_reference_golden_vectors(hip_lib):
    """sert_debug_ll_rank_distributions on the reference's LogLinearCallback inputs ll_in_{0,1,2} (T = 1, 3, 6,
    V_e = 25): ranking and values against ll_idx / ll_val, token entropies against ll_entropies -- every ranking form."""
    g = np.load(GOLDEN)
    for i in range(3):
        P = g['ll_in_%d' % i].astype(np.float32)
        T, V = P.shape
        s_h = np.empty(V)
        s_h[g['ll_idx_%d' % i]] = g['ll_val_%d' % i]
        L, S = host_log_joint(P)
        rtol, atol = tolerances(T, L, S)
        print('golden %d: T=%d max|L|=%.3f S=%.3e rtol=%.3e' % (i, T, np.abs(L).max(), S, rtol))
        for k in (None, 1, 10, 25, 40):
            idx, score, jh, th, status, _ = C.debug_ll_rank_distributions(P, [0, T], k)
            assert status[0] == C.LL_STATUS_DEVICE
            check_ranking(idx[0], score[0], s_h, rtol, atol, k=k)
            np.testing.assert_allclose(th, g['ll_entropies_%d' % i], rtol=1e-5)


TIE_LEVELS = np.array([1.0, 2.0, 3.0, 5.0, 8.0], np.float32)
TIE_OFFSETS = [0, 1, 3, 5]       # three queries of one, two and two tokens


def _tied_distributions(V):
    """(5, V) token rows, every entry one of five positive levels, each row normalised in float32: entities that drew the
    same levels in a query's tokens go through the same float32 operations and share one joint value, bit for bit."""
    rng = np.random.RandomState(V)
    P = TIE_LEVELS[rng.randint(0, TIE_LEVELS.size, (TIE_OFFSETS[-1], V))]
    return P / P.sum(axis=1, dtype=np.float32, keepdims=True)


def _in_tie_runs(values):
    """How many elements of `values` share their value with another one."""
    _, counts = np.unique(values, return_counts=True)
    return int(counts[counts >= 2].sum())


@pytest.mark.parametrize('V', [300, 8200])
def test_full_ranking_orders_ties_by_entity_index(hip_lib, V):
    """The full ranking of joint rows (k = -1: the in-LDS sort at V = 300, the LSD passes at V = 8200) where whole runs of
    entities share one joint value: every query is ranked on the device, idx is a permutation, score is non-increasing,
    idx ascends inside every run of equal score bits, and score[i] is entity idx[i]'s joint value -- the joint row
    scattered back through idx holds the same values, bit for bit, as the row a call with the queries in reversed order
    gives.  The inputs put at least half of every query's entities into a tie (checked on the host path's float64 joint
    and on the device's scores); the scores also meet the comparison rule against the host path."""
    P = _tied_distributions(V)
    Q = len(TIE_OFFSETS) - 1
    idx, score, _, _, status, _ = C.debug_ll_rank_distributions(P, TIE_OFFSETS, None)
    # the same queries, last first
    rows = np.concatenate([np.arange(TIE_OFFSETS[q], TIE_OFFSETS[q + 1]) for q in reversed(range(Q))])
    offs_r = np.concatenate([[0], np.cumsum([TIE_OFFSETS[q + 1] - TIE_OFFSETS[q] for q in reversed(range(Q))])])
    idx_r, score_r, _, _, status_r, _ = C.debug_ll_rank_distributions(P[rows], offs_r, None)
    for q in range(Q):
        dist = P[TIE_OFFSETS[q]:TIE_OFFSETS[q + 1]]
        L, S = host_log_joint(dist)
        assert _in_tie_runs(L) >= V / 2, (q, _in_tie_runs(L))
        assert status[q] == C.LL_STATUS_DEVICE and status_r[Q - 1 - q] == C.LL_STATUS_DEVICE
        i, s = idx[q].astype(np.int64), score[q]
        bits = s.view(np.uint32)
        assert np.array_equal(np.sort(i), np.arange(V))
        assert np.all(s[1:] <= s[:-1])
        same = bits[1:] == bits[:-1]
        assert _in_tie_runs(bits) >= V / 2, (q, _in_tie_runs(bits))
        assert np.all(i[1:][same] > i[:-1][same])
        J = np.empty(V, np.float32)
        J[i] = s
        J_r = np.empty(V, np.float32)
        J_r[idx_r[Q - 1 - q].astype(np.int64)] = score_r[Q - 1 - q]
        assert np.array_equal(np.sort(J.view(np.uint32)), np.sort(J_r.view(np.uint32)))
        assert np.array_equal(bits, J_r.view(np.uint32)[i])
        check_ranking(i, s, np.exp(L) / S, *tolerances(dist.shape[0], L, S))


def _engine_problem(seed, Vw, Ve, d, Q, T_max):
    rng = np.random.RandomState(seed)
    Rw = rng.uniform(-0.5, 0.5, (Vw, d)).astype(np.float32)
    W = (rng.standard_normal((d, Ve)) * 0.25).astype(np.float32)
    b = np.zeros(Ve, np.float32)
    # a small vocabulary: words repeat across queries; drawn with replacement: and within them
    queries = [list(rng.randint(0, Vw, rng.randint(1, T_max + 1))) for _ in range(Q)]
    return models.LogLinearPredictFn(R_w=Rw, W=W, b=b, window_size=4), queries


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, topic_id, idx, score):
        self.calls.append((topic_id, np.array(idx), np.array(score)))


def _host_path(fn, queries, batch_size=64, window=4):
    """Today's path: WordBatcher -> predict_fn -> LogLinearCallback.process; also the per-query distributions."""
    rec, dists = _Recorder(), {}
    cb = scoring.LogLinearCallback(None, None, {}, None, rec)
    wb = inference.WordBatcher(fn, batch_size, window, np.min_scalar_type(fn.R_w.shape[0] - 1), cb)
    orig = cb.process

    def process(payload, distribution, topic_id):
        dists[topic_id] = distribution.copy()
        orig(payload, distribution, topic_id)
    cb.process = process
    for q, toks in enumerate(queries):
        wb.submit(toks, topic_id=q)
    wb.process()
    return {t: (i, s) for t, i, s in rec.calls}, dists


# (V_e, T_max): 25, 715, 4096 (in-LDS sort), 10 000 (above the 8192 LDS bound: the LSD counting-sort passes)
SHAPES = [(25, 12), (715, 8), (4096, 8), (10000, 6)]


@pytest.mark.parametrize('Ve,T_max', SHAPES)
@pytest.mark.parametrize('d', [64, 300])
def test_engine_path_matches_the_host_path(hip_lib, Ve, T_max, d):
    """rank_queries on a random inference-only engine against LogLinearPredictFn.__call__ + LogLinearCallback.process
    on the same weights: rankings and scores under the comparison rule for every k, token and joint entropies at rtol 1e-5
    (near-one-hot joints included: their float32 entropy keeps about one ulp of 1, so the device has to evaluate it as
    the host does -- kernels_ll_rank.h: np_entropy_norm2)."""
    fn, queries = _engine_problem(Ve + d, 400, Ve, d, 300, T_max)
    host, dists = _host_path(fn, queries)
    tiny = 0
    tol = {}
    for q, toks in enumerate(queries):
        L, S = host_log_joint(dists[q])
        tiny += S < 2.0 ** -107
        tol[q] = tolerances(len(toks), L, S)
    assert tiny <= 0.05 * len(queries), tiny
    ks = [None, 1, 100, 1024] + ([2000] if 1024 < 2000 < Ve else []) + [Ve + 5]
    from sert_amd import math_utils
    misses = []
    for k in ks:
        r = fn.rank_queries(queries, k=None if k is None else k)
        assert not np.any(r.status == inference.QueryRanking.HOST)
        for q, toks in enumerate(queries):
            order, vals = host[q]
            s_h = np.empty(Ve)
            s_h[order] = vals
            rtol, atol = tol[q]
            check_ranking(r.idx[q], r.score[q], s_h, rtol, atol, k=k)
            if k is None:
                ent = scoring.compute_normalised_entropy(dists[q], base=2)
                np.testing.assert_allclose(r.token_entropy[q], ent, rtol=1e-5)
                jh = math_utils.entropy(s_h.astype(np.float32), base=2, normalize=True)
                if abs(r.joint_entropy[q] - jh) > 1e-5 * abs(jh):
                    # (figures: device, host, and the float64 entropy of the host's own float32 joint)
                    misses.append((q, float(r.joint_entropy[q]), float(jh), float(math_utils.entropy(s_h, base=2, normalize=True))))
    for m in misses:
        print('joint entropy beyond rtol 1e-5: query %d device %.9g host %.9g host joint in float64 %.9g' % m)
    assert not misses, len(misses)


def _debug_lines(text):
    out = []
    for line in text.splitlines():
        m = re.match(r'^Topic (\S+) (\S+): (.*)$', line)
        assert m, line
        toks = re.findall(r"\('([^']*)', np\.float32\(([^)]*)\)\)", m.group(3))
        out.append((m.group(1), float(m.group(2)), [w for w, _ in toks], [float(h) for _, h in toks]))
    return out


def test_host_status_query_takes_the_unbatched_path_bit_for_bit(hip_lib):
    """A query whose joint underflows everywhere (60 tokens, V_e = 4096, near-flat logits: S = 0) gets status HOST and
    its callback output through the batched front end equals the --no_batch path's bit for bit; the other queries of the
    same run are ranked on the device."""
    rng = np.random.RandomState(3)
    Vw, Ve, d, B, n = 300, 4096, 64, 16, 8
    Rw = rng.uniform(-0.5, 0.5, (Vw, d)).astype(np.float32)
    W = (rng.standard_normal((d, Ve)) * 1e-3).astype(np.float32)
    fn = models.LogLinearPredictFn(R_w=Rw, W=W, b=np.zeros(Ve, np.float32), window_size=n)
    queries = [list(rng.randint(0, Vw, 3)), list(rng.randint(0, Vw, 60)), list(rng.randint(0, Vw, 2))]
    tokens = {i: 'w%d' % i for i in range(Vw)}
    outs = []
    for batched in (False, True):
        rec, dbg = _Recorder(), io.StringIO()
        cb = scoring.LogLinearCallback(None, None, tokens, dbg, rec)
        fe = inference.create(fn, Rw, B, n, Vw, cb, batched=batched)
        assert isinstance(fe, inference.BatchedWordRanker if batched else inference.WordBatcher)
        for q, toks in enumerate(queries):
            fe.submit(toks, topic_id='T%d' % q)
        fe.process()
        outs.append((rec.calls, dbg.getvalue().splitlines()))
    r = fn.rank_queries(queries)
    assert list(r.status) == [C.LL_STATUS_DEVICE, C.LL_STATUS_HOST, C.LL_STATUS_DEVICE]
    (h_calls, h_dbg), (b_calls, b_dbg) = outs
    assert [c[0] for c in h_calls] == [c[0] for c in b_calls]
    assert h_calls[1][0] == 'T1' and h_dbg[1] == b_dbg[1]
    assert np.array_equal(h_calls[1][1], b_calls[1][1])
    assert np.array_equal(h_calls[1][2], b_calls[1][2], equal_nan=True)


@pytest.mark.parametrize('Ve,k', [(715, None), (715, 100), (10000, None), (10000, 100), (10000, 3000)])
def test_results_are_deterministic_and_independent_of_the_call(hip_lib, monkeypatch, Ve, k):
    """Each query's result is bit-identical across two identical calls, across a call with the queries in reversed order
    and across a call whose chunk budget forces several chunks."""
    d = 64
    fn, queries = _engine_problem(7, 400, Ve, d, 200, 6)

    def run(qs):
        r = fn.rank_queries(qs, k=k)
        return [(r.idx[q], r.score[q], r.joint_entropy[q], r.token_entropy[q], r.status[q]) for q in range(len(qs))]

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    base = run(queries)
    assert all(same(x, y) for x, y in zip(base, run(queries)))
    assert all(same(x, y) for x, y in zip(base, run(queries[::-1])[::-1]))
    # one slab of gathered rows and distributions (1024 x (d + V_e + 2) floats; the queries use fewer than 1024 distinct
    # words) + room for 40 queries' joint rows, outputs and, when the ranking takes the counting-sort passes, their sort
    # scratch (four int32 arrays and the digit histograms, 20 bytes per element): 200 queries need five chunks
    kk = Ve if k is None else k
    csort = Ve > 8192 and kk > 1024
    per_query = Ve * 4 + kk * 8 + (Ve * 20 if csort else 0)
    monkeypatch.setenv('SERT_LL_RANK_BUDGET', str(1024 * (d + Ve + 2) * 4 + 40 * per_query))
    assert all(same(x, y) for x, y in zip(base, run(queries)))


def _parse_run(path):
    from sert_amd.utils import trec_utils
    with open(path) as f:
        return trec_utils.parse_run(f)


def test_cli_batched_loglinear_query_matches_no_batch(hip_lib, tmp_path):
    """bin/query.py on a trained loglinear model: the default (batched, device-ranked) run against --no_batch -- _ef and
    _ep under the comparison rule (plus half a unit of the 10th decimal the run files print), _debug entropies
    numerically."""
    from tests.test_gpu_models import _write_tiny_corpus
    _write_tiny_corpus(tmp_path, 'loglinear')
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'),
                           '--meta', str(tmp_path / 'meta'), '--type', 'loglinear', '--iterations', '40', '--batch_size',
                           '32', '--word_representation_size', '16', '--model_output', str(tmp_path / 'model'),
                           '--seed', '1', '--loglevel', 'WARNING', '--regularization_lambda', '0.0'], env=env)
    last = sorted((f for f in os.listdir(str(tmp_path)) if f.startswith('model_')),
                  key=lambda f: int(f.split('_')[1].split('.')[0]))[-1]
    for tag, extra in (('b', []), ('h', ['--no_batch'])):
        subprocess.check_call([sys.executable, os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'),
                               '--model', str(tmp_path / last), '--topics', str(tmp_path / 'topics'),
                               '--run_out', str(tmp_path / ('run_' + tag)), '--loglevel', 'WARNING'] + extra, env=env)
    # the tolerances need each topic's L and S: the reference path's per-token distributions of the trained model
    sys.path.insert(0, os.path.join(ROOT, 'bin'))
    import query as Qcli
    _, fn, _, _ = Qcli.load_model(str(tmp_path / last))
    _, words, _, _, _ = Qcli.load_meta(str(tmp_path / 'meta'))
    with open(str(tmp_path / 'topics')) as f:
        topics = [line.strip().split(';', 1) for line in f if line.strip()]
    tol = {}
    for tid, text in topics:
        ids = [words[w].id for w in text.split() if w in words]
        batch = np.zeros((8, fn.window_size), np.uint8)
        batch.reshape(-1)[:len(ids)] = ids
        dist = fn(batch).reshape(-1, fn.W.shape[1])[:len(ids)]
        L, S = host_log_joint(dist)
        rtol, atol = tolerances(len(ids), L, S)
        tol[tid] = (rtol, atol + 0.5e-10)
    run_b, run_h = _parse_run(str(tmp_path / 'run_b_ef')), _parse_run(str(tmp_path / 'run_h_ef'))
    assert sorted(run_b) == sorted(run_h)
    for tid in run_h:
        ents = sorted(e for _, e in run_h[tid])
        assert sorted(e for _, e in run_b[tid]) == ents
        pos = {e: i for i, e in enumerate(ents)}
        s_h = np.empty(len(ents))
        for s, e in run_h[tid]:
            s_h[pos[e]] = s
        check_ranking([pos[e] for _, e in run_b[tid]], [s for s, _ in run_b[tid]], s_h, *tol[tid])
    ep_b, ep_h = _parse_run(str(tmp_path / 'run_b_ep')), _parse_run(str(tmp_path / 'run_h_ep'))
    assert sorted(ep_b) == sorted(ep_h)
    for ent in ep_h:
        hb = dict((t, s) for s, t in ep_b[ent])
        for s, t in ep_h[ent]:
            rtol, atol = tol[t]
            assert abs(hb[t] - s) <= rtol * max(hb[t], s) + atol
    with open(str(tmp_path / 'run_b_debug')) as f:
        dbg_b = _debug_lines(f.read())
    with open(str(tmp_path / 'run_h_debug')) as f:
        dbg_h = _debug_lines(f.read())
    assert [x[0] for x in dbg_b] == [x[0] for x in dbg_h] and [x[2] for x in dbg_b] == [x[2] for x in dbg_h]
    for b, h in zip(dbg_b, dbg_h):
        np.testing.assert_allclose(b[1], h[1], rtol=1e-5)
        np.testing.assert_allclose(b[3], h[3], rtol=1e-5)
