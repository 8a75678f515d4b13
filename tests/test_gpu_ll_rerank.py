"""-m gpu: per-query candidate lists ranked with the loglinear model on the device (sert_ll_rank_candidates, its debug call,
LogLinearPredictFn.rank_queries(candidates=...), the BatchedWordRanker front end with LogLinearCallback(candidates=...) and
bin/query.py --candidates).  The contract: a DEVICE query's result is the full ranking (sert_ll_rank_queries, k = -1) of that
query restricted to its list and cut to its head -- same entities, same order, same score BITS; entropies and status are the
full call's, bit for bit.  "Same" below means that (U.same_bits for floats) unless a bound is stated.  Which kernel ranked a
list is read from sert_debug_ll_rerank_counts.  tests/ll_rerank_cases.py builds the inputs and holds the expectation
(filter_full_ranking), tests/test_ll_rerank_inputs_cpu.py checks them."""
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import inference, models, scoring
from tests import ll_rerank_cases as L
from tests import util as U
from tests.test_gpu_ll_rank import GOLDEN, check_ranking, host_log_joint, tolerances

pytestmark = pytest.mark.gpu

CALLS, CHUNKS, LDS_LISTS, SLAB_LISTS, EMPTY = range(5)
DEVICE, HOST = C.LL_STATUS_DEVICE, C.LL_STATUS_HOST


def _counted(fn):
    before = C.debug_ll_rerank_counts()
    out = fn()
    return out, [a - b for a, b in zip(C.debug_ll_rerank_counts(), before)]


def _same_lists(got, want, what=''):
    assert len(got) == len(want), what
    for q, ((gi, gs), (wi, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(gi, dtype=np.int64), np.asarray(wi, dtype=np.int64)), (what, q)
        assert np.asarray(gs).dtype == np.float32 and U.same_bits(gs, ws), (what, q)


def _expected_counts(lists):
    n = [len(np.unique(x)) for x in lists]
    return [sum(1 <= x <= L.LDS_MAX for x in n), sum(x > L.LDS_MAX for x in n), sum(x == 0 for x in n)]


# ---- 1. the reference's recorded vectors -----------------------------------------------------------------------------------

@pytest.mark.parametrize('i', [0, 1, 2])
def test_golden_vectors(hip_lib, i):
    """ll_in_i (V_e = 25) once per list (all 25, one entity, every other entity, none): the debug call against
    debug_ll_rank_distributions(k=None) filtered, and against the reference's ll_idx / ll_val restricted to the list under
    check_ranking's rule with the tolerances tests/test_gpu_ll_rank.py derives."""
    g = np.load(GOLDEN)
    P = g['ll_in_%d' % i].astype(np.float32)
    T, V = P.shape
    lists = L.golden_lists(V)
    P4 = np.tile(P, (len(lists), 1))
    offsets = np.arange(len(lists) + 1, dtype=np.int64) * T
    idx_f, score_f, jh_f, th_f, status_f, _ = C.debug_ll_rank_distributions(P4, offsets, None)
    assert np.all(status_f == DEVICE)
    s_h = np.empty(V)
    s_h[g['ll_idx_%d' % i]] = g['ll_val_%d' % i]
    Lj, S = host_log_joint(P)
    rtol, atol = tolerances(T, Lj, S)
    for k in L.GOLDEN_K:
        at, idx, score, jh, th, status, _ = C.debug_ll_rank_candidates_distributions(P4, offsets, lists, k)
        got = L.split(at, idx, score)
        _same_lists(got, L.filter_full_ranking(idx_f, score_f, lists, k), 'k=%r' % (k,))
        assert U.same_bits(jh, jh_f) and U.same_bits(th, th_f) and np.array_equal(status, status_f)
        np.testing.assert_allclose(th[:T], g['ll_entropies_%d' % i], rtol=1e-5)
        for lst, (gi, gs) in zip(lists, got):
            assert len(gi) == (len(lst) if k is None else min(k, len(lst)))
            if len(lst):
                check_ranking(np.searchsorted(lst, gi), gs, s_h[lst.astype(np.int64)], rtol, atol, k=k)


# ---- 2. ties, every kernel, every edge -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tied_full(V):
    P, offsets, _ = L.tied_case(V)
    return C.debug_ll_rank_distributions(P, offsets, None)


@pytest.mark.parametrize('k', L.K_VALUES)
@pytest.mark.parametrize('V', sorted(L.TIED_LENGTHS))
def test_tied_lists_on_every_kernel(hip_lib, V, k):
    P, offsets, lists = L.tied_case(V)
    Q = len(lists)
    idx_f, score_f, jh_f, th_f, status_f, _ = _tied_full(V)
    assert np.all(status_f == DEVICE)
    (at, idx, score, jh, th, status, _), added = _counted(lambda: C.debug_ll_rank_candidates_distributions(P, offsets, lists, k))
    assert at.tolist() == C.ranked_indptr(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), k).tolist()
    got = L.split(at, idx, score)
    _same_lists(got, L.filter_full_ranking(idx_f, score_f, lists, k), 'V=%d k=%r' % (V, k))
    assert U.same_bits(jh, jh_f) and U.same_bits(th, th_f) and np.array_equal(status, status_f)
    # each list went to the kernel its length calls for
    assert added == [1, 1] + _expected_counts(lists), added
    for q, (gi, gs) in enumerate(got):
        bits = gs.view(np.uint32)
        same = bits[1:] == bits[:-1]
        assert np.all(gs[1:] <= gs[:-1]) and np.all(gi[1:][same] > gi[:-1][same]), q
        if k is None and len(lists[q]) >= 64:
            assert L.in_tie_runs(bits) >= len(lists[q]) / 2.0, q
    # the same queries, last first
    Pr, offs_r, lists_r = L.reversed_queries(P, offsets, lists)
    at_r, idx_r, score_r, jh_r, th_r, status_r, _ = C.debug_ll_rank_candidates_distributions(Pr, offs_r, lists_r, k)
    _same_lists(L.split(at_r, idx_r, score_r)[::-1], got, 'reversed')
    assert U.same_bits(jh_r[::-1], jh) and np.array_equal(status_r[::-1], status)
    for q in range(Q):
        r = Q - 1 - q
        assert U.same_bits(th_r[offs_r[r]:offs_r[r + 1]], th[offsets[q]:offsets[q + 1]])


# ---- 3. the engine call ----------------------------------------------------------------------------------------------------

def _predict_fn(case, window=4):
    return models.LogLinearPredictFn(R_w=case['Rw'], W=case['W'], b=case['b'], window_size=window)


def _ranking_lists(r):
    assert r.candidates is True
    return [(r.idx[q], r.score[q]) for q in range(len(r))]


def _same_extras(r, full):
    assert U.same_bits(r.joint_entropy, full.joint_entropy) and np.array_equal(r.status, full.status)
    for a, b in zip(r.token_entropy, full.token_entropy):
        assert U.same_bits(a, b)


@pytest.mark.parametrize('name', ['small', 'slab'])
def test_engine_call_matches_the_full_ranking_filtered(hip_lib, monkeypatch, name):
    """rank_queries(candidates=...) against rank_queries(k=None) filtered, for the whole list and two heads; then under a
    SERT_LL_RANK_BUDGET that holds the one slab of distinct-token rows (50 and 12 queries of at most six tokens: fewer than
    1024 distinct words) and a quarter of what the call's queries need behind it -- joint rows at 4 V_e bytes, candidates at 4
    bytes, results at 8 -- so that no three chunks can hold them all: at least three chunks, read from the counters, and the
    same results."""
    case = L.engine_case(name)
    fn = _predict_fn(case)
    queries, lists = case['queries'], case['lists']
    Ve, d = case['W'].shape[1], case['W'].shape[0]
    full = fn.rank_queries(queries)
    assert np.all(full.status == DEVICE)
    base = {}
    for k in (None, 7, 3000):
        r, added = _counted(lambda: fn.rank_queries(queries, k=k, candidates=lists))
        assert r.k == k and added == [1, 1] + _expected_counts(lists), added
        base[k] = _ranking_lists(r)
        _same_lists(base[k], L.filter_full_ranking(full.idx, full.score, lists, k), '%s k=%r' % (name, k))
        _same_extras(r, full)
        assert all(i.dtype == np.int64 for i, _ in base[k])
    lengths = [len(np.unique(x)) for x in lists]
    front = 1024 * (d + Ve + 2) * 4

    def chunks_of(budget, k):
        """The plan restated for lists within LDS: a chunk takes the next query while rows, joint rows, candidates and results fit."""
        n, pairs, outs, chunks = 0, 0, 0, 1
        for length in lengths:
            add = (1, length, length if k is None else min(k, length))
            if n and front + (n + add[0]) * Ve * 4 + (pairs + add[1]) * 4 + (outs + add[2]) * 8 > budget:
                n, pairs, outs, chunks = 0, 0, 0, chunks + 1
            n, pairs, outs = n + add[0], pairs + add[1], outs + add[2]
        return chunks

    for k in (None, 7):
        behind = sum(Ve * 4 + n * 4 + (n if k is None else min(k, n)) * 8 for n in lengths)
        for budget in (front + behind // 4, front + behind // 3 + 1000):
            monkeypatch.setenv('SERT_LL_RANK_BUDGET', str(budget))
            r, added = _counted(lambda: fn.rank_queries(queries, k=k, candidates=lists))
            assert added[CALLS] == 1 and added[CHUNKS] >= 3 and added[2:] == _expected_counts(lists), added
            if max(lengths) <= L.LDS_MAX:
                assert added[CHUNKS] == chunks_of(budget, k), (added, budget)
            _same_lists(_ranking_lists(r), base[k], '%s k=%r, %d chunks' % (name, k, added[CHUNKS]))
            _same_extras(r, full)


# ---- 4. a query the device cannot rank -------------------------------------------------------------------------------------

def test_host_query_between_two_ordinary_ones(hip_lib):
    case = L.host_case()
    fn = _predict_fn(case, case['window'])
    queries, lists = case['queries'], case['lists']
    full = fn.rank_queries(queries)
    r = fn.rank_queries(queries, candidates=lists)
    assert list(r.status) == [DEVICE, HOST, DEVICE] and list(full.status) == [DEVICE, HOST, DEVICE]
    # the HOST query: its list in entity order, score 0 (not meaningful: the caller takes the host path)
    assert np.array_equal(r.idx[1], lists[1]) and np.all(r.score[1] == 0) and np.isnan(r.joint_entropy[1])
    without = fn.rank_queries([queries[0], queries[2]], candidates=[lists[0], lists[2]])
    assert list(without.status) == [DEVICE, DEVICE]
    want = L.filter_full_ranking(full.idx, full.score, lists)
    for q, w in ((0, 0), (2, 1)):
        _same_lists([(r.idx[q], r.score[q])], [(without.idx[w], without.score[w])], 'neighbour %d' % q)
        _same_lists([(r.idx[q], r.score[q])], [want[q]], 'neighbour %d against the full ranking' % q)
        assert U.same_bits(r.joint_entropy[q:q + 1], without.joint_entropy[w:w + 1])
        assert U.same_bits(r.token_entropy[q], without.token_entropy[w])
    assert U.same_bits(r.token_entropy[1], full.token_entropy[1])


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------

def test_argument_faults(hip_lib):
    case = L.engine_case('small')
    fn = _predict_fn(case)
    fn.rank_queries(case['queries'][:2])              # (creates the engine)
    eng, lib = fn._engine, C.load()
    Vw, Ve = case['Rw'].shape[0], case['W'].shape[1]
    good = dict(tokens=[3, 4, 5, 6], offsets=[0, 1, 3, 4], indptr=[0, 2, 2, 5], ents=[4, 9, 0, 7, Ve - 1], k=-1)
    outs = dict(idx=np.empty(8, np.int32), score=np.empty(8, np.float32), jh=np.empty(3, np.float32), th=np.empty(4, np.float32),
                status=np.empty(3, np.int32))

    def call(handle=None, **kw):
        a = dict(good, **outs)
        a.update(kw)
        arr = {name: (None if a[name] is None else np.asarray(a[name], dtype=dt))
               for name, dt in (('tokens', np.int32), ('offsets', np.int64), ('indptr', np.int64), ('ents', np.int32))}
        rc = lib.sert_ll_rank_candidates(eng._h if handle is None else handle, C._addr(arr['tokens']), C._addr(arr['offsets']), 3,
                                         C._addr(arr['indptr']), C._addr(arr['ents']), a['k'], C._addr(a['idx']),
                                         C._addr(a['score']), C._addr(a['jh']), C._addr(a['th']), C._addr(a['status']))
        return rc, lib.sert_last_error().decode()

    p = U.make_vs_problem(1, 64, 4, 2, 50, 20, 8, 8)
    vs = U.vs_engine(p, 16, 4, 2, 0.0)
    before = C.debug_ll_rerank_counts()
    faults = [(dict(indptr=[1, 2, 2, 5]), 'cand_indptr[0] must be 0'),
              (dict(indptr=[0, 3, 2, 5]), 'cand_indptr decreases'),
              (dict(ents=[4, 9, 0, 7, Ve]), 'out of range'),
              (dict(ents=[4, -1, 0, 7, 8]), 'out of range'),
              (dict(ents=[9, 4, 0, 7, 8]), 'not strictly ascending'),
              (dict(ents=[4, 4, 0, 7, 8]), 'not strictly ascending'),
              (dict(k=0), 'k must be -1 (the whole list) or positive'),
              (dict(k=-2), 'k must be -1 (the whole list) or positive'),
              (dict(handle=vs._h), 'ranks with the loglinear model'),
              (dict(tokens=[3, Vw, 5, 6]), 'token id out of range'),
              (dict(tokens=[3, -1, 5, 6]), 'token id out of range'),
              (dict(offsets=[1, 2, 3, 4]), 'offsets[0] must be 0'),
              (dict(offsets=[0, 1, 1, 4]), 'at least one token')]
    faults += [({name: None}, 'null argument') for name in ('tokens', 'offsets', 'indptr', 'ents', 'idx', 'score', 'jh', 'th', 'status')]
    for kw, text in faults:
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw, msg)
        # nothing was launched or counted, and a good call right behind the refused one succeeds
        assert C.debug_ll_rerank_counts() == before, kw
        rc, msg = call()
        assert rc == 0, (kw, msg)
        before = C.debug_ll_rerank_counts()
    assert lib.sert_ll_rank_candidates(None, None, None, 3, None, None, -1, None, None, None, None, None) != 0
    vs.close()
    # the good call's results are the wrapper's
    at, idx, score, jh, th, status, _ = eng.ll_rank_candidates([[3], [4, 5], [6]], [[4, 9], [], [0, 7, Ve - 1]])
    assert at.tolist() == [0, 2, 2, 5] and np.array_equal(outs['idx'][:5], idx) and U.same_bits(outs['score'][:5], score)
    assert U.same_bits(outs['jh'], jh) and U.same_bits(outs['th'], th) and np.array_equal(outs['status'], status)
    for k in (0, -1):
        with pytest.raises(C.SertError, match='k must be'):
            eng.ll_rank_candidates([[3]], [[1]], k)
    with pytest.raises(C.SertError, match='candidate lists for'):
        eng.ll_rank_candidates([[3], [4]], [[1]])
    # the debug call refuses the same CSR faults
    P = np.full((2, 8), 0.125, np.float32)
    with pytest.raises(C.SertError, match='out of range'):
        C.debug_ll_rank_candidates_distributions(P, [0, 1, 2], [[1], [8]])


# ---- 6. the query front end ------------------------------------------------------------------------------------------------

class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, topic_id, idx, score):
        self.calls.append((topic_id, np.array(idx), np.array(score)))


def test_front_end_makes_the_calls_of_the_filtered_full_ranking(hip_lib):
    """BatchedWordRanker + LogLinearCallback(candidates=...) against the route without the candidate call, spelled out:
    rank_queries(k=None), then np.isin per topic.  The same rank_callback calls (topic order, entity ids, score bits) and the
    same _debug text, from exactly one candidate call; a topic without a list gets an empty ranking; the HOST query falls
    back to the per-token path and still reports a filtered ranking."""
    case = L.host_case()
    fn = _predict_fn(case, case['window'])
    queries = case['queries'] + [case['queries'][0]]
    topics = ['T%d' % q for q in range(len(queries))]
    cand = {t: lst[::-1].copy() for t, lst in zip(topics[:3], case['lists'])}          # (unsorted: the wrapper cleans them; T3 has none)
    tokens = {i: 'w%d' % i for i in range(case['Rw'].shape[0])}
    Vw = case['Rw'].shape[0]

    # the route without the candidate call
    rec_p, dbg_p = _Recorder(), io.StringIO()
    cb_p = scoring.LogLinearCallback(None, None, tokens, dbg_p, rec_p, candidates=cand)
    full = fn.rank_queries(queries, k=None)
    front = inference.BatchedWordRanker(fn, case['batch'], case['window'], np.min_scalar_type(Vw - 1), cb_p)
    full.distributions_of = lambda q: front._distributions(queries[q])
    assert full.candidates is False
    cb_p.process_batch(queries, full, [{'topic_id': t} for t in topics])
    # ... whose device-ranked topics are the full ranking through np.isin
    for q in (0, 2, 3):
        keep = np.isin(full.idx[q], cand.get(topics[q], np.zeros(0, np.int64)))
        assert rec_p.calls[q][0] == topics[q] and np.array_equal(rec_p.calls[q][1], full.idx[q][keep])
        assert U.same_bits(rec_p.calls[q][2], full.score[q][keep])

    rec, dbg = _Recorder(), io.StringIO()
    cb = scoring.LogLinearCallback(None, None, tokens, dbg, rec, candidates=cand)
    fe = inference.create(fn, case['Rw'], case['batch'], case['window'], Vw, cb, batched=True)
    assert isinstance(fe, inference.BatchedWordRanker)
    for toks, t in zip(queries, topics):
        fe.submit(toks, topic_id=t)
    _, added = _counted(fe.process)
    assert added[CALLS] == 1 and added[EMPTY] == 1 and added[LDS_LISTS] == 3, added
    assert [c[0] for c in rec.calls] == topics
    for (t, idx, score), (tp, idx_p, score_p) in zip(rec.calls, rec_p.calls):
        assert t == tp and idx.dtype == idx_p.dtype == np.int64 and np.array_equal(idx, idx_p), t
        assert score.dtype == score_p.dtype and np.array_equal(score.view(np.uint32), score_p.view(np.uint32)), t
    assert rec.calls[3][1].size == 0                                    # no list: an empty ranking
    assert len(rec.calls[1][1]) == len(case['lists'][1])                # the HOST query: every candidate reported
    assert sorted(rec.calls[1][1].tolist()) == case['lists'][1].tolist()
    assert dbg.getvalue() == dbg_p.getvalue() and dbg.getvalue().count('\n') == 4
    # a device-ranked candidate query keeps its ranked scores, in rank order
    assert U.same_bits(cb.topic_projections['T0'], rec.calls[0][2])


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------

_COUNTING_CLI = """
import runpy, sys
from sert_amd import _capi
sys.argv = sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name='__main__')
except SystemExit as e:
    assert not e.code, e.code
print('LL_RERANK_COUNTS', ' '.join(str(c) for c in _capi.debug_ll_rerank_counts()))
"""


def _run_lines(path):
    with io.open(path, encoding='utf8') as f:
        return [line.split() for line in f if line.strip()]


def test_cli_candidates_take_the_candidate_call(hip_lib, tmp_path):
    """bin/query.py --candidates on the tiny loglinear corpus: the candidate call ranked the lists (the counters, printed by
    the process that ran the CLI), and _ef is the full batched run filtered, line for line; _debug is the full run's for the
    topics that have a list."""
    from tests.test_gpu_models import _write_tiny_corpus
    _write_tiny_corpus(tmp_path, 'loglinear')
    env = dict(os.environ, PYTHONPATH=U.ROOT)
    subprocess.check_call([sys.executable, os.path.join(U.ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'),
                           '--meta', str(tmp_path / 'meta'), '--type', 'loglinear', '--iterations', '40', '--batch_size', '32',
                           '--word_representation_size', '16', '--model_output', str(tmp_path / 'model'),
                           '--seed', '1', '--loglevel', 'WARNING', '--regularization_lambda', '0.0'], env=env)
    last = sorted((f for f in os.listdir(str(tmp_path)) if f.startswith('model_')),
                  key=lambda f: int(f.split('_')[1].split('.')[0]))[-1]

    def query(tag, *extra):
        out = subprocess.run([sys.executable, '-c', _COUNTING_CLI, os.path.join(U.ROOT, 'bin', 'query.py'), '--meta',
                              str(tmp_path / 'meta'), '--model', str(tmp_path / last), '--topics', str(tmp_path / 'topics'),
                              '--run_out', str(tmp_path / ('run_' + tag)), '--loglevel', 'WARNING'] + list(extra), env=env,
                             stdout=subprocess.PIPE, check=True).stdout.decode()
        counts = [line.split()[1:] for line in out.splitlines() if line.startswith('LL_RERANK_COUNTS')]
        assert len(counts) == 1
        with io.open(str(tmp_path / ('run_%s_debug' % tag)), encoding='utf8') as f:
            debug = f.read().splitlines()
        return _run_lines(str(tmp_path / ('run_%s_ef' % tag))), debug, [int(c) for c in counts[0]]

    full, debug_full, counts_full = query('full')
    assert counts_full == [0, 0, 0, 0, 0]
    no_list = '5'
    picked = [f for f in full[::3] if f[0] != no_list]
    assert any(f[0] == no_list for f in full[::3]) and len(set(f[0] for f in picked)) >= 2
    with io.open(str(tmp_path / 'first_stage'), 'w', encoding='utf8') as f:
        for fields in picked:
            f.write(u' '.join(fields) + u'\n')
    cand, debug_cand, counts = query('cand', '--candidates', str(tmp_path / 'first_stage'))
    listed = set(f[0] for f in picked)
    assert counts[CALLS] == 1 and counts[LDS_LISTS] == len(listed) and counts[SLAB_LISTS] == 0 and counts[EMPTY] == 0, counts
    want = set((f[0], f[2]) for f in picked)
    keep = [(f[0], f[2], f[4]) for f in full if (f[0], f[2]) in want]
    assert [(f[0], f[2], f[4]) for f in cand] == keep and len(keep) == len(want)
    assert debug_cand == [line for line in debug_full if line.split()[1] in listed] and len(debug_cand) == len(listed)
