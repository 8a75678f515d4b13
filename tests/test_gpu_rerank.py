"""-m gpu: cosines and rankings of per-query candidate lists on the device (sert_scorer_pairs, sert_scorer_rank_candidates;
DESIGN.md, "Re-ranking candidate lists on the device").  Every comparison of indices is exact and every comparison of values
bit for bit (U.same_bits) unless a bound is stated; which kernel ranked a list is read from sert_debug_scorer_rerank_counts.
tests/rerank_cases.py builds the inputs, tests/test_rerank_inputs_cpu.py checks them."""
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import scoring
from tests import rerank_cases as R
from tests import util as U

pytestmark = pytest.mark.gpu

CALLS, CHUNKS, LDS_QUERIES, SLAB_QUERIES, PAIRS, EMPTY = range(6)


def _counted(sc, fn):
    before = sc.debug_rerank_counts()
    out = fn()
    return out, [a - b for a, b in zip(sc.debug_rerank_counts(), before)]


def _ranked(sc, P, lists, k=None):
    return R.split(*sc.rank_candidates(P, lists, k))


def _pair_cosines(sc, P, lists):
    indptr, cos = sc.score_pairs(P, lists, raw=True)
    return [cos[a:b] for a, b in zip(indptr[:-1], indptr[1:])]


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for q, ((idx, val), (widx, wval)) in enumerate(zip(got, want)):
        assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == widx.shape, (what, q, idx.shape, widx.shape)
        assert np.array_equal(idx, widx), (what, q, idx[:12].tolist(), 'want', widx[:12].tolist())
        assert U.same_bits(val, wval), (what, q, 'values differ in their bits')


def _check_against_pair_cosines(sc, P, lists, what):
    """The ranking of every list is rank_order of that list's pair cosines, the values (cos + 1) / 2 of them."""
    cos = _pair_cosines(sc, P, lists)
    got = _ranked(sc, P, lists)
    _same_lists(got, [R.expected_ranking(c, lst) for c, lst in zip(cos, lists)], what)
    return got, cos


# ---- 1. exact problems -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', R.EXACT_NAMES)
def test_exact_problems(hip_lib, name):
    case = R.exact_case(name)
    sc = C.Scorer(case['E'])
    got, added = _counted(sc, lambda: _ranked(sc, case['P'], case['lists']))
    _same_lists(got, case['want'], name)
    lengths = case['lengths']
    assert added[CALLS] == 1 and added[EMPTY] == 1 and added[PAIRS] == sum(lengths), added
    assert added[LDS_QUERIES] == sum(0 < n <= R.LDS_MAX for n in lengths) and added[SLAB_QUERIES] == sum(n > R.LDS_MAX for n in lengths)
    for cos, c16 in zip(_pair_cosines(sc, case['P'], case['lists']), case['c16']):
        assert np.array_equal(cos * np.float32(16), c16.astype(np.float32))
    sc.close()


# ---- 2. every kernel form and its boundary ---------------------------------------------------------------------------------

def test_every_kernel_form_and_its_boundary(hip_lib):
    E, P, lists = R.form_case()
    sc = C.Scorer(E)
    got, added = _counted(sc, lambda: _ranked(sc, P, lists))
    assert added[CALLS] == 1 and added[LDS_QUERIES] == 7 and added[SLAB_QUERIES] == 2, added
    assert added[PAIRS] == sum(R.FORM_LENGTHS) and added[EMPTY] == 0
    cos = _pair_cosines(sc, P, lists)
    _same_lists(got, [R.expected_ranking(c, lst) for c, lst in zip(cos, lists)], 'forms')
    sc.close()


# ---- 3. prefiltered table --------------------------------------------------------------------------------------------------

def test_prefiltered_table_agrees_with_the_full_table_calls(hip_lib):
    E, P, lists = R.prefilter_case()
    sc = C.Scorer(E)
    full_cos = sc.cosines(P)
    full_idx, full_val = sc.rank(P, None)
    cos = _pair_cosines(sc, P, lists)
    got = _ranked(sc, P, lists)
    for q, lst in enumerate(lists):
        assert U.same_bits(cos[q], full_cos[q, lst.astype(np.int64)]), q
        keep = np.isin(full_idx[q], lst)
        _same_lists([got[q]], [(full_idx[q][keep], full_val[q][keep])], ('restricted', q))
        if len(lst) == R.PREFILTER_V:
            _same_lists([got[q]], [(full_idx[q], full_val[q])], ('every entity', q))
    assert any(len(lst) == R.PREFILTER_V for lst in lists)
    sc.close()


# ---- 4. row widths ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d', R.WIDTHS)
def test_row_widths(hip_lib, d):
    E, P, lists, cos64 = R.width_case(d)
    sc = C.Scorer(E)
    got, cos = _check_against_pair_cosines(sc, P, lists, ('width', d))
    worst = max(float(np.abs(c.astype(np.float64) - c64).max()) for c, c64 in zip(cos, cos64))
    print('d = %d: worst |cos - float64 cos| = %.3g, bound %.3g' % (d, worst, R.width_bound(d)))
    assert worst <= R.width_bound(d), (d, worst, R.width_bound(d))
    sc.close()


# ---- 5. special values -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', [1100, 8300])
def test_special_values(hip_lib, V):
    E, P, lists = R.special_case(V)
    zero = list(R.ZERO_ROWS(V))
    sc = C.Scorer(E)
    (got, cos), added = _counted(sc, lambda: _check_against_pair_cosines(sc, P, lists, ('special', V)))
    assert added[SLAB_QUERIES if V > R.LDS_MAX else LDS_QUERIES] == 5 and added[LDS_QUERIES] + added[SLAB_QUERIES] == 5, added
    for q, (lst, (idx, val)) in enumerate(zip(lists, got)):
        if q in R.NAN_QUERIES:
            assert np.array_equal(idx, lst) and np.isnan(val).all(), q
        else:
            assert idx[-3:].tolist() == zero and np.isnan(val[-3:]).all() and not np.isnan(val[:-3]).any(), q
    sc.close()


# ---- 6. k ------------------------------------------------------------------------------------------------------------------

def test_k_is_the_head_of_the_whole_list(hip_lib):
    E, P, lists = R.k_case()
    sc = C.Scorer(E)
    full = _ranked(sc, P, lists)
    assert [len(i) for i, _ in full] == list(R.K_LENGTHS)
    for k in R.K_VALUES:
        out_indptr, idx, val = sc.rank_candidates(P, lists, k)
        assert out_indptr.tolist() == np.concatenate([[0], np.cumsum(np.minimum(R.K_LENGTHS, k))]).tolist()      # compact offsets
        assert len(idx) == out_indptr[-1] == len(val)
        _same_lists(R.split(out_indptr, idx, val), [(i[:k], v[:k]) for i, v in full], ('k', k))
    sc.close()


# ---- 7. independence -------------------------------------------------------------------------------------------------------

def test_a_query_does_not_depend_on_the_call(hip_lib, monkeypatch):
    E, P, lists = R.form_case()
    sc = C.Scorer(E)
    want, added = _counted(sc, lambda: _ranked(sc, P, lists))
    assert added[CHUNKS] == 1
    for q in (0, 6, 7):
        _same_lists(_ranked(sc, P[q:q + 1], lists[q:q + 1]), want[q:q + 1], ('alone', q))
    _same_lists(_ranked(sc, P[::-1], lists[::-1]), want[::-1], 'reversed')
    monkeypatch.setenv('SERT_SCORE_RANK_BUDGET', '1')
    got, added = _counted(sc, lambda: _ranked(sc, P, lists))
    assert added[CHUNKS] == len(lists) and added[LDS_QUERIES] == 7 and added[SLAB_QUERIES] == 2, added
    _same_lists(got, want, 'one query per chunk')
    monkeypatch.setenv('SERT_SCORE_RANK_BUDGET', str(8 * 200))            # the pair call: 200 pairs per chunk
    cut, added = _counted(sc, lambda: _pair_cosines(sc, P[:3], lists[:3]))
    assert added[CHUNKS] == -(-sum(R.FORM_LENGTHS[:3]) // 200), added
    monkeypatch.delenv('SERT_SCORE_RANK_BUDGET')
    whole = _pair_cosines(sc, P, lists)
    assert all(U.same_bits(a, b) for a, b in zip(cut, whole[:3]))
    sc.close()


@pytest.mark.parametrize('k', [None, 7])
def test_chunks_of_several_queries_are_ranked_chunk_relative(hip_lib, monkeypatch, k):
    """Two chunks, [0, 4) and [4, 9) (tests/test_rerank_inputs_cpu.py proves the plan): the second one's kernels see its
    queries, candidates and output offsets counted from query 4, a padded slab of two rows, LDS lists and an empty list."""
    E, P, lists = R.chunk_case()
    sc = C.Scorer(E)
    want, added = _counted(sc, lambda: _ranked(sc, P, lists, k))
    assert added[CHUNKS] == 1, added
    monkeypatch.setenv('SERT_SCORE_RANK_BUDGET', str(R.CHUNK_BUDGETS[k]))
    got, added = _counted(sc, lambda: _ranked(sc, P, lists, k))
    monkeypatch.delenv('SERT_SCORE_RANK_BUDGET')
    assert added[CHUNKS] == len(R.CHUNK_BOUNDS) - 1 == 2, added
    assert added[LDS_QUERIES] == 4 and added[SLAB_QUERIES] == 4 and added[EMPTY] == 1, added
    _same_lists(got, want, ('two chunks against one', k))
    cos = _pair_cosines(sc, P, lists)
    _same_lists(got, [R.expected_ranking(c, lst, k) for c, lst in zip(cos, lists)], ('two chunks against the pair cosines', k))
    sc.close()


# ---- 8. reuse --------------------------------------------------------------------------------------------------------------

def test_a_reused_scorer_answers_as_a_fresh_one(hip_lib):
    E, P, lists = R.prefilter_case()
    steps = ['topk', 'rank', 'scores', 'rank_candidates', 'score_pairs', 'rank', 'rank_candidates']

    def do(sc, op):
        if op == 'topk':
            return tuple(a.copy() for a in sc.topk(P, 10))
        if op == 'rank':
            return sc.rank(P[:3], None)
        if op == 'scores':
            return (sc.scores(P[:2]),)
        if op == 'rank_candidates':
            return sc.rank_candidates(P, lists)
        return sc.score_pairs(P, lists)

    sc = C.Scorer(E)
    reused = [do(sc, op) for op in steps]
    sc.close()
    fresh_results = {}
    for op, got in zip(steps, reused):
        if op not in fresh_results:
            fresh = C.Scorer(E)
            fresh_results[op] = do(fresh, op)
            fresh.close()
        for a, b in zip(got, fresh_results[op]):
            assert a.dtype == b.dtype and (U.same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)), op


# ---- 9. arguments ----------------------------------------------------------------------------------------------------------

def test_arguments(hip_lib):
    E, P = U.gaussian_score_problem(1200, 16, 3, seed=23)
    sc = C.Scorer(E)
    lib = C.load()
    idx = np.empty(64, dtype=np.int32)
    val = np.empty(64, dtype=np.float32)

    def rank(indptr, ents, k=-1, proj=P, out=(idx, val)):
        indptr = None if indptr is None else np.asarray(indptr, dtype=np.int64)
        ents = None if ents is None else np.asarray(ents, dtype=np.int32)
        rc = lib.sert_scorer_rank_candidates(sc._h, C._addr(proj), 3, C._addr(indptr), C._addr(ents), k, C._addr(out[0]), C._addr(out[1]))
        return rc, lib.sert_last_error().decode()

    def pairs(indptr, ents, out=val):
        indptr = None if indptr is None else np.asarray(indptr, dtype=np.int64)
        ents = None if ents is None else np.asarray(ents, dtype=np.int32)
        rc = lib.sert_scorer_pairs(sc._h, P.ctypes.data, 3, C._addr(indptr), C._addr(ents), 1, C._addr(out))
        return rc, lib.sert_last_error().decode()

    good = ([0, 2, 2, 5], [4, 9, 0, 7, 1199])
    before = sc.debug_rerank_counts()
    faults = [(([1, 2, 2, 5], good[1]), 'cand_indptr[0] must be 0'),
              (([0, 3, 2, 5], good[1]), 'cand_indptr decreases'),
              ((good[0], [4, 9, 0, 7, 1200]), 'out of range'),
              ((good[0], [4, -1, 0, 7, 8]), 'out of range')]
    for args, text in faults:
        for call in (rank, pairs):
            rc, msg = call(*args)
            assert rc != 0 and text in msg, (args, msg)
    for ents, text in (([9, 4, 0, 7, 8], 'not strictly ascending'), ([4, 4, 0, 7, 8], 'not strictly ascending')):
        rc, msg = rank(good[0], ents)
        assert rc != 0 and text in msg, (ents, msg)
        assert pairs(good[0], ents)[0] == 0                         # any order and duplicates: fine for the pair call
    for k in (0, -2):
        rc, msg = rank(*good, k=k)
        assert rc != 0 and 'k must be -1 (the whole list) or positive' in msg
    for kw in (dict(proj=None), dict(out=(None, val)), dict(out=(idx, None))):
        rc, msg = rank(*good, **kw)
        assert rc != 0 and 'null argument' in msg, kw
    for args in ((None, good[1]), (good[0], None)):
        for call in (rank, pairs):
            rc, msg = call(*args)
            assert rc != 0 and 'null argument' in msg
    assert pairs(*good, out=None)[0] != 0
    assert lib.sert_scorer_rank_candidates(None, P.ctypes.data, 3, None, None, -1, None, None) != 0
    after = sc.debug_rerank_counts()
    assert after[CALLS] - before[CALLS] == 2 and after[PAIRS] - before[PAIRS] == 10       # refused calls launch and count nothing
    assert rank(*good)[0] == 0
    with pytest.raises(C.SertError, match='k must be'):
        sc.rank_candidates(P, [[1], [2], [3]], 0)
    with pytest.raises(C.SertError, match='k must be'):
        sc.rank_candidates(P, [[1], [2], [3]], -1)
    # the wrapper cleans the lists; the pair call keeps order and duplicates
    messy = [[7, 3, 7, 900, 3], [], [5, 4, 3, 2, 1, 1]]
    clean = [[3, 7, 900], [], [1, 2, 3, 4, 5]]
    _same_lists(_ranked(sc, P, messy), _ranked(sc, P, clean), 'cleaned lists')
    indptr, cos = sc.score_pairs(P, messy, raw=True)
    assert indptr.tolist() == [0, 5, 5, 11]
    full = sc.score_pairs(P, [np.arange(1200)] * 3, raw=True)[1].reshape(3, 1200)
    assert U.same_bits(cos, np.concatenate([full[q, np.asarray(m, dtype=np.int64)] for q, m in enumerate(messy)]))
    assert U.same_bits(sc.score_pairs(P, messy)[1], (cos + np.float32(1)) / np.float32(2))
    sc.close()


# ---- 10. the query callback ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', [300, 8300])
@pytest.mark.parametrize('top', [None, 50])
def test_callback_ranks_the_candidates(hip_lib, V, top):
    E, P = U.gaussian_score_problem(V, 16, 5, seed=29)
    rng = np.random.RandomState(2900 + V)
    lengths = [V, 120, 0, 1, 77]
    cand = {'q%d' % i: rng.permutation(V)[:n].astype(np.int32) for i, n in enumerate(lengths)}
    del cand['q2']                                       # (a topic without a list: an empty ranking)
    ranked = []

    def make():
        return scoring.VectorSpaceCallback(E.copy(), types.SimpleNamespace(top=top), types.SimpleNamespace(entity_representation_size=16),
                                           {}, None, lambda t, idx, val: ranked.append((t, np.array(idx), np.array(val))),
                                           candidates=cand)
    cb = make()
    kwargs = [{'topic_id': 'q%d' % i} for i in range(5)]
    _, added = _counted(cb.scorer, lambda: cb.process_batch([[1]] * 5, P.copy(), kwargs))
    assert added[CALLS] == 1 and added[EMPTY] == 1 and added[SLAB_QUERIES] == (V > R.LDS_MAX), added
    lists = [cand.get('q%d' % i, np.zeros(0, np.int32)) for i in range(5)]
    want = _ranked(cb.scorer, P, lists, top)
    assert len(ranked) == 5
    for q, (tid, idx, val) in enumerate(ranked):
        assert tid == 'q%d' % q and idx.dtype == np.int64 and len(idx) == min(lengths[q], top or V)
        assert np.array_equal(idx, want[q][0]) and U.same_bits(val, want[q][1])
    batch, ranked[:] = list(ranked), []
    one = make()
    for q in range(5):
        one.process([1], P[q:q + 1].copy(), 'q%d' % q)
    for (tid, idx, val), (btid, bidx, bval) in zip(ranked, batch):
        assert tid == btid and idx.dtype == np.int64 and np.array_equal(idx, bidx) and U.same_bits(val, bval)


# ---- 11. the CLI, both kinds -----------------------------------------------------------------------------------------------

def _run_lines(path):
    with io.open(path, encoding='utf8') as f:
        return [line.split() for line in f if line.strip()]


@pytest.mark.parametrize('kind', ['vectorspace', 'loglinear'])
def test_cli_candidates(hip_lib, tmp_path, kind):
    from tests.test_gpu_models import _write_tiny_corpus
    _write_tiny_corpus(tmp_path, kind)
    env = dict(os.environ, PYTHONPATH=U.ROOT)
    cmd = [sys.executable, os.path.join(U.ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'),
           '--meta', str(tmp_path / 'meta'), '--type', kind, '--iterations', '40', '--batch_size', '32',
           '--word_representation_size', '16', '--model_output', str(tmp_path / 'model'),
           '--seed', '1', '--loglevel', 'WARNING', '--regularization_lambda', '0.0']
    if kind == 'vectorspace':
        cmd += ['--num_negative_samples', '5', '--one_hot_classes', '--entity_representation_size', '16']
    subprocess.check_call(cmd, env=env)
    last = sorted((f for f in os.listdir(str(tmp_path)) if f.startswith('model_')),
                  key=lambda f: int(f.split('_')[1].split('.')[0]))[-1]

    def query(tag, *extra):
        r = subprocess.run([sys.executable, os.path.join(U.ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'),
                            '--model', str(tmp_path / last), '--topics', str(tmp_path / 'topics'),
                            '--run_out', str(tmp_path / ('run_' + tag)), '--loglevel', 'WARNING'] + list(extra), env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True)
        return _run_lines(str(tmp_path / ('run_%s_ef' % tag))), r.stdout.decode('utf-8', 'replace')

    full, _ = query('full')
    no_list = '5'
    picked = [f for f in full[::3] if f[0] != no_list]
    assert any(f[0] == no_list for f in full[::3]) and len(set(f[0] for f in picked)) == 11
    with io.open(str(tmp_path / 'first_stage'), 'w', encoding='utf8') as f:
        for fields in picked:
            f.write(u' '.join(fields) + u'\n')
        f.write(u'0 Q0 E777 90 0.5 first\n3 Q0 NOBODY 91 0.5 first\n')
    batched, log_b = query('cand_b', '--candidates', str(tmp_path / 'first_stage'))
    single, log_s = query('cand_s', '--candidates', str(tmp_path / 'first_stage'), '--no_batch')
    for log in (log_b, log_s):
        assert 'Dropped 2 candidates' in log and log.count('Dropped') == 1, log
    want = {}
    for fields in picked:
        want.setdefault(fields[0], set()).add(fields[2])
    for run in (batched, single):
        assert no_list not in set(f[0] for f in run)                     # the topic without a list: in neither run file
        got = {}
        for fields in run:
            got.setdefault(fields[0], []).append((fields[2], fields[4]))
        assert sorted(got) == sorted(want)
        for topic, entries in got.items():
            assert set(e for e, _ in entries) == want[topic] and len(entries) == len(want[topic]), topic
            scores = [float(s) for _, s in entries]
            assert all(a >= b for a, b in zip(scores, scores[1:])), topic
    if kind == 'loglinear':
        # the full run filtered: same order, scores as printed -- each against the full run of its own mode: the device
        # ranking and the per-token host path of --no_batch agree within a tolerance only, candidates or not
        # (tests/test_gpu_ll_rank.py::test_cli_batched_loglinear_query_matches_no_batch)
        full_single, _ = query('full_s', '--no_batch')
        for run, ref in ((batched, full), (single, full_single)):
            keep = [(f[0], f[2], f[4]) for f in ref if f[2] in want.get(f[0], ())]
            assert [(f[0], f[2], f[4]) for f in run] == keep
    else:
        assert [(f[0], f[2], f[4]) for f in batched] == [(f[0], f[2], f[4]) for f in single]
        d = 16
        bound = (2 * d + 8) * 2.0 ** -25 + 0.5e-10
        full_score = dict(((f[0], f[2]), float(f[4])) for f in full)
        worst = max(abs(float(f[4]) - full_score[(f[0], f[2])]) for f in batched)
        print('vectorspace: worst |score - full run score| = %.3g, bound %.3g' % (worst, bound))
        assert worst <= bound, (worst, bound)
