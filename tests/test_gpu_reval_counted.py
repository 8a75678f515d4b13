"""-m gpu: retrieval evaluation at any depth by counting ranks (sert_reval_create_counted, sert_reval_judged_ranks,
sert_debug_count_ranks; sert_amd.evaluation; bin/train.py --eval_top above 1024) -- DESIGN.md, "Evaluation depth without a
sort".

The ranks are compared EXACTLY: with a host ordering restated here for the counting kernel alone, with the position in
Scorer.rank(proj, None) on the same parameters for the evaluator.  The metrics are compared with the trec_utils functions
(evaluation.host_metrics) on that ranking cut at the depth, bound 1e-9 as in tests/test_gpu_reval.py: float64 sums of at most
1e5 terms differ by at most n 2^-53 ~ 1.1e-11 relative between summation orders, and every metric is <= 1 in magnitude for
gains in [-1, 2] over an ideal DCG that holds the largest gains."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import evaluation, training
from sert_amd.utils import trec_utils
from tests import test_gpu_reval as R          # (its helpers, as a module)
from tests import util as U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, 'golden', 'product_search')
TOL = 1e-9
NEG_NAN = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]
POS_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


# ---- 1: the counting kernel alone ------------------------------------------------------------------------------------

def _crafted_rows(V):
    """(6, V) float32.  0: Gaussian values with +0 and -0, NaNs of both signs, +-inf, denormals and duplicates strewn in;
    1: all NaN, of both signs; 2: the two zeros and a few numbers around them; 3: a handful of levels in long runs, with
    infinities and NaNs; 4: strictly descending; 5: one value throughout."""
    rng = np.random.RandomState(700 + V)
    at = np.arange(V)
    r = (0.3 * rng.randn(V)).astype(np.float32)
    r[at % 7 == 3] = np.float32(0.0)
    r[at % 14 == 5] = np.float32(-0.0)
    r[at % 41 == 11] = POS_NAN
    r[at % 43 == 13] = NEG_NAN
    r[at % 97 == 17] = np.inf
    r[at % 101 == 19] = -np.inf
    r[at % 53 == 23] = np.float32(1e-41)
    r[at % 59 == 29] = np.float32(-1e-41)
    r[at % 37 == 31] = r[min(2, V - 1)]
    z = np.where(rng.rand(V) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    z[at % 50 == 0] = (1e-3 * rng.randn(int((at % 50 == 0).sum()))).astype(np.float32)
    levels = np.array([-1.0, -0.25, -0.0, 0.0, 0.25, 1.0, np.inf, -np.inf, POS_NAN, NEG_NAN], dtype=np.float32)
    runs = levels[np.repeat(rng.randint(0, len(levels), size=V), rng.randint(1, 40))[:V]]
    return np.stack([r, np.where(at % 3 == 0, NEG_NAN, POS_NAN).astype(np.float32), z, runs,
                     np.linspace(1.0, -1.0, V, dtype=np.float32) if V > 1 else np.ones(1, np.float32),
                     np.full(V, 0.125, dtype=np.float32)])


def _host_ranks(rows):
    """rank[q][e], 1-based, under the scorer's order restated: NaN (either sign) after every number, then the cosine
    descending with -0 equal to +0, then the lowest entity index."""
    out = np.empty(rows.shape, dtype=np.int64)
    for q, row in enumerate(rows):
        nan = np.isnan(row)
        neg = np.where(nan, np.float32(0), -row + np.float32(0))          # (-0 and +0: one value)
        order = np.lexsort((np.arange(len(row)), neg, nan))               # (last key first)
        out[q, order] = np.arange(1, len(row) + 1)
    return out


@pytest.mark.parametrize('V', [1, 3, 64, 257, 1027, 4100, 8195, 8196])
def test_counting_kernel_on_crafted_rows(hip_lib, V):
    """V = 1, odd sizes, multiples of 4 (16-byte loads) and not (dwords), more than one trip of the four-load loop (4100),
    rows cut into two pieces whose counts meet in the atomics (from 8192 columns).  Two calls per V: one whose lists
    hold at most 8 entities (the tile of 8), one with a list of every entity and lists beyond 32 (the tile of 32, several
    passes).  Every list form on every kind of row: the forms rotate over the rows."""
    rows = _crafted_rows(V)
    want = _host_ranks(rows)
    assert sorted(want[0].tolist()) == list(range(1, V + 1))
    rng = np.random.RandomState(V)
    pick = lambda n: np.sort(rng.choice(V, size=min(V, n), replace=False))
    forms_small = [lambda: np.zeros(0, np.int64), lambda: pick(1), lambda: pick(8), lambda: pick(5), lambda: np.asarray([V - 1]),
                   lambda: pick(3)[::-1]]
    forms_large = [lambda: np.arange(V), lambda: pick(40), lambda: pick(33), lambda: np.zeros(0, np.int64), lambda: pick(1),
                   lambda: pick(9)]
    for forms in (forms_small, forms_large):
        for shift in range(len(forms)):
            judged = [forms[(q + shift) % len(forms)]() for q in range(rows.shape[0])]
            got = C.debug_count_ranks(rows, judged)
            for q, ents in enumerate(judged):
                assert got[q].dtype == np.int32 and np.array_equal(got[q], want[q, ents]), (V, shift, q, ents[:8], got[q][:8])
    # no list at all: nothing is launched, nothing comes back
    assert all(len(g) == 0 for g in C.debug_count_ranks(rows, [[] for _ in rows]))


# ---- the evaluator ---------------------------------------------------------------------------------------------------

def _counted(engine, token_lists, rels, k):
    """A counted handle for relevance dicts (keys >= num_entities: entities the model does not know), and per topic the
    uploaded entity indices in upload order."""
    num_entities = engine.cfg.num_entities
    depth = num_entities if k is None or k >= num_entities else k
    judgements, ents = [], []
    for rel in rels:
        known = sorted((e, g) for e, g in rel.items() if e < num_entities)
        ents.append(np.asarray([e for e, _ in known], dtype=np.int64))
        judgements.append((np.asarray([e for e, _ in known], dtype=np.int32), np.asarray([g for _, g in known], dtype=np.float32)))
    idcg = [evaluation.ideal_dcg(rel, depth) for rel in rels]
    num_rel = [sum(1 for g in rel.values() if g > 0) for rel in rels]
    ev = C.RetrievalEval(engine, token_lists, judgements, idcg, num_rel, k, counted=True)
    assert ev.depth == depth
    return ev, ents


def _reference_ranking(eng, p, lists):
    """Scorer.rank(proj, None) built as tests/test_gpu_reval.py does: get_tensor -> numpy means -> predict_project."""
    Rw = eng.get_tensor(C.T_RW, p['Rw'].shape)
    Re = eng.get_tensor(C.T_RE, p['Re'].shape)
    avg = np.stack([Rw[t, :].mean(axis=0) for t in lists])
    scorer = C.Scorer(Re)
    idx = scorer.rank(eng.predict_project(avg), None)[0].copy()
    scorer.close()
    assert idx.shape == (len(lists), Re.shape[0])
    return idx


def _positions(ranking):
    pos = np.empty(ranking.shape, dtype=np.int64)
    pos[np.arange(ranking.shape[0])[:, None], ranking] = np.arange(1, ranking.shape[1] + 1)[None, :]
    return pos


def _run_and_check(eng, lists, rels, k, ranking, label):
    """One counted evaluation: status, ranks == positions in `ranking` (every judged entity of every topic), metrics within
    TOL of host_metrics on the ranking cut at the depth.  -> (metrics, ranks per topic)."""
    ev, ents = _counted(eng, lists, rels, k)
    metrics, status = ev.run()
    flat = ev.judged_ranks()
    indptr = ev.rel_indptr
    depth = ev.depth
    ev.close()
    assert np.all(status == C.LL_STATUS_DEVICE)
    pos = _positions(ranking)
    ranks = [flat[indptr[q]:indptr[q + 1]] for q in range(len(lists))]
    for q in range(len(lists)):
        assert np.array_equal(ranks[q], pos[q, ents[q]]), (label, q, ranks[q][:10], pos[q, ents[q]][:10])
    R._check_metrics(metrics, ranking[:, :depth], rels, label)
    return metrics, ranks


@pytest.mark.parametrize('Ve,de,dw', [(500, 24, 32), (300, 20, 30)])
def test_small_trained_models(hip_lib, Ve, de, dw):
    """2: 47 topics of 1-12 tokens and one of 40, a batch announced right before every run; k = every entity, V_e, far above
    V_e, 100, 5, 1; the eight judgement patterns of _judgements around each depth's cut (a list of every entity among them:
    many passes of the tile).  Up to min(V_e, 1024) the figures also meet the ranking evaluator's on the same engine."""
    eng, p = R._train_vs(Ve, de, 21, dw)
    rng = np.random.RandomState(4)
    lists = R._queries(rng, p['Rw'].shape[0], 47)
    # the counted evaluator first: nothing has flushed the lazy word table for it.  No judgements: every figure is 0
    eng.hint_next_batch(3)
    probe, _ = _counted(eng, lists, [{} for _ in lists], None)
    metrics, status = probe.run()
    assert len(probe.judged_ranks()) == 0
    probe.close()
    assert np.all(status == C.LL_STATUS_DEVICE) and not metrics.any()
    ranking = _reference_ranking(eng, p, lists)
    for k in (None, Ve, Ve + 1700, 100, 5, 1):
        depth = Ve if k is None or k >= Ve else k
        rels = R._judgements(rng, ranking[:, :depth], Ve)
        eng.hint_next_batch(3)
        metrics, _ = _run_and_check(eng, lists, rels, k, ranking, 'counted V_e=%d k=%s' % (Ve, k))
        if k is not None and k <= min(Ve, 1024):
            old = R._reval(eng, lists, rels, k)
            old_metrics, _, old_idx, _ = old.run(return_ranking=True)
            old.close()
            assert np.array_equal(old_idx, ranking[:, :depth])
            worst = np.abs(metrics - old_metrics).max()
            print('against the ranking evaluator, k=%d: largest difference %.3g' % (k, worst))
            assert worst <= TOL, (k, worst)
    eng.close()


def test_depth_above_1024_that_still_cuts(hip_lib):
    """3: V_e = 1500, k = 1025, relevant entities at ranks 1, 1024, 1025, 1026 and 1500: the one at 1025 counts, the one at
    1026 does not."""
    Ve = 1500
    eng, p = R._train_vs(Ve, 24, 25)
    lists = R._queries(np.random.RandomState(7), p['Rw'].shape[0], 5)
    ranking = _reference_ranking(eng, p, lists)
    places = (1, 1024, 1025, 1026, 1500)
    rels = [dict((int(ranking[q, r - 1]), 1.0 + (r == 1025)) for r in places) for q in range(len(lists))]
    metrics, ranks = _run_and_check(eng, lists, rels, 1025, ranking, 'V_e=1500 k=1025')
    for q in range(len(lists)):
        assert sorted(ranks[q].tolist()) == list(places)
        assert metrics[q, C.REVAL_NUM_REL_RET] == 3.0 and metrics[q, C.REVAL_RECIP_RANK] == 1.0 and metrics[q, C.REVAL_P5] == 0.2
        idcg = evaluation.ideal_dcg(rels[q], 1025)
        with_1025 = (1.0 + 1.0 / np.log2(1025.0) + 2.0 / np.log2(1026.0)) / idcg
        assert abs(metrics[q, C.REVAL_NDCG] - with_1025) <= TOL
        assert abs(metrics[q, C.REVAL_MAP] - (1.0 + 2.0 / 1024 + 3.0 / 1025) / 5) <= TOL
    eng.close()


def test_bf16_prefiltered_table(hip_lib):
    """4: V_e = 32768 (the table takes the bf16 prefilter, so the cosines ranked are the exact_dot32 ones), d_e = 32, 8
    topics, k = every entity and 2000.  Judgements around the cut of each depth, a list longer than 2000, zero and
    negative gains, unknown entities."""
    Ve = 32768
    eng, p = R._train_vs(Ve, 32, 21)
    rng = np.random.RandomState(11)
    lists = R._queries(rng, p['Rw'].shape[0], 7)
    assert len(lists) == 8
    ranking = _reference_ranking(eng, p, lists)
    for k in (None, 2000):
        depth = Ve if k is None else k
        rels = []
        for q in range(len(lists)):
            rel = {int(ranking[q, 0]): 1.0, int(ranking[q, depth - 1]): 2.0, int(ranking[q, Ve - 1]): 0.5, Ve + 5: 1.0}
            if depth < Ve:
                rel[int(ranking[q, depth])] = 1.0                                    # (first rank outside)
            for i, e in enumerate(rng.choice(Ve, size=2020 if q == 3 else 30, replace=False)):
                rel.setdefault(int(e), [1.0, 0.0, -1.0, 2.0][i % 4])
            rels.append(rel)
        rels[5] = {}
        eng.hint_next_batch(3)
        _run_and_check(eng, lists, rels, k, ranking, 'bf16-prefiltered V_e=%d k=%s' % (Ve, k))
    eng.close()


def test_zero_entity_row_and_duplicated_rows(hip_lib):
    """5: an all-zero entity row (no direction: NaN cosine) judged relevant has rank V_e; of two identical rows the
    higher index has the lower one's rank + 1."""
    Ve = 500
    eng, p = R._train_vs(Ve, 24, 23)
    lists = R._queries(np.random.RandomState(5), p['Rw'].shape[0], 15)
    probe = R._reval(eng, lists, [{} for _ in lists], 5)
    top = probe.run(return_ranking=True)[2][:, 0]
    probe.close()
    Re = eng.get_tensor(C.T_RE, p['Re'].shape)
    lo, hi = sorted((int(top[0]), (int(top[0]) + 7) % Ve))
    zero = (hi + 11) % Ve
    assert zero != lo
    Re[hi] = Re[lo] = Re[int(top[0])].copy()
    Re[zero] = 0
    eng.set_tensor(C.T_RE, Re)
    ranking = _reference_ranking(eng, p, lists)
    assert np.all(ranking[:, -1] == zero)
    for k in (None, 100):
        # hi relevant, its twin lo judged irrelevant (so that its rank is reported), the NaN entity relevant
        rels = [dict({hi: 1.0, lo: 0.0, zero: 2.0}, **({} if int(top[q]) in (lo, hi) else {int(top[q]): 0.5}))
                for q in range(len(lists))]
        _, ranks = _run_and_check(eng, lists, rels, k, ranking, 'zero row + twins k=%s' % k)
        for q, rel in enumerate(rels):
            rank_of = dict(zip(sorted(rel), ranks[q].tolist()))
            assert rank_of[zero] == Ve and rank_of[hi] == rank_of[lo] + 1, (q, rank_of)
        assert dict(zip(sorted(rels[0]), ranks[0].tolist()))[lo] == 1
    eng.close()


def test_slab_edges(hip_lib):
    """6: 1100 topics at V_e = 300 -- three slabs of the cosine buffer, the last one of 76 rows.  The figures and ranks of the
    topics around each slab edge, and of the last slab, are those of the same topics in a handle of their own."""
    Ve = 300
    eng, p = R._train_vs(Ve, 24, 26)
    rng = np.random.RandomState(12)
    lists = R._queries(rng, p['Rw'].shape[0], 1099)
    assert len(lists) == 1100
    rels = [dict((int(e), [1.0, 2.0, 0.0, 0.5, -1.0][i % 5]) for i, e in enumerate(rng.choice(Ve, size=1 + q % 11, replace=False)))
            for q in range(len(lists))]
    ev, _ = _counted(eng, lists, rels, None)
    metrics, status = ev.run()
    flat, indptr = ev.judged_ranks(), ev.rel_indptr
    ev.close()
    assert np.all(status == C.LL_STATUS_DEVICE) and len(np.unique(metrics[:, C.REVAL_NDCG])) > 500
    for a, b in ((0, 20), (500, 530), (1010, 1040), (1024, 1100)):
        sub, _ = _counted(eng, lists[a:b], rels[a:b], None)
        sub_metrics, _ = sub.run()
        sub_flat = sub.judged_ranks()
        sub.close()
        assert np.array_equal(sub_metrics, metrics[a:b]), (a, b)
        assert np.array_equal(sub_flat, flat[indptr[a]:indptr[b]]), (a, b)
    # and the whole set against the reference ranking
    ranking = _reference_ranking(eng, p, lists)
    pos = _positions(ranking)
    for q, rel in enumerate(rels):
        assert np.array_equal(flat[indptr[q]:indptr[q + 1]], pos[q, sorted(rel)]), q
    R._check_metrics(metrics, ranking, rels, 'slab edges')
    eng.close()


def test_counted_evaluation_does_not_disturb_training(hip_lib, tmp_path):
    """7: two runs of the same model and seed through training.train, three epochs, one evaluated by a counted handle (k =
    None on a vectorspace model) at every epoch boundary: dumped parameters and optimiser state are np.array_equal."""
    dumps = []
    for with_eval in (False, True):
        model, Vw, Ve = R._toy_model('vectorspace', 5)
        retrieval = None
        if with_eval:
            evaluator = R._toy_evaluator(model, Vw, Ve, None)
            assert evaluator._eval.counted and evaluator.arrays.depth == Ve
            retrieval = [('validation', evaluator)]
        out = str(tmp_path / ('eval' if with_eval else 'plain'))
        np.random.seed(123)
        training.train(model, 3, out, abort_threshold=1e-12, additional_args=['namespace'], save_optimizer_state=True,
                       retrieval=retrieval)
        assert os.path.exists(out + '_retrieval.json') == with_eval
        dumps.append(training.read_checkpoint(out + '_3.bin'))
        model._engine.close()
    a, b = dumps
    for x, y in zip(a['tables'], b['tables']):
        assert np.array_equal(x, y)
    sa, sb = a['predict_fn'].__getstate__(), b['predict_fn'].__getstate__()
    assert np.array_equal(sa['W'], sb['W']) and np.array_equal(sa['b'], sb['b'])
    for name, value in a['trailer']['optimizer_state'].items():
        assert np.array_equal(value, b['trailer']['optimizer_state'][name]), name
    assert a['trailer']['errors'] == b['trailer']['errors']
    assert len(b['trailer']['retrieval']) == 4 and 'retrieval' not in a['trailer']
    assert all('ndcg' in entry['validation'] for entry in b['trailer']['retrieval'].values())


def test_counted_live_means_live(hip_lib):
    """8: the figures follow the parameters: a second run() after more steps differs, and equals a fresh handle's; a new
    entity table is seen by the next run."""
    eng, p = R._train_vs(400, 24, 23)
    rng = np.random.RandomState(2)
    lists = R._queries(rng, p['Rw'].shape[0], 30)
    rels = [dict((int(e), 1.0) for e in rng.choice(400, size=40, replace=False)) for _ in lists]
    ev, _ = _counted(eng, lists, rels, None)
    before, ranks_before = ev.run()[0].copy(), ev.judged_ranks()
    for step in range(4):
        eng.train_batch(step)
    after, ranks_after = ev.run()[0].copy(), ev.judged_ranks()
    assert not np.array_equal(before, after) and not np.array_equal(ranks_before, ranks_after)
    fresh, _ = _counted(eng, lists, rels, None)
    assert np.array_equal(fresh.run()[0], after) and np.array_equal(fresh.judged_ranks(), ranks_after)
    fresh.close()
    Re = eng.get_tensor(C.T_RE, p['Re'].shape)
    eng.set_tensor(C.T_RE, Re[::-1].copy())
    ev.close()
    metrics, _ = _run_and_check(eng, lists, rels, None, _reference_ranking(eng, p, lists), 'after set_tensor')
    assert not np.array_equal(metrics, after)
    eng.close()


def test_counted_error_paths_return_messages(hip_lib):
    """9: refusals come through the error path with their message."""
    eng, p = R._train_vs(300, 24, 24)
    one = (np.asarray([1, 5], np.int32), np.asarray([1.0, 1.0], np.float32))

    def create(judgements=(one,), k=5, engine=eng, counted=True):
        return C.RetrievalEval(engine, [[1, 2]], list(judgements), [1.0], [1], k, counted=counted)

    for kwargs, text in ((dict(k=0), 'k must be -1'), (dict(k=-2), 'k must be -1'),
                         (dict(judgements=[(np.asarray([5, 1], np.int32), one[1])]), 'ascending'),
                         (dict(judgements=[(np.asarray([1, 300], np.int32), one[1])]), 'out of range')):
        with pytest.raises(C.SertError) as err:
            create(**kwargs)
        assert text in str(err.value), (kwargs, str(err.value))
    ev = create(k=2000)
    with pytest.raises(C.SertError) as err:
        ev.judged_ranks()
    assert 'no sert_reval_run' in str(err.value)
    with pytest.raises(C.SertError):
        ev.run(return_ranking=True)
    # the C boundary itself: a ranking output that is not NULL
    metrics, status = np.empty((1, C.REVAL_NUM_METRICS)), np.empty(1, np.int32)
    idx, score = np.empty((1, 300), np.int32), np.empty((1, 300), np.float32)
    assert hip_lib.sert_reval_run(ev._h, metrics.ctypes.data, status.ctypes.data, idx.ctypes.data, score.ctypes.data) != 0
    assert b'sert_scorer_rank' in hip_lib.sert_last_error()
    assert ev.run()[1][0] == C.LL_STATUS_DEVICE and len(ev.judged_ranks()) == 2
    ev.close()
    ranked = create(counted=False)
    ranked.run()
    with pytest.raises(C.SertError) as err:
        ranked.judged_ranks()
    assert 'not a counted evaluator' in str(err.value)
    ranked.close()
    eng.close()
    pl = U.make_ll_problem(1, 64, 5, 500, 50, 16, 'int')
    ll = U.ll_engine(pl, 64, 5, 0.01, keep_grads=0)
    with pytest.raises(C.SertError) as err:
        create(engine=ll)
    assert 'vectorspace kinds' in str(err.value)
    ll.close()


# ---- 10: the CLI on the product-search fixtures ---------------------------------------------------------------------------

def _product_corpus(tmp_path):
    """A corpus around tests/golden/product_search: two documents per product of product_list, written in the words of a
    topic the qrels judge it relevant for (any topic otherwise) plus a few words of another topic."""
    with open(os.path.join(GOLD, 'topics')) as f:
        topics = trec_utils.parse_topics(f)
    with open(os.path.join(GOLD, 'product_list')) as f:
        products = [line.strip() for line in f if line.strip()]
    relevant_for = {}
    for name in ('validation', 'test'):
        with open(os.path.join(GOLD, 'qrel_' + name)) as f:
            for topic, rel in trec_utils.parse_qrels(f).items():
                for entity, gain in rel.items():
                    if gain > 0 and topic in topics:
                        relevant_for.setdefault(entity, topic)
    rng = np.random.RandomState(0)
    ids = list(topics)
    docs, assocs = [], []
    for i, product in enumerate(products):
        own = topics[relevant_for.get(product, ids[rng.randint(len(ids))])].split()
        for d in range(2):
            other = topics[ids[rng.randint(len(ids))]].split()
            text = rng.choice(own, size=18).tolist() + rng.choice(other, size=4).tolist()
            docs.append('<DOC>\n<DOCNO> D%04d_%d </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n' % (i, d, ' '.join(text)))
            assocs.append('%s D%04d_%d 1' % (product, i, d))
    (tmp_path / 'docs.trectext').write_text(''.join(docs))
    (tmp_path / 'assocs').write_text('\n'.join(assocs) + '\n')
    return len(products)


def test_cli_evaluates_every_entity_above_the_top_k_range(hip_lib, tmp_path):
    """10: bin/train.py --type vectorspace ... --eval_top 5000 (refused before: above min(entities, 1024)) writes 'ndcg',
    not 'ndcg_cut_K', and every epoch's entry equals bin/query.py without --top on that epoch's dump followed by the host
    metric functions.  The run file orders equal scores by entity id; the comparison needs the judged entities of a topic
    free of such ties, which is asserted."""
    num_products = _product_corpus(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'bin', 'prepare.py'), '--seed', '3', str(tmp_path / 'docs.trectext'),
                           '--assoc_path', str(tmp_path / 'assocs'), '--window_size', '4', '--overlapping',
                           '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1', '--no_instance_weights',
                           '--meta_output', str(tmp_path / 'meta'), '--data_output', str(tmp_path / 'data.npz'),
                           '--loglevel', 'ERROR'], env=env)
    iterations = 1
    sets = ('validation', 'test')
    subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'), '--meta',
                    str(tmp_path / 'meta'), '--type', 'vectorspace', '--iterations', str(iterations), '--batch_size', '64',
                    '--word_representation_size', '16', '--entity_representation_size', '16', '--num_negative_samples', '2',
                    '--one_hot_classes', '--regularization_lambda', '0.0', '--model_output', str(tmp_path / 'model'), '--seed', '1',
                    '--loglevel', 'INFO', '--eval_topics', os.path.join(GOLD, 'topics'), '--eval_qrels'] +
                   ['%s=%s' % (name, os.path.join(GOLD, 'qrel_' + name)) for name in sets] + ['--eval_top', '5000'],
                   env=env, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    with open(str(tmp_path / 'model_retrieval.json')) as f:
        history = json.load(f)
    assert sorted(history) == [str(e) for e in range(iterations + 1)]
    qrels = {}
    for name in sets:
        with open(os.path.join(GOLD, 'qrel_' + name)) as f:
            qrels[name] = trec_utils.parse_qrels(f)
    for epoch in range(iterations + 1):
        run_out = str(tmp_path / ('run%d' % epoch))
        subprocess.check_call([sys.executable, os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'), '--model',
                               str(tmp_path / ('model_%d.bin' % epoch)), '--topics', os.path.join(GOLD, 'topics'),
                               '--run_out', run_out, '--loglevel', 'ERROR'], env=env)
        with open(run_out + '_ef') as f:
            run = trec_utils.parse_run(f)
        assert run and all(len(entries) == num_products for entries in run.values())       # (every entity ranked)
        for name in sets:
            got = history[str(epoch)][name]
            assert got['num_q'] == len(qrels[name])
            assert 'ndcg' in got and not any(key.startswith('ndcg_cut') for key in got), sorted(got)
            per_topic = {}
            for topic, rel in qrels[name].items():
                if topic not in run:
                    continue
                scores = [s for s, _ in run[topic]]
                for s, e in run[topic]:
                    assert e not in rel or scores.count(s) == 1, 'the run ties a judged entity: %s %s' % (topic, e)
                per_topic[topic] = evaluation.host_metrics(trec_utils._ranked(run[topic]), rel, num_products)
            assert per_topic
            want = evaluation.summarise(list(qrels[name]), per_topic, num_products, num_products)
            for key in ('ndcg', 'map', 'recip_rank', 'P_5'):
                assert abs(got[key] - want[key]) <= TOL, (epoch, name, key, got[key], want[key])
