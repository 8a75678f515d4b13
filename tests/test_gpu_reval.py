"""-m gpu: retrieval evaluation on the live model (sert_reval_*, sert_amd.evaluation, bin/train.py --eval_*).

The rankings are compared BIT FOR BIT with the existing query paths on the same parameters, the metrics with the
trec_utils functions evaluated in float64 on the device's own ranking.  Bound on the metrics: 1e-9 absolute -- float64
sums of at most 1e5 non-negative terms differ by at most n 2^-53 ~ 1.1e-11 relative between summation orders, and every
metric is <= 1."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import _capi as C
from sert_amd import evaluation, inference, models, scoring, training
from sert_amd.utils import trec_utils
from tests import util as U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = 1e-9


def _queries(rng, vocab, count, max_len=12, long_one=40):
    lists = [list(rng.randint(0, vocab, size=rng.randint(1, max_len + 1))) for _ in range(count)]
    if long_one:
        lists.append(list(rng.randint(0, vocab, size=long_one)))
    return lists


def _judgements(rng, ranking, num_entities):
    """Per topic a relevance dict entity index -> gain, built around the ranking the existing path gives.  Keys >=
    num_entities stand for judged entities the model does not know.  Cycles through: empty, one entry (the entity at
    rank 1), unknown entities only, graded gains 0.5 / 1 / 2, a list longer than the ranked depth, the entity at the
    last rank, rank 1 and last rank together, a mix with zero and negative gains."""
    depth = ranking.shape[1]
    out = []
    for q in range(ranking.shape[0]):
        case = q % 8
        first, last = int(ranking[q, 0]), int(ranking[q, depth - 1])
        if case == 0:
            rel = {}
        elif case == 1:
            rel = {first: 1.0}
        elif case == 2:
            rel = {num_entities + 3: 1.0, num_entities + 7: 2.0}
        elif case == 3:
            ents = rng.choice(num_entities, size=min(num_entities, 9), replace=False)
            rel = dict((int(e), [0.5, 1.0, 2.0][i % 3]) for i, e in enumerate(ents))
        elif case == 4:
            ents = rng.choice(num_entities, size=min(num_entities, depth + 20), replace=False)
            rel = dict((int(e), 1.0) for e in ents)
            for extra in range(depth + 20 - len(ents) + 5):       # (longer than the depth even when every entity is ranked)
                rel[num_entities + extra] = 1.0
        elif case == 5:
            rel = {last: 2.0}
        elif case == 6:
            rel = {first: 0.5, last: 1.0, num_entities + 1: 1.0}
        else:
            ents = rng.choice(num_entities, size=min(num_entities, 12), replace=False)
            rel = dict((int(e), [1.0, 0.0, -1.0, 2.0][i % 4]) for i, e in enumerate(ents))
        out.append(rel)
    return out


def _reval(engine, token_lists, rels, k):
    num_entities = engine.cfg.num_entities
    depth = num_entities if k is None or k >= num_entities else k
    judgements = []
    for rel in rels:
        known = sorted((e, g) for e, g in rel.items() if e < num_entities)
        judgements.append((np.asarray([e for e, _ in known], dtype=np.int32), np.asarray([g for _, g in known], dtype=np.float32)))
    idcg = [evaluation.ideal_dcg(rel, depth) for rel in rels]
    num_rel = [sum(1 for g in rel.values() if g > 0) for rel in rels]
    return C.RetrievalEval(engine, token_lists, judgements, idcg, num_rel, k)


def _check_metrics(metrics, idx, rels, label):
    depth = idx.shape[1]
    worst = 0.0
    for q, rel in enumerate(rels):
        want = evaluation.host_metrics([int(e) for e in idx[q]], rel, depth)
        for c, name in enumerate(evaluation.METRICS):
            err = abs(metrics[q, c] - want[name])
            worst = max(worst, err)
            assert err <= TOL, (label, q, name, metrics[q, c], want[name])
    print('%s: %d topics, depth %d, largest metric difference %.3g' % (label, len(rels), depth, worst))


def _steps(eng, first, count):
    for step in range(first, first + count):        # (lazy word-table updates, every step announced: the run-ahead is in play)
        eng.hint_next_batch((step + 1) % 8)
        eng.train_batch(step % 8)


def _train_vs(Ve, de, seed, dw=32):
    B, n, z, Vw = 128, 5, 4, 3000
    p = U.make_vs_problem(seed, B * 8, n, z, Vw, Ve, dw, de, zipf=True)
    eng = U.vs_engine(p, B, n, z, 0.01, keep_grads=0)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    _steps(eng, 0, 32)
    return eng, p


def _plant_score_ladder(eng, Ve, de, seed):
    """Among V_e >= 32768 random entities the 101 best cosines of a topic lie so close together that float32 ties are
    expected (gaps ~3e-4 against a resolution of 6e-8, 100 pairs per topic and 48 topics).  So that no comparison rests on
    a tie: a bias that dominates the projection (every topic projects near p0 = tanh(b)) and an entity table with 108
    entities at cosines 0.95, 0.934, ... to p0 (gaps 0.016; a topic's own words and two further training steps, which move
    an element by about the learning rate 1e-3 of a row of norm >= 2, shift a cosine by less than a third of that) and
    every other entity below -0.85.  Directions orthogonal to p0 and the row norms stay random."""
    rng = np.random.RandomState(seed)
    b = (2.0 * rng.choice([-1.0, 1.0], size=de)).astype(np.float32)
    p0 = np.tanh(b.astype(np.float64))
    p0 /= np.linalg.norm(p0)
    c = -0.85 - 0.14 * rng.rand(Ve)
    planted = rng.choice(Ve, size=108, replace=False)
    c[planted] = 0.95 - 0.016 * np.arange(108)
    noise = rng.randn(Ve, de)
    noise -= np.outer(noise.dot(p0), p0)
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    table = c[:, None] * p0[None, :] + np.sqrt(1.0 - c * c)[:, None] * noise
    table *= rng.uniform(2.0, 4.0, size=(Ve, 1))
    eng.set_tensor(C.T_B, b)
    eng.set_tensor(C.T_RE, table.astype(np.float32))


@pytest.mark.parametrize('Ve,de,dw', [(500, 24, 32), (300, 20, 30), (32768, 32, 32)])
def test_vectorspace_ranking_and_metrics_equal_the_query_path(hip_lib, Ve, de, dw):
    """1 + 2 (vectorspace): sert_reval_run's ranking is np.array_equal to get_tensor -> numpy means -> predict_project ->
    Scorer.rank on the same parameters (V_e below and at the bf16-prefilter size, k in 1 / 5 / 100, topics of 1-12 tokens
    and one of 40), with a batch announced right before; the metrics match the host functions on that ranking.

    The two small shapes rank with the parameters as training left them (d_w = 30: the scalar form of the gather-mean):
    there every topic has its own order, and they are the evidence for the gather-mean and the projection.  In the V_e =
    32 768 case the order is dictated by the planted ladder (see _plant_score_ladder) and is much the same for every topic;
    what that case shows is that the large-table kernels (bf16 prefilter, fused selection) on device-resident blocks return
    bit-equal scores and indices."""
    eng, p = _train_vs(Ve, de, 21, dw)
    if Ve >= 32768:
        _plant_score_ladder(eng, Ve, de, 8)
        _steps(eng, 32, 2)        # (set_tensor flushed the lazy word table: two more steps put it back in play)
    rng = np.random.RandomState(4)
    lists = _queries(rng, p['Rw'].shape[0], 47)
    for k in (100, 5, 1):
        eng.hint_next_batch(3)
        # the evaluator first (nothing has flushed the lazy word table for it), judgements come after the reference ranking
        probe = _reval(eng, lists, [{} for _ in lists], k)
        _, status, idx, score = probe.run(return_ranking=True)
        probe.close()
        Rw = eng.get_tensor(C.T_RW, p['Rw'].shape)
        Re = eng.get_tensor(C.T_RE, p['Re'].shape)
        avg = np.stack([Rw[t, :].mean(axis=0) for t in lists])
        proj = eng.predict_project(avg)
        scorer = C.Scorer(Re)
        ref_idx, ref_val = (a.copy() for a in scorer.rank(proj, k))
        wide = scorer.rank(proj, min(k + 1, Ve))[1].copy()
        scorer.close()
        assert np.all(np.diff(wide, axis=1) < 0), 'the existing path ranks a tie inside the first k + 1'
        assert np.all(status == C.LL_STATUS_DEVICE)
        assert np.array_equal(idx, ref_idx) and np.array_equal(score, ref_val), k
        rels = _judgements(rng, ref_idx, Ve)
        ev = _reval(eng, lists, rels, k)
        metrics, _, idx2, _ = ev.run(return_ranking=True)
        ev.close()
        assert np.array_equal(idx2, ref_idx)
        _check_metrics(metrics, idx2, rels, 'vectorspace V_e=%d k=%d' % (Ve, k))
    eng.close()


@pytest.mark.parametrize('Ve,de,dw', [(500, 24, 32)])
def test_vectorspace_ranking_and_metrics_equal_the_query_path_with_a_zero_row_and_a_tie(hip_lib, Ve, de, dw):
    """The case the test above keeps out (it asserts a tie-free ranking): a table with an all-zero entity row -- no
    direction, NaN score, last at full depth -- and a relevant entity that duplicates a lower-index irrelevant one.  The
    evaluator's ranking stays bit-equal to the query path's ("One ranking order"), the metrics within 1e-9 of
    the host functions on that ranking."""
    eng, p = _train_vs(Ve, de, 23, dw)
    rng = np.random.RandomState(5)
    lists = _queries(rng, p['Rw'].shape[0], 15)
    probe = _reval(eng, lists, [{} for _ in lists], 5)
    top = probe.run(return_ranking=True)[2][:, 0]
    probe.close()
    Re = eng.get_tensor(C.T_RE, p['Re'].shape)
    lo, hi = sorted((int(top[0]), (int(top[0]) + 7) % Ve))
    zero = (hi + 11) % Ve
    assert zero != lo
    Re[hi] = Re[lo] = Re[int(top[0])].copy()
    Re[zero] = 0
    eng.set_tensor(C.T_RE, Re)
    for k in (Ve, 100, 5):
        # hi relevant, its lower-index twin lo judged by nobody; each topic's own best entity as well, unless it is the pair
        rels = [dict({hi: 1.0, zero: 2.0}, **({} if int(top[q]) in (lo, hi) else {int(top[q]): 0.5})) for q in range(len(lists))]
        assert all(lo not in rel for rel in rels)
        ev = _reval(eng, lists, rels, k)
        metrics, status, idx, score = ev.run(return_ranking=True)
        ev.close()
        Rw = eng.get_tensor(C.T_RW, p['Rw'].shape)
        avg = np.stack([Rw[t, :].mean(axis=0) for t in lists])
        scorer = C.Scorer(eng.get_tensor(C.T_RE, p['Re'].shape))
        ref_idx, ref_val = (a.copy() for a in scorer.rank(eng.predict_project(avg), k))
        scorer.close()
        assert np.all(status == C.LL_STATUS_DEVICE)
        assert np.array_equal(idx, ref_idx) and U.same_bits(score, ref_val), k
        for q in range(len(lists)):
            at = idx[q].tolist()
            if lo in at and hi in at:
                assert at.index(hi) == at.index(lo) + 1 and score[q, at.index(hi)] == score[q, at.index(lo)]
        assert idx[0, 0] == lo and idx[0, 1] == hi
        if k == Ve:
            assert np.all(idx[:, -1] == zero) and np.isnan(score[:, -1]).all() and not np.isnan(score[:, :-1]).any()
        _check_metrics(metrics, idx, rels, 'vectorspace zero row + tie k=%d' % k)
    eng.close()


def test_tied_entities_rank_by_lowest_index(hip_lib):
    """Two identical entity rows: the evaluator ranks the lower index first and scores that ranking."""
    eng, p = _train_vs(300, 24, 22)
    Re = eng.get_tensor(C.T_RE, p['Re'].shape)
    lists = _queries(np.random.RandomState(1), p['Rw'].shape[0], 6, long_one=0)
    ev = _reval(eng, lists, [{} for _ in lists], 5)
    top = ev.run(return_ranking=True)[2][:, 0]
    ev.close()
    a, b = int(top[0]), (int(top[0]) + 7) % 300
    Re[b] = Re[a]
    eng.set_tensor(C.T_RE, Re)
    lo, hi = min(a, b), max(a, b)
    rels = [{hi: 1.0} for _ in lists]
    ev = _reval(eng, lists, rels, 5)
    metrics, _, idx, score = ev.run(return_ranking=True)
    ev.close()
    assert idx[0, 0] == lo and idx[0, 1] == hi and score[0, 0] == score[0, 1]
    assert abs(metrics[0, C.REVAL_RECIP_RANK] - 0.5) <= TOL
    _check_metrics(metrics, idx, rels, 'tie')
    eng.close()


def _spread_bias(Ve, seed):
    """A bias that keeps float32 ties out of the rankings: 150 entities on a ladder 0.02 .. 3 (steps of 0.02, relative
    score gaps of 2 % where the trained weights shuffle the order), the others on a ladder -2 .. 0 (steps >= 2.2e-4)."""
    rng = np.random.RandomState(seed)
    b = np.empty(Ve)
    order = rng.permutation(Ve)
    b[order[:150]] = np.linspace(0.02, 3.0, 150)
    b[order[150:]] = np.linspace(-2.0, 0.0, Ve - 150)
    return b.astype(np.float32)


@pytest.mark.parametrize('Ve,d,budget', [(715, 32, None), (9000, 32, None), (715, 30, '1')])
def test_loglinear_ranking_and_metrics_equal_ll_rank_queries(hip_lib, monkeypatch, Ve, d, budget):
    """1 + 2 (loglinear): ranking, scores and status np.array_equal to sert_ll_rank_queries (top-k selection, the LDS sort at
    V_e = 715, the counting sort at V_e > 8192; k = 100 and every entity), metrics against the host functions.  Topics of
    1-6 tokens: longer products underflow float32 at these V_e and come back HOST on either path.

    budget '1': SERT_LL_RANK_BUDGET of one byte, so every topic is a chunk of its own (23 chunks) and the evaluator's
    per-chunk offsets (inputs, status, ranking rows, the topic offset of the metrics kernel) are all in play; d = 30 there
    takes the unvectorised row gather.  The k = 100 rounds rank with the trained weights (every topic its own order) and
    are the primary evidence; in the k = all rounds the order is the bias ladder's, the same for every topic, and the check
    rests on the bit-equal scores."""
    if budget:
        monkeypatch.setenv('SERT_LL_RANK_BUDGET', budget)
    B, n, Vw = 64, 5, 2000
    p = U.make_ll_problem(31, B * 4, n, Vw, Ve, d, 'int')
    p['b'] = _spread_bias(Ve, 3)
    eng = U.ll_engine(p, B, n, 0.01, keep_grads=0)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    for step in range(8):
        eng.hint_next_batch((step + 1) % 4)
        eng.train_batch(step % 4)
    rng = np.random.RandomState(6)
    lists = _queries(rng, Vw, 23, max_len=6, long_one=0)
    for k in (100, None):
        if k is None:
            # every entity ranked: the logits are the exact ladder (W shrunk far below its steps), so all V_e scores differ
            eng.set_tensor(C.T_W, eng.get_tensor(C.T_W) * np.float32(1e-5))
            eng.set_tensor(C.T_B, _spread_bias(Ve, 3))
        eng.hint_next_batch(1)
        probe = _reval(eng, lists, [{} for _ in lists], k)
        assert probe.num_chunks() == (len(lists) if budget else 1)       # (the budget really cut the call)
        _, status, idx, score = probe.run(return_ranking=True)
        probe.close()
        ref_idx, ref_score, _, _, ref_status, _ = eng.ll_rank_queries(lists, k)
        assert np.all(ref_status == C.LL_STATUS_DEVICE), 'a topic takes the host path on the existing call'
        wide = ref_score if k is None else eng.ll_rank_queries(lists, k + 1)[1]
        assert np.all(np.diff(wide, axis=1) < 0), 'the existing path ranks a tie inside the first k + 1'
        assert np.array_equal(status, ref_status)
        assert np.array_equal(idx, ref_idx) and np.array_equal(score, ref_score), k
        rels = _judgements(rng, ref_idx, Ve)
        ev = _reval(eng, lists, rels, k)
        metrics, _, idx2, _ = ev.run(return_ranking=True)
        ev.close()
        assert np.array_equal(idx2, ref_idx)
        _check_metrics(metrics, idx2, rels, 'loglinear V_e=%d k=%s' % (Ve, k))
    eng.close()


def _toy_model(kind, seed):
    B, n, Vw, Ve, d = 64, 4, 300, 40, 16
    np.random.seed(seed)
    if kind == 'vectorspace':
        p = U.make_vs_problem(seed, B * 6, n, 3, Vw, Ve, d, 24)
        cls, extra = models.VectorSpaceLanguageModel, dict(entity_representations_init=p['Re'], num_negative_samples=3)
    else:
        p = U.make_ll_problem(seed, B * 6, n, Vw, Ve, d, 'int')
        cls, extra = models.LanguageModel, dict(output_layer_size=Ve)
    cls.sampler_seed = 77
    try:
        model = cls(batch_size=B, window_size=n, representations_init=p['Rw'], regularization_lambda=0.01,
                    training_set=(p['X'][:B * 4], p['y'][:B * 4], p['w'][:B * 4]),
                    validation_set=(p['X'][B * 4:], p['y'][B * 4:]), **extra)
    finally:
        cls.sampler_seed = None
    return model, Vw, Ve


class _Entry(object):
    def __init__(self, id):
        self.id = id


def _toy_evaluator(model, Vw, Ve, k):
    words = dict(('w%d' % i, _Entry(i)) for i in range(Vw))
    inv = dict((i, 'E%d' % i) for i in range(Ve))
    rng = np.random.RandomState(9)
    topics = dict(('t%d' % q, ' '.join('w%d' % w for w in rng.randint(0, Vw, size=rng.randint(1, 5)))) for q in range(12))
    # 60 tokens: the loglinear joint underflows float32 (V_e = 40: about e^-220), the device reports HOST
    topics['long'] = ' '.join('w%d' % w for w in rng.randint(0, Vw, size=60))
    qrels = dict((t, dict(('E%d' % e, 1.0) for e in rng.choice(Ve, size=3, replace=False))) for t in topics)
    return evaluation.RetrievalEvaluator(model, topics, qrels, words, inv, k)


@pytest.mark.parametrize('kind', ['vectorspace', 'loglinear'])
def test_evaluation_does_not_disturb_training(hip_lib, tmp_path, kind):
    """3: two runs of the same model and seed through training.train, three epochs, one evaluated at every epoch boundary:
    the dumped parameters and the optimiser state are np.array_equal.  The evaluated set holds a 60-token topic, which
    the loglinear model hands back as HOST: the host path (predict_fn on the live engine) runs at every boundary too."""
    dumps = []
    for with_eval in (False, True):
        model, Vw, Ve = _toy_model(kind, 5)
        retrieval = [('validation', _toy_evaluator(model, Vw, Ve, 10 if kind == 'vectorspace' else None))] if with_eval else None
        out = str(tmp_path / ('eval' if with_eval else 'plain'))
        np.random.seed(123)
        training.train(model, 3, out, abort_threshold=1e-12, additional_args=['namespace'], save_optimizer_state=True,
                       retrieval=retrieval)     # (a dump starts with bin/train.py's namespace: read_checkpoint counts on it)
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


def test_host_status_topic_takes_the_host_path(hip_lib):
    """A loglinear topic the device hands back (status HOST) is evaluated through the per-token host path: its figures are
    the host metric functions on the ranking scoring.LogLinearCallback.process gives for it; the device-ranked topics
    beside it are untouched by that."""
    model, Vw, Ve = _toy_model('loglinear', 6)
    for _ in range(2):
        model.train()
    ev = _toy_evaluator(model, Vw, Ve, None)
    a = ev.arrays
    status = ev._eval.run()[1]
    long_q = a.device_topics.index('long')
    assert status[long_q] == C.LL_STATUS_HOST and (np.delete(status, long_q) == C.LL_STATUS_DEVICE).all()
    got = ev.evaluate()
    ranked = {}
    callback = scoring.LogLinearCallback(None, None, None, None,
                                         lambda topic_id, order, scores: ranked.__setitem__(topic_id, [int(i) for i in order]))
    batcher = inference.WordBatcher(model.predict_fn, model.batch_size, model.window_size,
                                    np.min_scalar_type(model.vocabulary_size - 1), callback)
    batcher.submit(a.token_lists[long_q], topic_id='long')
    batcher.process()
    want = evaluation.host_metrics(['E%d' % i for i in ranked['long']], ev.qrels['long'], a.depth)
    for name in evaluation.METRICS:
        assert abs(got['per_topic']['long'][name] - want[name]) <= TOL, (name, got['per_topic']['long'], want)
    # the others: the device's figures against the host functions on the device's ranking
    metrics, _, idx, _ = ev._eval.run(return_ranking=True)
    for q, topic in enumerate(a.device_topics):
        if q == long_q:
            continue
        want = evaluation.host_metrics(['E%d' % i for i in idx[q]], ev.qrels[topic], a.depth)
        for c, name in enumerate(evaluation.METRICS):
            assert abs(metrics[q, c] - want[name]) <= TOL and got['per_topic'][topic][name] == metrics[q, c]
    assert got['num_q'] == len(a.population) == 13
    ev.close()
    model._engine.close()


def test_live_means_live(hip_lib):
    """4: the figures follow the parameters -- they change with a training step and equal those of an evaluator created
    on the stepped model; a new entity table (set_tensor) is seen by the next run."""
    eng, p = _train_vs(400, 24, 23)
    rng = np.random.RandomState(2)
    lists = _queries(rng, p['Rw'].shape[0], 30)
    rels = [dict((int(e), 1.0) for e in rng.choice(400, size=40, replace=False)) for _ in lists]
    ev = _reval(eng, lists, rels, 100)
    before = ev.run()[0].copy()
    for step in range(4):
        eng.train_batch(step)
    after = ev.run()[0].copy()
    assert not np.array_equal(before, after)
    fresh = _reval(eng, lists, rels, 100)
    assert np.array_equal(fresh.run()[0], after)
    fresh.close()
    Re = eng.get_tensor(C.T_RE, p['Re'].shape)
    eng.set_tensor(C.T_RE, Re[::-1].copy())
    metrics, _, idx, _ = ev.run(return_ranking=True)
    assert not np.array_equal(metrics, after)
    _check_metrics(metrics, idx, rels, 'after set_tensor')
    ev.close()
    eng.close()


def test_error_paths_return_messages(hip_lib):
    """6: bad arguments fail through the error path with a message; nothing is launched."""
    eng, p = _train_vs(300, 24, 24)
    Vw = p['Rw'].shape[0]
    one = (np.asarray([1, 5], np.int32), np.asarray([1.0, 1.0], np.float32))

    def create(lists=([1, 2],), judgements=(one,), k=5, engine=eng):
        return C.RetrievalEval(engine, list(lists), list(judgements), [1.0] * len(lists), [1] * len(lists), k)

    create().close()
    for kwargs, text in ((dict(judgements=[(np.asarray([5, 1], np.int32), one[1])]), 'ascending'),
                         (dict(judgements=[(np.asarray([1, 300], np.int32), one[1])]), 'out of range'),
                         (dict(lists=[[1, Vw]]), 'token id out of range'),
                         (dict(lists=[[]]), 'at least one token'),
                         (dict(k=0), 'vectorspace evaluator ranks k'),
                         (dict(k=None), 'vectorspace evaluator ranks k'),
                         (dict(k=301), 'vectorspace evaluator ranks k')):
        with pytest.raises(C.SertError) as err:
            create(**kwargs)
        assert text in str(err.value), (kwargs, str(err.value))
    eng.close()
    pl = U.make_ll_problem(1, 64, 5, 500, 50, 16, 'int')
    ll = U.ll_engine(pl, 64, 5, 0.01, keep_grads=0)
    with pytest.raises(C.SertError) as err:
        create(k=0, engine=ll)
    assert 'k must be -1' in str(err.value)
    ll.close()


def _cli(tmp_path, env, prefix, iterations, flags=True, resume=None, kind='vectorspace'):
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'), '--meta',
           str(tmp_path / 'meta'), '--type', kind, '--iterations', str(iterations), '--batch_size', '64',
           '--word_representation_size', '16', '--entity_representation_size', '16', '--num_negative_samples', '2',
           '--one_hot_classes', '--regularization_lambda', '0.0', '--model_output', str(tmp_path / prefix), '--seed', '1',
           '--save_optimizer_state', '--loglevel', 'INFO']
    if flags:
        cmd += ['--eval_topics', str(tmp_path / 'topics'), '--eval_qrels', 'validation=' + str(tmp_path / 'qrel_validation'),
                'test=' + str(tmp_path / 'qrel_test')]
    if resume:
        cmd += ['--resume', str(tmp_path / resume)]
    done = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return done.stdout.decode('utf-8', 'replace')


def test_cli_reports_retrieval_quality_per_epoch(hip_lib, tmp_path):
    """5: bin/prepare.py -> bin/train.py --eval_topics ... --eval_qrels validation=... test=...: one JSON entry per set
    for epoch 0 and every epoch, each equal to bin/query.py on that epoch's dump followed by the host metric functions;
    the logged best epoch is the arg-max (earliest on a tie); --resume continues the file; no flags, no file."""
    from tests.test_prepare_cpu import _corpus
    _corpus(tmp_path, ndocs=60)
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'bin', 'prepare.py'), '--seed', '3', str(tmp_path / 'docs.trectext'),
                           '--assoc_path', str(tmp_path / 'assocs'), '--window_size', '4', '--overlapping',
                           '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1', '--no_instance_weights',
                           '--meta_output', str(tmp_path / 'meta'), '--data_output', str(tmp_path / 'data.npz'),
                           '--loglevel', 'ERROR'], env=env)
    (tmp_path / 'topics').write_text('t0;alpha beta gamma\nt1;kappa lambda sigma\nt2;red green blue\nt3;zzzz qqqq\n')
    # t3 has no in-vocabulary term and t4 no topic text: both count with 0; E7 is an entity the model does not know
    (tmp_path / 'qrel_validation').write_text('t0 0 E0 1\nt0 0 E1 0\nt1 0 E1 2\nt1 0 E7 1\nt2 0 E2 1\nt3 0 E0 1\nt4 0 E1 1\n')
    (tmp_path / 'qrel_test').write_text('t0 0 E1 1\nt1 0 E2 1\nt1 0 E1 1\nt2 0 E0 1\n')
    iterations = 2
    log = _cli(tmp_path, env, 'model', iterations)
    with open(str(tmp_path / 'model_retrieval.json')) as f:
        history = json.load(f)
    assert sorted(history) == [str(e) for e in range(iterations + 1)]
    qrels = {}
    for name in ('validation', 'test'):
        with open(str(tmp_path / ('qrel_' + name))) as f:
            qrels[name] = trec_utils.parse_qrels(f)
    for epoch in range(iterations + 1):
        run_out = str(tmp_path / ('run%d' % epoch))
        subprocess.check_call([sys.executable, os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'), '--model',
                               str(tmp_path / ('model_%d.bin' % epoch)), '--topics', str(tmp_path / 'topics'), '--top', '3',
                               '--run_out', run_out, '--loglevel', 'ERROR'], env=env)
        with open(run_out + '_ef') as f:
            run = trec_utils.parse_run(f)
        for entries in run.values():
            scores = sorted(s for s, _ in entries)
            assert all(a < b for a, b in zip(scores, scores[1:])), 'the run ranks a tie'
        for name in ('validation', 'test'):
            got = history[str(epoch)][name]
            assert got['num_q'] == len(qrels[name])
            per_topic = dict((t, evaluation.host_metrics(trec_utils._ranked(run.get(t, [])), rel, 3))
                             for t, rel in qrels[name].items() if t in run)
            want = evaluation.summarise(list(qrels[name]), per_topic, 3, 3)
            for key in ('ndcg', 'map', 'recip_rank', 'P_5'):
                assert abs(got[key] - want[key]) <= TOL, (epoch, name, key, got[key], want[key])
    ndcgs = [history[str(e)]['validation']['ndcg'] for e in range(iterations + 1)]
    best = ndcgs.index(max(ndcgs))
    assert 'Best epoch by validation NDCG: %d ' % best in log, log[-2000:]
    assert log.count('retrieval on validation') == iterations + 1 and log.count('retrieval on test') == iterations + 1

    # --resume continues the file of the interrupted run
    _cli(tmp_path, env, 'part', 1)
    with open(str(tmp_path / 'part_retrieval.json')) as f:
        assert sorted(json.load(f)) == ['0', '1']
    _cli(tmp_path, env, 'part', iterations, resume='part_1.bin')
    with open(str(tmp_path / 'part_retrieval.json')) as f:
        assert json.load(f) == history

    # without the flags: no such file, and the dumped namespace knows nothing of them
    _cli(tmp_path, env, 'plain', 1, flags=False)
    assert not os.path.exists(str(tmp_path / 'plain_retrieval.json'))
    with open(str(tmp_path / 'plain_1.bin'), 'rb') as f:
        namespace = pickle.load(f)
    assert not any(name.startswith('eval_') for name in vars(namespace))
