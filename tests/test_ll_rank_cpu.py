"""CPU (no GPU): the Python layer of the batched loglinear ranking.  inference.create(batched=True) routes a loglinear
callback to the BatchedWordRanker front end; LogLinearCallback.process_batch writes the _debug lines and makes the
rank_callback calls that LogLinearCallback.process makes, and sends the queries of status HOST through process.  The
device is replaced by a NumPy stand-in: per-token distributions from a fixed (V_w, V_e) table, ``rank_queries`` built
from oracle.loglinear_rank and scoring.compute_normalised_entropy."""
import io

import numpy as np

from oracle import sert_oracle as O
from sert_amd import inference, math_utils, scoring


class StandIn(object):
    """A loglinear predict_fn: __call__(batch, mask) -> (B, n, V_e) and rank_queries(token_lists, k)."""

    def __init__(self, table):
        self.table = table

    def __call__(self, batch, mask=None):
        return self.table[np.asarray(batch, dtype=np.int64)]

    def rank_queries(self, token_lists, k=None):
        V = self.table.shape[1]
        kk = V if k is None or k >= V else k
        Q = len(token_lists)
        idx, score = np.zeros((Q, kk), np.int64), np.zeros((Q, kk), np.float32)
        joint_h, token_h, status = np.zeros(Q, np.float32), [], np.zeros(Q, np.int32)
        for q, toks in enumerate(token_lists):
            dist = self.table[toks]
            token_h.append(np.asarray(scoring.compute_normalised_entropy(dist, base=2), np.float32))
            with np.errstate(divide='ignore', invalid='ignore'):
                order, vals = O.loglinear_rank(dist)
            if not np.isfinite(vals.sum()) or O.aggregate_product(dist).sum() == 0:
                status[q] = inference.QueryRanking.HOST
                continue
            idx[q], score[q] = order[:kk], vals[:kk]
            joint = np.empty(V, np.float32)
            joint[order] = vals
            joint_h[q] = math_utils.entropy(joint, base=2, normalize=True)
        return inference.QueryRanking(idx, score, joint_h, token_h, status, k=k)


def _problem(seed=0, Vw=40, Ve=30):
    rng = np.random.RandomState(seed)
    logits = rng.standard_normal((Vw, Ve)).astype(np.float32)
    table = np.exp(logits)
    table /= table.sum(axis=1, keepdims=True)
    table[Vw - 1] = 1.0 / Ve        # (a flat word: (1/30)^40 underflows float32 for every entity, S = 0)
    queries = [list(rng.randint(0, Vw - 1, rng.randint(1, 6))) for _ in range(12)]
    queries.insert(5, [Vw - 1] * 2 + [3])     # (two flat words: small, not zero -> ranked by the stand-in's "device")
    queries.insert(7, [Vw - 1] * 40)
    return StandIn(table.astype(np.float32)), queries, {i: 'w%d' % i for i in range(Vw)}


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, topic_id, idx, score):
        self.calls.append((topic_id, np.asarray(idx), np.asarray(score)))


def _run(fn, queries, tokens, batched):
    rec, dbg = _Recorder(), io.StringIO()
    cb = scoring.LogLinearCallback(None, None, tokens, dbg, rec)
    processed = []
    orig = cb.process

    def process(payload, distribution, topic_id):
        processed.append(topic_id)
        orig(payload, distribution, topic_id)
    cb.process = process
    fe = inference.create(fn, None, 16, 3, len(tokens), cb, batched=batched)
    for q, toks in enumerate(queries):
        fe.submit(toks, topic_id='T%d' % q)
    fe.process()
    return fe, rec.calls, dbg.getvalue(), processed


def test_create_routes_loglinear_to_the_batched_front_end():
    fn, _, tokens = _problem()
    cb = scoring.LogLinearCallback(None, None, tokens, None, lambda *a: None)
    assert isinstance(inference.create(fn, None, 4, 3, 40, cb, batched=True), inference.BatchedWordRanker)
    assert isinstance(inference.create(fn, None, 4, 3, 40, cb, batched=False), inference.WordBatcher)
    # a predict_fn without rank_queries keeps the unbatched path
    assert isinstance(inference.create(lambda b, m=None: fn(b), None, 4, 3, 40, cb, batched=True), inference.WordBatcher)


def test_process_batch_writes_what_process_writes():
    fn, queries, tokens = _problem()
    _, h_calls, h_dbg, _ = _run(fn, queries, tokens, batched=False)
    fe, b_calls, b_dbg, processed = _run(fn, queries, tokens, batched=True)
    assert isinstance(fe, inference.BatchedWordRanker)
    assert b_dbg == h_dbg
    assert [c[0] for c in b_calls] == [c[0] for c in h_calls]
    for (_, hi, hs), (_, bi, bs) in zip(h_calls, b_calls):
        assert np.array_equal(hi, bi) and np.array_equal(hs, bs, equal_nan=True)


def test_host_status_queries_go_through_process():
    fn, queries, tokens = _problem()
    r = fn.rank_queries(queries)
    host = ['T%d' % q for q in np.flatnonzero(r.status == inference.QueryRanking.HOST)]
    assert host == ['T7']
    _, _, _, processed = _run(fn, queries, tokens, batched=True)
    assert processed == host
    _, _, _, processed = _run(fn, queries, tokens, batched=False)
    assert len(processed) == len(queries)
