#!/usr/bin/env python
"""Wall time of one retrieval evaluation of a live model: evaluation.RetrievalEvaluator.evaluate() -- the call bin/train.py
makes per epoch and qrel set, as it makes it (per_topic=False) and with the per-topic dicts; its device part alone
(_capi.RetrievalEval.run) is recorded beside it -- against what the same figures cost without it -- in the same process and on the same parameters: the tables and the dense
layer copied to the host as model.get_state() does, the entity table uploaded again into a _capi.Scorer (vectorspace) or
the topics ranked by ll_rank_queries (loglinear), the query means taken with NumPy, and the trec_utils functions looped
over the rankings in Python.  The pickle, the process start and the run-file round trip of bin/query.py, which the
reference's per-epoch selection also pays (product-search.sh:136-170), are NOT charged to that side.

    python tools/reval_bench.py --out profiles/r08_reval.json

Shapes: (a) product search: V_e = 32 768, d_w = 300, d_e = 128, 1 000 topics of 1-12 tokens, k = 100;
(b) C5: 10 000 topics x V_e = 100 000, d = 128, k = 100; (c) loglinear at the W3C shape: V_e = 715, d = 300, 100 topics,
every entity ranked.  Median of --calls calls after --warmup.

--depths K ... (vectorspace shapes): the same shapes at other depths, 'none' = every entity -- above 1024 the evaluator counts
the judged entities' ranks instead of ranking (sert_reval_create_counted; DESIGN.md, "Evaluation depth without a sort"), and the
other side is Scorer.rank(proj, k) on the device (sert_scorer_rank) followed by the trec_utils functions; that call ALONE on
the same projections is recorded beside it (rank_alone_ms_*).  The host side of a deep ranking is slow (Python over Q x depth
entries), so the other side is timed --baseline_calls times after --baseline_warmup, and ONCE without warm-up where Q x depth
exceeds 1e8 (baseline_calls in the record says which).

    python tools/reval_bench.py --shapes product_search c5 --depths none 1000 --baseline_calls 3 --baseline_warmup 1 \
        --out profiles/r10_reval_counted.json
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi as C  # noqa: E402
from sert_amd import evaluation  # noqa: E402
from sert_amd.utils import trec_utils  # noqa: E402

SHAPES = {
    'product_search': dict(kind='vectorspace', Vw=100000, Ve=32768, dw=300, de=128, topics=1000, max_len=12, k=100),
    'c5': dict(kind='vectorspace', Vw=100000, Ve=100000, dw=128, de=128, topics=10000, max_len=12, k=100),
    'w3c_loglinear': dict(kind='loglinear', Vw=100000, Ve=715, dw=300, de=0, topics=100, max_len=6, k=None),
}


def glorot(rng, shape):
    a = np.sqrt(6.0 / sum(shape))
    return rng.uniform(-a, a, size=shape).astype(np.float32)


def make_engine(s, rng):
    vs = s['kind'] == 'vectorspace'
    eng = C.Engine(kind=C.KIND_VECTORSPACE if vs else C.KIND_LOGLINEAR, batch_size=1024, global_batch_size=1024,
                   window_size=8, vocab_size=s['Vw'], num_entities=s['Ve'], word_dim=s['dw'], entity_dim=s['de'],
                   num_negatives=10 if vs else 0, id_bytes=4, device=0, keep_grads=0, deterministic=1, lambda_=0.01,
                   lr=1e-3 if vs else 1.0, beta1=0.9 if vs else 0.95, beta2=0.999 if vs else 0.0, eps=1e-8 if vs else 1e-6,
                   seed=1)
    eng.set_tensor(C.T_RW, glorot(rng, (s['Vw'], s['dw'])))
    if vs:
        eng.set_tensor(C.T_RE, glorot(rng, (s['Ve'], s['de'])))
        eng.set_tensor(C.T_W, glorot(rng, (s['dw'], s['de'])))
        eng.set_tensor(C.T_B, (0.1 * rng.randn(s['de'])).astype(np.float32))
    else:
        eng.set_tensor(C.T_W, glorot(rng, (s['dw'], s['Ve'])))
        eng.set_tensor(C.T_B, (0.1 * rng.randn(s['Ve'])).astype(np.float32))
    return eng


def host_figures(idx, rels, depth):
    ndcg = ap = 0.0
    slow = idx.size > 1e8          # (minutes of Python: say that it is alive)
    for q, rel in enumerate(rels):
        if slow and q % 1000 == 0:
            print('# host metrics: topic %d of %d' % (q, len(rels)), file=sys.stderr, flush=True)
        ranked = idx[q].tolist()
        ndcg += trec_utils.ndcg_at_k(ranked, rel, depth)
        ap += trec_utils.average_precision(ranked, rel)
    return ndcg / len(rels), ap / len(rels)


def parent_path(eng, s, lists, rels, depth, keep=None):
    """One evaluation without the evaluator; -> (mean ndcg, mean ap).  keep: a dict that receives the projections."""
    Rw = eng.get_tensor(C.T_RW, (s['Vw'], s['dw']))
    eng.get_tensor(C.T_W)
    eng.get_tensor(C.T_B)                  # (get_state: predict_fn carries W and b)
    if s['kind'] == 'vectorspace':
        Re = eng.get_tensor(C.T_RE, (s['Ve'], s['de']))
        scorer = C.Scorer(Re)
        avg = np.empty((len(lists), s['dw']), dtype=np.float32)
        for i, tokens in enumerate(lists):
            avg[i] = Rw[tokens, :].mean(axis=0)
        proj = eng.predict_project(avg)
        if keep is not None:
            keep['proj'] = proj
        idx, _ = scorer.rank(proj, s['k'])
        out = host_figures(idx, rels, depth)
        scorer.close()
        return out
    idx = eng.ll_rank_queries(lists, s['k'])[0]
    return host_figures(idx, rels, depth)


def timed(fn, warmup, calls):
    for _ in range(warmup):
        last = fn()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        last = fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3, float(min(times)) * 1e3, last


def run_shape(name, s, warmup, calls, baseline_warmup=None, baseline_calls=None):
    rng = np.random.RandomState(7)
    eng = make_engine(s, rng)
    lists = [rng.randint(0, s['Vw'], size=rng.randint(1, s['max_len'] + 1)).tolist() for _ in range(s['topics'])]
    rels = [dict((int(e), 1.0) for e in rng.choice(s['Ve'], size=5, replace=False)) for _ in lists]
    depth = s['Ve'] if s['k'] is None or s['k'] >= s['Ve'] else s['k']
    # the evaluator as bin/train.py builds it: topic texts, qrels by entity id, the vocabulary, the entity map
    words = dict(('w%d' % i, types.SimpleNamespace(id=i)) for i in range(s['Vw']))
    inv = dict((i, 'E%d' % i) for i in range(s['Ve']))
    topics = dict(('t%d' % q, ' '.join('w%d' % t for t in tokens)) for q, tokens in enumerate(lists))
    qrels = dict(('t%d' % q, dict(('E%d' % e, g) for e, g in rel.items())) for q, rel in enumerate(rels))
    ev = evaluation.RetrievalEvaluator(types.SimpleNamespace(_engine=eng), topics, qrels, words, inv, s['k'])
    assert ev.arrays.token_lists == lists

    def figures(result):
        return result[evaluation.ndcg_key(result)], result['map']

    def device_part():
        metrics, status = ev._eval.run()
        assert not status.any()
        return float(metrics[:, C.REVAL_NDCG].mean()), float(metrics[:, C.REVAL_MAP].mean())

    eval_ms, eval_min, eval_fig = timed(lambda: figures(ev.evaluate(per_topic=False)), warmup, calls)
    full_ms, full_min, full_fig = timed(lambda: figures(ev.evaluate()), warmup, calls)
    run_ms, run_min, _ = timed(device_part, warmup, calls)
    bw, bc = (warmup if baseline_warmup is None else baseline_warmup), (calls if baseline_calls is None else baseline_calls)
    if len(lists) * depth > 1e8:
        bw, bc = 0, 1
    keep = {}
    parent_ms, parent_min, parent_fig = timed(lambda: parent_path(eng, s, lists, rels, depth, keep), bw, bc)
    assert eval_fig == full_fig
    rank_alone = {}
    if s['kind'] == 'vectorspace':
        # the ranking call of the other side alone, on the projections it ranked: a scorer on the same table, created outside the clock
        scorer = C.Scorer(eng.get_tensor(C.T_RE, (s['Ve'], s['de'])))
        ms, lo, _ = timed(lambda: scorer.rank(keep['proj'], s['k'])[0].shape, bw, bc)
        scorer.close()
        # the counted handle's run() at this depth, whichever handle the evaluator picked for it
        ar = ev.arrays
        ch = C.RetrievalEval(eng, ar.token_lists, ar.judgements, ar.ideal_dcg, ar.num_rel, s['k'], counted=True)
        cms, clo, _ = timed(lambda: ch.run()[0].shape, warmup, calls)
        ch.close()
        rank_alone = dict(rank_alone_ms_median=ms, rank_alone_ms_min=lo, counted_run_ms_median=cms, counted_run_ms_min=clo,
                          counted_run_over_rank_alone=cms / ms)
    counted = bool(getattr(ev._eval, 'counted', False))
    ev.close()
    eng.close()
    rec = dict(s, shape=name, depth=depth, calls=calls, warmup=warmup, counted=counted, baseline_calls=bc, baseline_warmup=bw,
               **rank_alone)
    rec.update(
               evaluate_ms_median=eval_ms, evaluate_ms_min=eval_min,
               evaluate_with_per_topic_ms_median=full_ms, evaluate_with_per_topic_ms_min=full_min,
               device_run_ms_median=run_ms, device_run_ms_min=run_min,
               parent_path_ms_median=parent_ms, parent_path_ms_min=parent_min,
               parent_over_evaluate=parent_ms / eval_ms, parent_over_evaluate_with_per_topic=parent_ms / full_ms,
               evaluate_mean_ndcg=eval_fig[0], parent_mean_ndcg=parent_fig[0], evaluate_mean_map=eval_fig[1], parent_mean_map=parent_fig[1])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument('--depths', nargs='+', default=['shape'], help="depths of the vectorspace shapes: 'shape' (the shape's own k), 'none' (every entity) or a number")
    ap.add_argument('--baseline_calls', type=int, default=None, help='calls of the other side (default: --calls)')
    ap.add_argument('--baseline_warmup', type=int, default=None, help='warm-up calls of the other side (default: --warmup)')
    args = ap.parse_args()
    runs = []
    for name in args.shapes:
        for d in (args.depths if SHAPES[name]['kind'] == 'vectorspace' else ['shape']):
            runs.append((name, SHAPES[name] if d == 'shape' else dict(SHAPES[name], k=None if d == 'none' else int(d))))
    C.require_gpu()
    result = {'device': C.device_info(0), 'what': 'median wall time of one evaluation.  evaluate: RetrievalEvaluator.evaluate(per_topic=False), the call of '
              'the epoch driver; evaluate_with_per_topic: evaluate() with its dict per topic; device_run: RetrievalEval.run alone; '
              'parent_path: get_tensor x 3-4 -> Scorer / ll_rank_queries -> NumPy means -> trec_utils in Python (baseline_calls calls after '
              'baseline_warmup); rank_alone: the Scorer.rank call of parent_path alone on the same projections; counted: the evaluator '
              'counts ranks instead of ranking.  Same process, same parameters',
              'shapes': [run_shape(name, s, args.warmup, args.calls, args.baseline_warmup, args.baseline_calls) for name, s in runs]}
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
