#!/usr/bin/env python
"""Loglinear query ranking: the batched device path (LogLinearPredictFn.rank_queries + LogLinearCallback.process_batch
through inference.BatchedWordRanker) against the host path bin/query.py --no_batch takes (WordBatcher + predict_fn +
LogLinearCallback.process), in the same process on the same box, queries/s of each.

    python tools/ll_query_bench.py --out profiles/r07_ll_query.json

Settings: the W3C query setting (d = 300, V_e = 715, window 8, batch 1024, 10 000 queries of 1-6 tokens) and d = 300,
V_e = 100 000 with k = 100 and k = None (--host_queries_big queries on the host path there: each of its predict_fn calls
ships batch x window x V_e floats to the host).  Random weights: R_w ~ U(-0.5, 0.5), W ~ N(0, 0.25^2), b = 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi, inference, models, scoring  # noqa: E402


def make(Vw, Ve, d, Q, seed=0):
    rng = np.random.RandomState(seed)
    fn = models.LogLinearPredictFn(R_w=rng.uniform(-0.5, 0.5, (Vw, d)).astype(np.float32),
                                   W=(rng.standard_normal((d, Ve)) * 0.25).astype(np.float32),
                                   b=np.zeros(Ve, np.float32), window_size=8)
    return fn, [list(rng.randint(0, Vw, rng.randint(1, 7))) for _ in range(Q)]


class _Sink(object):
    def __init__(self):
        self.n = 0

    def __call__(self, topic_id, idx, score):
        self.n += 1


def run(fn, queries, batched, batch_size, k=None):
    """Seconds for all queries, callback output included (rank_callback only counts)."""
    sink = _Sink()
    cb = scoring.LogLinearCallback(None, None, {}, None, sink)
    t0 = time.perf_counter()
    if batched:
        fe = inference.BatchedWordRanker(fn, batch_size, 8, np.min_scalar_type(fn.R_w.shape[0] - 1), cb, k=k)
    else:
        fe = inference.create(fn, None, batch_size, 8, fn.R_w.shape[0], cb, batched=False)
    for q, toks in enumerate(queries):
        fe.submit(toks, topic_id=q)
    fe.process()
    dt = time.perf_counter() - t0
    assert sink.n == len(queries)
    return dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--vocab', type=int, default=20000)
    ap.add_argument('--queries', type=int, default=10000)
    ap.add_argument('--device_queries_big', type=int, default=2000)
    ap.add_argument('--host_queries_big', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    rows = []
    settings = [('w3c', 715, None, a.queries, a.queries),
                ('ve100k_k100', 100000, 100, a.device_queries_big, a.host_queries_big),
                ('ve100k_all', 100000, None, a.device_queries_big, a.host_queries_big)]
    for name, Ve, k, qd, qh in settings:
        fn, queries = make(a.vocab, Ve, 300, max(qd, qh))
        run(fn, queries[:min(qd, 64)], True, 1024, k)          # warm-up (engine, library, allocations)
        run(fn, queries[:min(qh, 64)], False, 1024)
        dev = min(run(fn, queries[:qd], True, 1024, k) for _ in range(a.repeats))
        host = min(run(fn, queries[:qh], False, 1024) for _ in range(a.repeats if qh >= 1000 else 1))
        row = dict(setting=name, d=300, V_e=Ve, k=k, window=8, batch=1024, vocab=a.vocab,
                   device_queries=qd, device_s=dev, device_qps=qd / dev,
                   host_queries=qh, host_s=host, host_qps=qh / host, speedup=(qd / dev) / (qh / host))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = dict(device=_capi.device_info(0), results=rows)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
