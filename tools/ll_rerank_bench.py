#!/usr/bin/env python
"""Re-ranking candidate lists with the loglinear model (bin/query.py --candidates): LogLinearPredictFn.rank_queries(candidates=...)
(sert_ll_rank_candidates: only the listed entities are sorted and copied out) against the route that exists without it --
rank_queries(k=None), every entity of every topic ranked on the device and copied to the host, then np.isin per topic, as
LogLinearCallback._report filters -- one process, one model per setting, the two alternating; topics/s of each.

    python tools/ll_rerank_bench.py --out profiles/r12_ll_rerank.json

Per setting one warm-up call of each route (the results of the two are compared, list by list, index for index and score bit
for score bit: asserted there and in every alternation, not reported), then --repeats alternations (candidates, full,
candidates, full, ...).  The record holds every time, the medians, what the candidate call did (sert_debug_ll_rerank_counts:
chunks, lists per kernel) and the time of the device call alone (Engine.ll_rank_candidates on lists made CSR-clean beforehand,
without the per-topic slicing of rank_queries).  Settings: the W3C query setting (d = 300, V_e = 715, 10 000 queries of 1-6
tokens, 100 candidates) and V_e = 100 000 (2 000 queries x 100 and x 1 000 candidates); uniform word table, Gaussian output
layer, candidates drawn uniformly, as tools/ll_query_bench.py and tools/rerank_bench.py draw theirs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi, models  # noqa: E402

SETTINGS = [('w3c_100', 715, 10000, 100),
            ('ve100k_100', 100000, 2000, 100),
            ('ve100k_1000', 100000, 2000, 1000)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def make(Vw, Ve, d, Q, seed=0):
    rng = np.random.RandomState(seed)
    fn = models.LogLinearPredictFn(R_w=rng.uniform(-0.5, 0.5, (Vw, d)).astype(np.float32),
                                   W=(rng.standard_normal((d, Ve)) * 0.25).astype(np.float32),
                                   b=np.zeros(Ve, np.float32), window_size=8)
    return fn, [list(rng.randint(0, Vw, rng.randint(1, 7))) for _ in range(Q)], rng


def draw_candidates(rng, V, topics, n):
    """Per topic n distinct entities, uniformly drawn, ascending int32."""
    return [np.sort(rng.choice(V, size=n, replace=False)).astype(np.int32) for _ in range(topics)]


def full_route(fn, queries, lists):
    """rank_queries(k=None), then per topic np.isin against its list.  (seconds ranking, seconds filtering, [(idx, score)])."""
    t_rank, r = timed(lambda: fn.rank_queries(queries, k=None))
    t0 = time.perf_counter()
    out = []
    for q, lst in enumerate(lists):
        keep = np.isin(r.idx[q], lst)
        out.append((r.idx[q][keep], r.score[q][keep]))
    return t_rank, time.perf_counter() - t0, out, r


def candidate_route(fn, queries, lists):
    t, r = timed(lambda: fn.rank_queries(queries, k=None, candidates=lists))
    return t, [(r.idx[q], r.score[q]) for q in range(len(queries))], r


def assert_identical(name, cand, full, rc, rf):
    for q, ((ci, cs), (fi, fs)) in enumerate(zip(cand, full)):
        assert np.array_equal(ci, fi), (name, q)
        assert np.array_equal(cs.view(np.uint32), fs.view(np.uint32)), (name, q)
    assert np.array_equal(rc.status, rf.status) and not rc.status.any(), name
    assert np.array_equal(rc.joint_entropy.view(np.uint32), rf.joint_entropy.view(np.uint32)), name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--vocab', type=int, default=20000)
    ap.add_argument('--only', default=None, help='comma-separated setting names')
    a = ap.parse_args()
    rows = []
    for name, Ve, Q, n in SETTINGS:
        if a.only and name not in a.only.split(','):
            continue
        fn, queries, rng = make(a.vocab, Ve, 300, Q)
        lists = draw_candidates(rng, Ve, Q, n)
        _, cand, rc = candidate_route(fn, queries, lists)              # warm-up: allocations, the engine
        _, _, full, rf = full_route(fn, queries, lists)
        assert_identical(name, cand, full, rc, rf)
        eng = fn._engine
        cand_s, full_s, rank_s, filter_s, call_s = [], [], [], [], []
        for r in range(a.repeats):
            c0 = _capi.debug_ll_rerank_counts()
            t, cand, rc = candidate_route(fn, queries, lists)
            c1 = _capi.debug_ll_rerank_counts()
            cand_s.append(t)
            t_rank, t_filter, full, rf = full_route(fn, queries, lists)
            assert_identical(name, cand, full, rc, rf)
            del cand, full, rc, rf
            rank_s.append(t_rank)
            filter_s.append(t_filter)
            full_s.append(t_rank + t_filter)
            t, _ = timed(lambda: eng.ll_rank_candidates(queries, lists))
            call_s.append(t)
            print(json.dumps(dict(setting=name, alternation=r, candidates_s=cand_s[-1], full_s=full_s[-1], full_rank_s=t_rank,
                                  full_filter_s=t_filter, device_call_s=call_s[-1])), flush=True)
        mc, mf = float(np.median(cand_s)), float(np.median(full_s))
        row = dict(setting=name, V_e=Ve, d=300, vocab=a.vocab, topics=Q, candidates_per_topic=n, identical=True,
                   chunks_per_call=c1[1] - c0[1], lds_lists_per_call=c1[2] - c0[2], slab_lists_per_call=c1[3] - c0[3],
                   empty_lists_per_call=c1[4] - c0[4],
                   candidates_s=cand_s, full_s=full_s, full_rank_s=rank_s, full_filter_s=filter_s, device_call_s=call_s,
                   candidates_median_s=mc, full_median_s=mf, full_rank_median_s=float(np.median(rank_s)),
                   device_call_median_s=float(np.median(call_s)),
                   candidates_topics_per_s=Q / mc, full_topics_per_s=Q / mf, speedup=mf / mc,
                   speedup_over_the_ranking_alone=float(np.median(rank_s)) / mc, work_ratio=Ve / float(n),
                   candidates_faster_in_every_alternation=bool(all(x < y for x, y in zip(cand_s, full_s))))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del fn, eng
    out = dict(device=_capi.device_info(0), results=rows)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
