#!/usr/bin/env python
"""Re-ranking per-query candidate lists (bin/query.py --candidates): the device call (Scorer.rank_candidates ->
sert_scorer_rank_candidates) against the route that exists without it -- Scorer.rank(P, None), every entity ranked on the
device and copied to the host, then filtered to the candidate set there -- one process, one scorer per setting, the two
alternating; topics/s of each.

    python tools/rerank_bench.py --out profiles/r11_rerank.json

Per setting one warm-up call of each route, then --repeats alternations (candidates, full, candidates, full, ...); the record
holds every time, the medians, which kernel ranked the lists (sert_debug_scorer_rerank_counts) and the time of
Scorer.score_pairs on the same lists -- the pair kernel with its copies, priced as a row gather (bytes of table rows per
second).  Both tables are bf16-prefiltered (V_e >= 32768), where the two routes agree bit for bit: that is asserted, not
reported.  Gaussian entity table, tanh(Gaussian) projections, as bench.py's query workload; candidates drawn uniformly.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi  # noqa: E402

SETTINGS = [('products_100', 32768, 128, 1000, 100),     # the product-search table, a short and a long first-stage list
            ('products_1000', 32768, 128, 1000, 1000),
            ('c5_1000', 100000, 128, 10000, 1000)]       # bench.py's C5 query workload


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def draw_candidates(rng, V, topics, n):
    """Per topic n distinct entities, uniformly drawn, ascending int32."""
    lists = []
    for _ in range(topics):
        u = np.unique(rng.randint(0, V, size=n + n // 16 + 8))
        assert len(u) >= n
        lists.append(u[np.sort(rng.permutation(len(u))[:n])].astype(np.int32))
    return lists


def full_route(sc, P, lists):
    """Scorer.rank(P, None), then per topic the entities of its list, in ranking order.  (seconds ranking, seconds filtering,
    the lists of (idx, val))."""
    t_rank, (idx, val) = timed(lambda: sc.rank(P, None))
    t0 = time.perf_counter()
    out = []
    member = np.zeros(sc.num_entities, dtype=bool)
    for q, lst in enumerate(lists):
        member[lst] = True
        keep = member[idx[q]]
        out.append((idx[q][keep], val[q][keep]))
        member[lst] = False
    return t_rank, time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default=None, help='comma-separated setting names')
    a = ap.parse_args()
    rows = []
    for name, V, d, Q, n in SETTINGS:
        if a.only and name not in a.only.split(','):
            continue
        rng = np.random.RandomState(7)
        E = rng.randn(V, d).astype(np.float32)
        P = np.tanh(rng.randn(Q, d)).astype(np.float32)
        lists = draw_candidates(rng, V, Q, n)
        sc = _capi.Scorer(E)
        _, (at, idx, val) = timed(lambda: sc.rank_candidates(P, lists))       # warm-up: allocations
        _, _, full = full_route(sc, P, lists)
        for q, (fidx, fval) in enumerate(full):
            assert np.array_equal(idx[at[q]:at[q + 1]], fidx), (name, q)
            assert np.array_equal(val[at[q]:at[q + 1]].view(np.uint32), fval.view(np.uint32)), (name, q)
        del full
        sc.score_pairs(P, lists, raw=True)
        cand_s, full_s, rank_s, filter_s, pairs_s = [], [], [], [], []
        for r in range(a.repeats):
            c0 = sc.debug_rerank_counts()
            t, _ = timed(lambda: sc.rank_candidates(P, lists))
            c1 = sc.debug_rerank_counts()
            cand_s.append(t)
            t_rank, t_filter, _ = full_route(sc, P, lists)
            rank_s.append(t_rank)
            filter_s.append(t_filter)
            full_s.append(t_rank + t_filter)
            t, _ = timed(lambda: sc.score_pairs(P, lists, raw=True))
            pairs_s.append(t)
            print(json.dumps(dict(setting=name, alternation=r, candidates_s=cand_s[-1], full_s=full_s[-1], full_rank_s=t_rank,
                                  full_filter_s=t_filter, score_pairs_s=pairs_s[-1])), flush=True)
        sc.close()
        mc, mf, mp = float(np.median(cand_s)), float(np.median(full_s)), float(np.median(pairs_s))
        pairs = Q * n
        row = dict(setting=name, V_e=V, d=d, topics=Q, candidates_per_topic=n, identical=True,
                   chunks_per_call=c1[1] - c0[1], lds_queries_per_call=c1[2] - c0[2], slab_queries_per_call=c1[3] - c0[3],
                   candidates_s=cand_s, full_s=full_s, full_rank_s=rank_s, full_filter_s=filter_s, score_pairs_s=pairs_s,
                   candidates_median_s=mc, full_median_s=mf, full_rank_median_s=float(np.median(rank_s)),
                   candidates_topics_per_s=Q / mc, full_topics_per_s=Q / mf, speedup=mf / mc,
                   speedup_over_the_ranking_alone=float(np.median(rank_s)) / mc, work_ratio=V / float(n),
                   score_pairs_median_s=mp, score_pairs_row_gather_gb_per_s=pairs * d * 4 / mp / 1e9,
                   candidates_faster_in_every_alternation=bool(all(x < y for x, y in zip(cand_s, full_s))))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = dict(device=_capi.device_info(0), results=rows)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
