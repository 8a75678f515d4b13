#!/usr/bin/env python
"""Full rankings of the cosine scorer (bin/query.py --type vectorspace with --top unset or above 1024): the device path
(Scorer.rank -> sert_scorer_rank) against the host ordering it replaces (Scorer.rank(..., on_device=False): every cosine over
PCIe + a stable argsort per query), one process, one scorer per shape, the two alternating; queries/s of each.

    python tools/score_rank_bench.py --out profiles/r09_score_rank.json

Per shape one warm-up call of each path, then --repeats alternations (device, host, device, host, ...); the record holds
every time, the medians, the path that ran (rows per path from sert_debug_scorer_rank_counts) and, for the two sorts, the
share of the device call's time its copies to the host took on the second stream (events around them; the top-k path
copies inside sert_scorer_topk and has no such figure).
Gaussian entity table, tanh(Gaussian) projections, as bench.py's query workload.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi  # noqa: E402

SHAPES = [('w3c_all', 715, 128, 10000, None),            # depth 715 <= 1024: the top-k path (sert_scorer_topk's kernels)
          ('lds4096_all', 4096, 128, 5000, None),        # the LDS sort, every slot used
          ('lds8192_all', 8192, 128, 5000, None),        # ... at its largest: 64 KiB of LDS per query
          ('lds8192_k2000', 8192, 128, 5000, 2000),
          ('products_all', 32768, 128, 1000, None),      # the product-search table: counting-sort passes, exact_dot32 slab
          ('ve100k_all', 100000, 128, 2000, None),
          ('ve100k_k2000', 100000, 128, 2000, 2000)]
PATHS = ('topk', 'lds', 'csort')                         # sert_debug_scorer_rank_counts[2:5]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default=None, help='comma-separated shape names')
    a = ap.parse_args()
    rows = []
    for name, V, d, Q, k in SHAPES:
        if a.only and name not in a.only.split(','):
            continue
        rng = np.random.RandomState(7)
        E = rng.randn(V, d).astype(np.float32)
        P = np.tanh(rng.randn(Q, d)).astype(np.float32)
        sc = _capi.Scorer(E)
        _, dev = timed(lambda: sc.rank(P, k))                              # warm-up: allocations, first touch of the result arrays
        _, host = timed(lambda: sc.rank(P, k, on_device=False))
        same = bool(np.array_equal(dev[0], host[0]) and np.array_equal(dev[1].view(np.uint32), host[1].view(np.uint32)))
        del dev, host
        dev_s, host_s, copy_s = [], [], []
        for r in range(a.repeats):
            c0 = sc.debug_rank_counts()
            t, _ = timed(lambda: sc.rank(P, k))
            c1 = sc.debug_rank_counts()
            dev_s.append(t)
            copy_s.append((c1[5] - c0[5]) * 1e-6)
            t, _ = timed(lambda: sc.rank(P, k, on_device=False))
            host_s.append(t)
            print(json.dumps(dict(setting=name, alternation=r, device_s=dev_s[-1], host_s=host_s[-1], copy_out_s=copy_s[-1])),
                  flush=True)
        chunks = c1[1] - c0[1]
        path_rows = {n: c1[2 + i] - c0[2 + i] for i, n in enumerate(PATHS)}
        path = [n for n in PATHS if path_rows[n]]
        sc.close()
        md, mh = float(np.median(dev_s)), float(np.median(host_s))
        row = dict(setting=name, V_e=V, d=d, queries=Q, k=k, identical=same, chunks_per_call=chunks, path=path[0] if len(path) == 1 else path,
                   rows_per_path_per_call=path_rows,
                   device_s=dev_s, host_s=host_s, device_median_s=md, host_median_s=mh, device_qps=Q / md, host_qps=Q / mh,
                   speedup=mh / md, copy_out_share=None if path == ['topk'] else float(np.median(np.array(copy_s) / np.array(dev_s))),
                   device_faster_in_every_alternation=bool(all(x < y for x, y in zip(dev_s, host_s))))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = dict(device=_capi.device_info(0), results=rows)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
