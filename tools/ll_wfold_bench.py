#!/usr/bin/env python
"""Folding new WORDS into a loglinear model (sert_ll_wfold_*) against the step it replaces: one process, alternating, medians.

    python tools/ll_wfold_bench.py --out profiles/r21_ll_wfold.json

Per setting: the word fold-in step through sert_ll_wfold_train_batches (Nw new word rows on top of a frozen loglinear model
with V_w words) and the full loglinear step through sert_train_batches of a model with V_w + Nw words, at the same B, window,
d and V_e, on the same tokens.  Tokens are Zipfian over the trained words; one or two positions of every window (one with
probability 1/2) hold a new word, uniform over the Nw -- the record states the share of new positions.  One warm-up pass of
each, then --repeats alternations of --steps steps; a time is a host clock around a call that ends in its one host
synchronisation.  The one-time upload of the fold-in (sert_ll_wfold_upload: host validation, the inverted index, copies, the
frozen table -- gather, GEMM and log-softmax over the distinct frozen words) is timed apart, with the size of the table.

    python tools/ll_wfold_bench.py --labels 8 --out profiles/r22_ll_wfold_rows.json

--labels K: label ROWS (sert_ll_wfold_upload_csr) of K distinct trained entries of value 1 / K per instance.  Three steps
alternate in the one process: the fold-in on the rows, the fold-in of a second handle on the integer labels y (the first
column of every row), and the step the rows fold-in replaces -- sert_train_batches of the full model with V_w + Nw words
trained on the same CSR rows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi as C  # noqa: E402

# name, B, V_w, V_e, Nw, d, window
SETTINGS = [('w3c', 1024, 100000, 715, 1024, 300, 8),                  # bench.py's W3C loglinear settings
            ('ve_100000', 1024, 100000, 100000, 1024, 300, 8)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def glorot(rng, shape):
    a = np.sqrt(6.0 / sum(shape))
    return rng.uniform(-a, a, size=shape).astype(np.float32)


def engine(B, Rw, W, n, inference_only=0):
    Vw, d = Rw.shape
    e = C.Engine(kind=C.KIND_LOGLINEAR, batch_size=B, global_batch_size=B, window_size=n, vocab_size=Vw, num_entities=W.shape[1],
                 word_dim=d, entity_dim=0, num_negatives=0, id_bytes=4, device=0, keep_grads=0, deterministic=1,
                 inference_only=inference_only, lambda_=0.01, lr=1.0, beta1=0.95, beta2=0.0, eps=1e-6, seed=0)
    e.set_tensor(C.T_RW, Rw)
    e.set_tensor(C.T_W, W)
    e.set_tensor(C.T_B, np.zeros(W.shape[1], np.float32))
    return e


def tokens(rng, Vw, Nw, M, n):
    """Zipfian trained words; one or two positions per window hold a new word."""
    X = rng.permutation(Vw)[np.minimum(rng.zipf(1.1, size=(M, n)) - 1, Vw - 1)].astype(np.int32)
    rows = np.arange(M)
    first = rng.randint(0, n, M)
    X[rows, first] = Vw + rng.randint(0, Nw, M)
    two = rng.rand(M) < 0.5
    second = (first + 1 + rng.randint(0, n - 1, M)) % n
    X[rows[two], second[two]] = Vw + rng.randint(0, Nw, int(two.sum()))
    return X


def label_rows(rng, M, Ve, K):
    """(M, Ve) canonical CSR: K distinct columns per row -- a random start, then V_e // K apart, modulo V_e, ascending -- of
    value 1 / K."""
    cols = (rng.randint(0, Ve, M)[:, None] + (Ve // K) * np.arange(K)[None, :]) % Ve
    cols = np.sort(cols, axis=1).astype(np.int32)
    assert (np.diff(cols, axis=1) > 0).all()
    return scipy.sparse.csr_matrix((np.full(M * K, 1.0 / K, np.float32), cols.reshape(-1), np.arange(0, M * K + 1, K)),
                                   shape=(M, Ve))


def rows_setting(name, B, Vw, Ve, Nw, d, n, steps, repeats, num_batches, K):
    """--labels K: the rows fold-in, the integer fold-in and the full model on the rows, alternating."""
    rng = np.random.RandomState(0)
    M = B * num_batches
    X = tokens(rng, Vw, Nw, M, n)
    Y = label_rows(rng, M, Ve, K)
    y = Y.indices[::K].copy()
    Rw = glorot(rng, (Vw + Nw, d))
    W = glorot(rng, (d, Ve))
    full = engine(B, Rw, W, n)
    full.upload_dataset(C.SPLIT_TRAIN, X.astype(np.uint32), csr=Y, w=np.ones(M, np.float32))
    frozen = engine(1, Rw[:Vw], W, n, inference_only=1)
    rows = C.LlWordFoldIn(frozen, Rw[Vw:], B, 0.01)
    ints = C.LlWordFoldIn(frozen, Rw[Vw:], B, 0.01)
    frozen.close()
    t_upload_rows, _ = timed(lambda: rows.upload_csr(X, Y.indptr, Y.indices, Y.data, None))
    t_upload_int, _ = timed(lambda: ints.upload(X, y, None))
    order = np.arange(steps, dtype=np.int64) % num_batches
    for h in (rows, ints, full):
        h.train_batches(order)
    t_rows, t_int, t_full = [], [], []
    for _ in range(repeats):
        t_rows.append(timed(lambda: rows.train_batches(order))[0] / steps)
        t_int.append(timed(lambda: ints.train_batches(order))[0] / steps)
        t_full.append(timed(lambda: full.train_batches(order))[0] / steps)
    plan_rows, plan_int = rows.plan(), ints.plan()
    for h in (full, rows, ints):
        h.close()
    med = lambda t: 1e3 * float(np.median(t))
    rec = dict(setting=name, B=B, V_w=Vw, V_e=Ve, Nw=Nw, d=d, window=n, steps=steps, instances=M, labels_per_row=K,
               label_entries=int(Y.nnz), new_position_share=float((X >= Vw).mean()), plan_rows=plan_rows, plan_int=plan_int,
               rows_step_ms=[1e3 * t for t in t_rows], int_step_ms=[1e3 * t for t in t_int],
               full_rows_step_ms=[1e3 * t for t in t_full], rows_step_ms_median=med(t_rows), int_step_ms_median=med(t_int),
               full_rows_step_ms_median=med(t_full), upload_rows_ms=1e3 * t_upload_rows, upload_int_ms=1e3 * t_upload_int)
    rec['rows_over_int_median'] = rec['rows_step_ms_median'] / rec['int_step_ms_median']
    rec['speedup_over_full_median'] = rec['full_rows_step_ms_median'] / rec['rows_step_ms_median']
    rec['rows_faster_than_full_in_every_alternation'] = bool(all(a < b for a, b in zip(t_rows, t_full)))
    return rec


def step_setting(name, B, Vw, Ve, Nw, d, n, steps, repeats, num_batches):
    rng = np.random.RandomState(0)
    M = B * num_batches
    X = tokens(rng, Vw, Nw, M, n)
    y = rng.randint(0, Ve, M).astype(np.int32)
    Rw = glorot(rng, (Vw + Nw, d))
    W = glorot(rng, (d, Ve))
    full = engine(B, Rw, W, n)
    full.upload_dataset(C.SPLIT_TRAIN, X.astype(np.uint32), y_int=y, w=np.ones(M, np.float32))
    frozen = engine(1, Rw[:Vw], W, n, inference_only=1)
    fold = C.LlWordFoldIn(frozen, Rw[Vw:], B, 0.01)
    frozen.close()
    t_upload, _ = timed(lambda: fold.upload(X, y, None))
    distinct = int(np.unique(X[X < Vw]).size)
    order = np.arange(steps, dtype=np.int64) % num_batches
    full.train_batches(order)
    fold.train_batches(order)
    t_fold, t_full = [], []
    for _ in range(repeats):
        t_fold.append(timed(lambda: fold.train_batches(order))[0] / steps)
        t_full.append(timed(lambda: full.train_batches(order))[0] / steps)
    plan = fold.plan()
    full.close()
    fold.close()
    rec = dict(setting=name, B=B, V_w=Vw, V_e=Ve, Nw=Nw, d=d, window=n, steps=steps, instances=M,
               new_position_share=float((X >= Vw).mean()), plan=plan,
               ll_wfold_step_ms=[1e3 * t for t in t_fold], full_step_ms=[1e3 * t for t in t_full],
               ll_wfold_step_ms_median=1e3 * float(np.median(t_fold)), full_step_ms_median=1e3 * float(np.median(t_full)),
               ll_wfold_faster_in_every_alternation=bool(all(a < b for a, b in zip(t_fold, t_full))),
               upload_ms=1e3 * t_upload, upload_instances=M, distinct_frozen_words=distinct, frozen_table_bytes=distinct * Ve * 4)
    rec['speedup_median'] = rec['full_step_ms_median'] / rec['ll_wfold_step_ms_median']
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--num_batches', type=int, default=8)
    ap.add_argument('--settings', nargs='+', default=[s[0] for s in SETTINGS])
    ap.add_argument('--labels', type=int, default=0,
                    help='K > 0: label rows of K trained entries of value 1 / K (sert_ll_wfold_upload_csr) beside the integer '
                         'upload and the full model on the same rows; 0: integer labels against the full model')
    args = ap.parse_args(argv)
    C.require_gpu()
    out = dict(device=C.device_info(0), steps=[])
    for s in SETTINGS:
        if s[0] in args.settings:
            if args.labels > 0:
                rec = rows_setting(*s, steps=args.steps, repeats=args.repeats, num_batches=args.num_batches, K=args.labels)
            else:
                rec = step_setting(*s, steps=args.steps, repeats=args.repeats, num_batches=args.num_batches)
            print(json.dumps(rec))
            out['steps'].append(rec)
            with open(args.out, 'w') as f:
                json.dump(out, f, indent=1, sort_keys=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
