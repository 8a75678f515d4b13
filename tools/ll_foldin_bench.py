#!/usr/bin/env python
"""Folding new entities into a loglinear model (sert_ll_foldin_*) against the step it replaces: one process, alternating.

    python tools/ll_foldin_bench.py --out profiles/r15_ll_foldin.json

Per setting: the fold-in step through sert_ll_foldin_train_batches (N new columns on top of a frozen loglinear model with V_e
entities) and the full loglinear step through sert_train_batches of a model with V_e + N entities, at the same B, window and
d, on the same Zipfian tokens.  One warm-up pass of each, then --repeats alternations of --steps steps; a time is a host
clock around a call that ends in its one host synchronisation.  The one-time cost of the fold-in's upload
(sert_ll_foldin_upload: host validation and word lists, copies, the logit cache GEMM over the distinct words, the row pass) is
timed apart, with the size of the cache.

With --labels K the same process also times the fold-in step on label ROWS (sert_ll_foldin_upload_csr): K entries per
instance, K // 2 of them on trained columns and the rest on new ones, values 1 / K, on a second handle over the same tokens --
alternating with the other two, so that the row step stands beside the integer-label step of the same process.

With --refresh R the same process also times a handle that REFRESHES R trained columns (sert_ll_foldin_create_refresh: R
refreshed + N new slots) and the plain handle it should equal: sert_ll_foldin_create with R + N new columns on a model that
holds the other V_e - R columns only, initialised with the refreshed columns' trained values.  Both launch the same kernels on
the same shapes and the same numbers; the record says whether their losses came out equal bit for bit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi as C  # noqa: E402

# name, B, V_w, V_e, N, d, window
SETTINGS = [('w3c', 1024, 100000, 715, 64, 300, 8),                  # bench.py's W3C loglinear settings
            ('ve_100000', 1024, 100000, 100000, 64, 300, 8)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def glorot(rng, shape):
    a = np.sqrt(6.0 / sum(shape))
    return rng.uniform(-a, a, size=shape).astype(np.float32)


def engine(rng, B, Vw, Ve, d, n, inference_only=0):
    e = C.Engine(kind=C.KIND_LOGLINEAR, batch_size=B, global_batch_size=B, window_size=n, vocab_size=Vw, num_entities=Ve,
                 word_dim=d, entity_dim=0, num_negatives=0, id_bytes=4, device=0, keep_grads=0, deterministic=1,
                 inference_only=inference_only, lambda_=0.01, lr=1.0, beta1=0.95, beta2=0.0, eps=1e-6, seed=0)
    e.set_tensor(C.T_RW, glorot(rng, (Vw, d)))
    e.set_tensor(C.T_W, glorot(rng, (d, Ve)))
    e.set_tensor(C.T_B, np.zeros(Ve, np.float32))
    return e


def zipf_tokens(rng, Vw, shape):
    return rng.permutation(Vw)[np.minimum(rng.zipf(1.1, size=shape) - 1, Vw - 1)].astype(np.uint32)


def label_rows(rng, M, Ve, N, K):
    """(indptr, indices, data) of M rows with K entries: K // 2 distinct trained columns, then K - K // 2 distinct new ones."""
    kt = K // 2
    kn = K - kt
    assert 0 <= kt <= Ve and 1 <= kn <= N
    # (k distinct sorted columns of V: sorted draws from [0, V - k] plus 0 .. k - 1)
    draw = lambda V, k: np.sort(rng.randint(0, V - k + 1, (M, k)), axis=1) + np.arange(k)
    cols = np.concatenate([draw(Ve, kt), Ve + draw(N, kn)], axis=1).astype(np.int32)
    return np.arange(M + 1, dtype=np.int64) * K, cols.reshape(-1), np.full(M * K, 1.0 / K, np.float32)


def refresh_pair(rng, frozen, B, Vw, Ve, N, d, n, R, X, M):
    """(the refresh handle, the plain handle on the column-deleted model), both with the same upload of slot labels"""
    ids = rng.choice(Ve, R, replace=False).astype(np.int32)
    W, b = frozen.get_tensor(C.T_W, (d, Ve)), frozen.get_tensor(C.T_B, (Ve,))
    Wn = glorot(rng, (d, N))
    keep = np.setdiff1d(np.arange(Ve), ids)
    refresh = C.LlFoldIn(frozen, Wn, None, B, 0.01, refresh_ids=ids)
    deleted = C.Engine(kind=C.KIND_LOGLINEAR, batch_size=1, global_batch_size=1, window_size=n, vocab_size=Vw,
                       num_entities=Ve - R, word_dim=d, entity_dim=0, num_negatives=0, id_bytes=4, device=0, keep_grads=0,
                       deterministic=1, inference_only=1, lambda_=0.01, lr=1.0, beta1=0.95, beta2=0.0, eps=1e-6, seed=0)
    deleted.set_tensor(C.T_RW, frozen.get_tensor(C.T_RW, (Vw, d)))
    deleted.set_tensor(C.T_W, np.ascontiguousarray(W[:, keep]))
    deleted.set_tensor(C.T_B, np.ascontiguousarray(b[keep]))
    plain = C.LlFoldIn(deleted, np.ascontiguousarray(np.concatenate([W[:, ids], Wn], axis=1)),
                       np.concatenate([b[ids], np.zeros(N, np.float32)]), B, 0.01)
    deleted.close()
    y = rng.randint(0, R + N, M).astype(np.int32)
    t_upload, _ = timed(lambda: refresh.upload(X.astype(np.int32), y, None))
    plain.upload(X.astype(np.int32), y, None)
    return refresh, plain, t_upload


def step_setting(name, B, Vw, Ve, N, d, n, steps, repeats, num_batches, labels=0, refresh=0):
    rng = np.random.RandomState(0)
    M = B * num_batches
    X = zipf_tokens(rng, Vw, (M, n))
    full = engine(rng, B, Vw, Ve + N, d, n)
    full.upload_dataset(C.SPLIT_TRAIN, X, y_int=rng.randint(0, Ve + N, M).astype(np.int32), w=np.ones(M, np.float32))
    frozen = engine(rng, 1, Vw, Ve, d, n, inference_only=1)
    fold = C.LlFoldIn(frozen, glorot(rng, (d, N)), None, B, 0.01)
    rows = C.LlFoldIn(frozen, glorot(rng, (d, N)), None, B, 0.01) if labels else None
    pair = refresh_pair(rng, frozen, B, Vw, Ve, N, d, n, refresh, X, M) if refresh else None
    frozen.close()
    t_upload, _ = timed(lambda: fold.upload(X.astype(np.int32), rng.randint(0, N, M).astype(np.int32), None))
    distinct = int(np.unique(X).size)
    order = np.arange(steps, dtype=np.int64) % num_batches
    full.train_batches(order)
    fold.train_batches(order)
    t_fold, t_full, t_rows, t_refresh, t_deleted = [], [], [], [], []
    if pair is not None:
        same_bits = bool(np.array_equal(pair[0].train_batches(order).view(np.uint32), pair[1].train_batches(order).view(np.uint32)))
    if rows is not None:
        indptr, indices, data = label_rows(rng, M, Ve, N, labels)
        t_upload_rows, _ = timed(lambda: rows.upload_csr(X.astype(np.int32), indptr, indices, data, None))
        rows.train_batches(order)
    for _ in range(repeats):
        t_fold.append(timed(lambda: fold.train_batches(order))[0] / steps)
        if rows is not None:
            t_rows.append(timed(lambda: rows.train_batches(order))[0] / steps)
        if pair is not None:
            t_refresh.append(timed(lambda: pair[0].train_batches(order))[0] / steps)
            t_deleted.append(timed(lambda: pair[1].train_batches(order))[0] / steps)
        t_full.append(timed(lambda: full.train_batches(order))[0] / steps)
    full.close()
    fold.close()
    rec = dict(setting=name, B=B, V_w=Vw, V_e=Ve, N=N, d=d, window=n, steps=steps, instances=M,
               foldin_step_ms=[1e3 * t for t in t_fold], full_step_ms=[1e3 * t for t in t_full],
               foldin_step_ms_median=1e3 * float(np.median(t_fold)), full_step_ms_median=1e3 * float(np.median(t_full)),
               foldin_faster_in_every_alternation=bool(all(a < b for a, b in zip(t_fold, t_full))),
               upload_ms=1e3 * t_upload, upload_instances=M, distinct_words=distinct, logit_cache_bytes=distinct * Ve * 4)
    rec['speedup_median'] = rec['full_step_ms_median'] / rec['foldin_step_ms_median']
    if rows is not None:
        rows.close()
        rec.update(labels_per_row=labels, trained_labels_per_row=labels // 2, rows_step_ms=[1e3 * t for t in t_rows],
                   rows_step_ms_median=1e3 * float(np.median(t_rows)), rows_upload_ms=1e3 * t_upload_rows)
        rec['rows_over_integer_median'] = rec['rows_step_ms_median'] / rec['foldin_step_ms_median']
    if pair is not None:
        pair[0].close()
        pair[1].close()
        rec.update(refreshed=refresh, refresh_slots=refresh + N, refresh_frozen_columns=Ve - refresh,
                   refresh_step_ms=[1e3 * t for t in t_refresh], deleted_plain_step_ms=[1e3 * t for t in t_deleted],
                   refresh_step_ms_median=1e3 * float(np.median(t_refresh)),
                   deleted_plain_step_ms_median=1e3 * float(np.median(t_deleted)), refresh_upload_ms=1e3 * pair[2],
                   refresh_logit_cache_bytes=distinct * (Ve - refresh) * 4, refresh_losses_equal_deleted_plain_bitwise=same_bits)
        rec['refresh_over_deleted_plain_median'] = rec['refresh_step_ms_median'] / rec['deleted_plain_step_ms_median']
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--num_batches', type=int, default=8)
    ap.add_argument('--settings', nargs='+', default=[s[0] for s in SETTINGS])
    ap.add_argument('--labels', type=int, default=0,
                    help='K > 0: also time the step on label rows of K entries, K // 2 of them trained (sert_ll_foldin_upload_csr)')
    ap.add_argument('--refresh', type=int, default=0,
                    help='R > 0: also time a handle that refreshes R trained columns (R + N slots) and the plain handle with R + N '
                         'new columns on the column-deleted model (sert_ll_foldin_create_refresh)')
    args = ap.parse_args(argv)
    C.require_gpu()
    out = dict(device=C.device_info(0), steps=[])
    for s in SETTINGS:
        if s[0] in args.settings:
            rec = step_setting(*s, steps=args.steps, repeats=args.repeats, num_batches=args.num_batches, labels=args.labels,
                               refresh=args.refresh)
            print(json.dumps(rec))
            out['steps'].append(rec)
            with open(args.out, 'w') as f:
                json.dump(out, f, indent=1, sort_keys=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    sys.exit(main())
