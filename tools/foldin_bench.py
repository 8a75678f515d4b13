#!/usr/bin/env python
"""Folding new entities in (sert_foldin_*) against the step it replaces: one process, the two alternating, medians.

    python tools/foldin_bench.py --out profiles/r13_foldin.json

Per setting: the fold-in step through sert_foldin_train_batches (N new rows on top of a frozen model with V_e entities)
and the full vectorspace step through sert_train_batches of a model with V_e + N entities, at the same B, z, d_w, d_e and
window, device-drawn negatives both.  One warm-up pass of each, then --repeats alternations of --steps steps; a time is a
host clock around a call that ends in its one host synchronisation.  The one-time projection of the fold-in instances
(sert_foldin_upload: host validation, copy, window mean, GEMM) is timed apart.

--refresh R (`python tools/foldin_bench.py --refresh 1024 --out profiles/r14_refresh.json`): per setting, in place of the
two-way alternation and the end-to-end figure, the REFRESH step -- sert_foldin_create_refresh with R trained rows refreshed and no new entity, whose
loss kernel looks every negative up in a slot table -- alternating in the same process with the fold-in step of
sert_foldin_create with N new rows and with the full step; the ratio reported is refresh / fold-in.

The end-to-end figure (--e2e_epochs K > 0): K epochs of fold-in of N entities x --e2e_instances instances against K
epochs of training on the union set ((V_e + N) x --e2e_instances instances), uploads included, at the first setting.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import _capi as C  # noqa: E402

# name, B, V_w, V_e, N, d_w, d_e, window, z
SETTINGS = [('product_search', 4096, 65536, 32768, 1024, 300, 128, 4, 10),      # product-search.sh:109, :126-131
            ('c2_b65536', 65536, 100000, 1000, 1024, 128, 128, 10, 10)]         # bench.py's flagship dimensions


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def glorot(rng, shape):
    a = np.sqrt(6.0 / sum(shape))
    return rng.uniform(-a, a, size=shape).astype(np.float32)


def engine(rng, B, Vw, Ve, dw, de, n, z, inference_only=0):
    e = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=B, global_batch_size=B, window_size=n, vocab_size=Vw, num_entities=Ve,
                 word_dim=dw, entity_dim=de, num_negatives=z, id_bytes=4, device=0, keep_grads=0, deterministic=1,
                 inference_only=inference_only, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=7)
    e.set_tensor(C.T_RW, glorot(rng, (Vw, dw)))
    e.set_tensor(C.T_RE, glorot(rng, (Ve, de)))
    e.set_tensor(C.T_W, glorot(rng, (dw, de)))
    e.set_tensor(C.T_B, np.zeros(de, np.float32))
    return e


def zipf_tokens(rng, Vw, shape):
    return rng.permutation(Vw)[np.minimum(rng.zipf(1.1, size=shape) - 1, Vw - 1)].astype(np.uint32)


def step_setting(name, B, Vw, Ve, N, dw, de, n, z, steps, repeats, num_batches):
    rng = np.random.RandomState(0)
    M = B * num_batches
    X = zipf_tokens(rng, Vw, (M, n))
    full = engine(rng, B, Vw, Ve + N, dw, de, n, z)
    full.upload_dataset(C.SPLIT_TRAIN, X, y_int=rng.randint(0, Ve + N, M).astype(np.int32), w=np.ones(M, np.float32))
    frozen = engine(rng, 1, Vw, Ve, dw, de, n, 0, inference_only=1)
    fold = C.FoldIn(frozen, glorot(rng, (N, de)), B, z, 0.01, lr=1e-3, seed=7)
    frozen.close()
    t_upload, _ = timed(lambda: fold.upload(X.astype(np.int32), rng.randint(0, N, M).astype(np.int32), None))
    order = np.arange(steps, dtype=np.int64) % num_batches
    full.train_batches(order)
    fold.train_batches(order)
    t_fold, t_full = [], []
    for _ in range(repeats):
        t_fold.append(timed(lambda: fold.train_batches(order))[0] / steps)
        t_full.append(timed(lambda: full.train_batches(order))[0] / steps)
    full.close()
    fold.close()
    rec = dict(setting=name, B=B, V_w=Vw, V_e=Ve, N=N, d_w=dw, d_e=de, window=n, z=z, steps=steps, instances=M,
               foldin_step_ms=[1e3 * t for t in t_fold], full_step_ms=[1e3 * t for t in t_full],
               foldin_step_ms_median=1e3 * float(np.median(t_fold)), full_step_ms_median=1e3 * float(np.median(t_full)),
               foldin_faster_in_every_alternation=bool(all(a < b for a, b in zip(t_fold, t_full))),
               projection_upload_ms=1e3 * t_upload, projection_upload_instances=M)
    rec['speedup_median'] = rec['full_step_ms_median'] / rec['foldin_step_ms_median']
    return rec


def refresh_setting(name, B, Vw, Ve, N, dw, de, n, z, steps, repeats, num_batches, R):
    """The refresh step (R refreshed trained rows, num_new = 0), the fold-in step of sert_foldin_create (N new rows) and the
    full step (V_e + N entities), alternating."""
    rng = np.random.RandomState(0)
    R = min(R, Ve)          # (a setting with fewer trained rows than R: every one of them is refreshed)
    M = B * num_batches
    X = zipf_tokens(rng, Vw, (M, n))
    full = engine(rng, B, Vw, Ve + N, dw, de, n, z)
    full.upload_dataset(C.SPLIT_TRAIN, X, y_int=rng.randint(0, Ve + N, M).astype(np.int32), w=np.ones(M, np.float32))
    frozen = engine(rng, 1, Vw, Ve, dw, de, n, 0, inference_only=1)
    fold = C.FoldIn(frozen, glorot(rng, (N, de)), B, z, 0.01, lr=1e-3, seed=7)
    refresh = C.FoldIn(frozen, None, B, z, 0.01, lr=1e-3, seed=7,
                       refresh_ids=rng.permutation(Ve)[:R].astype(np.int32))
    frozen.close()
    assert refresh.table() == dict(map=True, num_refresh=R, num_new=0, rows=R) and not fold.table()['map']
    fold.upload(X.astype(np.int32), rng.randint(0, N, M).astype(np.int32), None)
    refresh.upload(X.astype(np.int32), rng.randint(0, R, M).astype(np.int32), None)
    order = np.arange(steps, dtype=np.int64) % num_batches
    handles = (('refresh', refresh), ('foldin', fold), ('full', full))
    for _, h in handles:
        h.train_batches(order)
    times = dict((k, []) for k, _ in handles)
    for _ in range(repeats):
        for k, h in handles:
            times[k].append(timed(lambda: h.train_batches(order))[0] / steps)
    plans = dict(refresh=refresh.plan(), foldin=fold.plan())
    for _, h in handles:
        h.close()
    rec = dict(setting=name, B=B, V_w=Vw, V_e=Ve, R=R, N=N, d_w=dw, d_e=de, window=n, z=z, steps=steps, instances=M, plans=plans)
    for k in times:
        rec[k + '_step_ms'] = [1e3 * t for t in times[k]]
        rec[k + '_step_ms_median'] = 1e3 * float(np.median(times[k]))
    rec['refresh_over_foldin_median'] = rec['refresh_step_ms_median'] / rec['foldin_step_ms_median']
    rec['full_over_refresh_median'] = rec['full_step_ms_median'] / rec['refresh_step_ms_median']
    return rec


def end_to_end(name, B, Vw, Ve, N, dw, de, n, z, epochs, per_entity):
    rng = np.random.RandomState(1)

    def fold_run():
        M = N * per_entity
        X = zipf_tokens(rng, Vw, (M, n)).astype(np.int32)
        y = rng.permutation(np.repeat(np.arange(N, dtype=np.int32), per_entity))
        frozen = engine(rng, 1, Vw, Ve, dw, de, n, 0, inference_only=1)
        t0 = time.perf_counter()
        fold = C.FoldIn(frozen, glorot(rng, (N, de)), B, z, 0.01, lr=1e-3, seed=7)
        fold.upload(X, y, None)
        t_setup = time.perf_counter() - t0
        nb = fold.num_batches()
        t0 = time.perf_counter()
        for _ in range(epochs):
            fold.train_batches(rng.permutation(nb).astype(np.int64))
        t_train = time.perf_counter() - t0
        fold.close()
        frozen.close()
        return dict(instances=M, batches_per_epoch=nb, setup_s=t_setup, epochs_s=t_train)

    def union_run():
        M = (Ve + N) * per_entity
        X = zipf_tokens(rng, Vw, (M, n))
        y = rng.permutation(np.repeat(np.arange(Ve + N, dtype=np.int32), per_entity))
        full = engine(rng, B, Vw, Ve + N, dw, de, n, z)
        t0 = time.perf_counter()
        full.upload_dataset(C.SPLIT_TRAIN, X, y_int=y, w=np.ones(M, np.float32))
        t_setup = time.perf_counter() - t0
        nb = M // B
        t0 = time.perf_counter()
        for _ in range(epochs):
            full.train_batches(rng.permutation(nb).astype(np.int64))
        t_train = time.perf_counter() - t0
        full.close()
        return dict(instances=M, batches_per_epoch=nb, setup_s=t_setup, epochs_s=t_train)

    fold, union = fold_run(), union_run()
    return dict(setting=name, epochs=epochs, instances_per_entity=per_entity, foldin=fold, union_training=union,
                speedup_epochs=union['epochs_s'] / fold['epochs_s'],
                speedup_with_setup=(union['epochs_s'] + union['setup_s']) / (fold['epochs_s'] + fold['setup_s']))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--num_batches', type=int, default=8)
    ap.add_argument('--e2e_epochs', type=int, default=2)
    ap.add_argument('--e2e_instances', type=int, default=256)
    ap.add_argument('--refresh', type=int, default=0, metavar='R',
                    help='also time the refresh step with R refreshed trained rows and no new entity (0: not)')
    ap.add_argument('--settings', nargs='+', default=[s[0] for s in SETTINGS])
    args = ap.parse_args(argv)
    C.require_gpu()
    out = dict(device=C.device_info(0), steps=[], end_to_end=None)
    if args.refresh > 0:
        out['refresh'] = []
    for s in SETTINGS:
        if s[0] in args.settings and args.refresh > 0:
            rec = refresh_setting(*s, steps=args.steps, repeats=args.repeats, num_batches=args.num_batches, R=args.refresh)
            print(json.dumps(rec))
            out['refresh'].append(rec)
        elif s[0] in args.settings:
            rec = step_setting(*s, steps=args.steps, repeats=args.repeats, num_batches=args.num_batches)
            print(json.dumps(rec))
            out['steps'].append(rec)
            with open(args.out, 'w') as f:
                json.dump(out, f, indent=1, sort_keys=True)
    if args.e2e_epochs > 0 and args.refresh == 0 and SETTINGS[0][0] in args.settings:
        out['end_to_end'] = end_to_end(*SETTINGS[0], epochs=args.e2e_epochs, per_entity=args.e2e_instances)
        print(json.dumps(out['end_to_end']))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    sys.exit(main())
