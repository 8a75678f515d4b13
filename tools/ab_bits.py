#!/usr/bin/env python
"""Bit-for-bit A/B of two builds of the library over tiny problems that reach every loss kernel family.

    python tools/ab_bits.py --lib sert_amd/variants/libsert_parent.so --out parent.npz
    python tools/ab_bits.py --out change.npz --against parent.npz

Each problem runs two training steps and both evaluations (a fold-in: two steps and one evaluation) and records the losses,
the row losses, every parameter, gradient and optimiser moment, the fold-in rows, and the form the engine reports it
took.  The entity-chain group runs two steps of every case of tests/egrad_key_cases.py (the sorted cases and, through the
sort as well as on their own path, the bucket cases), tests/foldin_key_cases.py and tests/refresh_cases.py, and records dR_e
after each step, or the fold-in's E, m and v, with the losses and the plan of the sorted chain (eg_plan, FoldIn.plan()).  The
fold-ins group runs every case of tests/ll_foldin_cases.py, tests/ll_foldin_label_cases.py, tests/ll_refresh_cases.py and
tests/wfold_cases.py, and through LlWordFoldIn every case of tests/ll_wfold_cases.py (integer labels) and
tests/ll_wfold_rows_cases.py (label rows): two train_batch steps, one train_batches call over two batches and one eval_batch,
with the losses and every trainable tensor and accumulator after each; a vectorspace word fold-in once on the case's explicit
negatives and once on device-drawn ones.  --against compares the uint32 views element by element (NaN payloads count) and fails on any difference.
The library is chosen by SERT_LIB, read at import, and SERT_LL_NODEDUP once per process: every (library, group) runs in a fresh
child process started with subprocess, one at a time.  The run fails if the forms taken do not cover FAMILIES."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 37                       # a ragged last workgroup in both lane layouts (16 and 4 rows per workgroup)
# loglinear: name -> (n, V_e); csrc/host/step_softmax_loglinear.inc, ll_forward
LL = {'wave1': (7, 256), 'wave2': (7, 400), 'wave4': (7, 800), 'wave8': (7, 1028), 'table128': (7, 601),
      'table512': (7, 2050), 'fusedrow': (65, 300), 'stream_v4': (3, 13000), 'stream_scalar': (3, 13001)}
LL_PER_TOKEN = ('fusedrow', 'stream_v4', 'stream_scalar')            # the group under SERT_LL_NODEDUP: no slot table
# vectorspace: name -> (z, d_e); csrc/host/step_vectorspace.inc, vs_loss
VS = {'percand20': (12, 20), 'percand64': (12, 64), 'regs6': (5, 8), 'regs11': (10, 64), 'regs12': (11, 20), 'scalar': (3, 130)}
FS = {'fs16': 200, 'fs32': 1500, 'fs0': 2100}                        # V_e -> fs_softmax_ce<.., EPL>: 16 to 1024, 32 to 2048
FOLDIN = {'vector20': 20, 'vector64': 64, 'scalar130': 130}          # d_e; each with and without refreshed rows (the slot map)
FAMILIES = (['ll %s %s %s' % (f, lab, m) for lab in ('int', 'csr') for f, m in
             [('wave%d' % e, 'slots') for e in (1, 2, 4, 8)] + [('table128', 'slots'), ('table512', 'slots'),
              ('fused_row512 train', 'slots'), ('fused_row512 train', 'tokens'), ('fused_row512 eval', 'slots'),
              ('fused_row512 eval', 'tokens'), ('stream1', 'slots'), ('stream0', 'slots'), ('stream1', 'tokens'),
              ('stream0', 'tokens')]] +
            ['nce per_candidate train', 'nce per_candidate eval', 'nce scalar train', 'nce scalar eval'] +
            ['nce regs%d %s' % (c, t) for c in (6, 11, 12) for t in ('train', 'eval')] + ['fs epl%d' % e for e in (16, 32, 0)] +
            ['foldin %s %s %s' % (f, m, t) for f in ('vector', 'scalar') for m in ('two_part', 'map') for t in ('train', 'eval')] +
            # the sorted entity-gradient chain: every <VEC, NCH> of the chunked reduce under either fix-up, as the cases state them
            ['egrad %s %s' % (i, f) for i, f in [('1,4', 'wave'), ('1,4', 'workgroup'), ('4,1', 'wave'), ('4,1', 'workgroup'),
                                                 ('4,2', 'wave'), ('4,2', 'workgroup'), ('4,5', 'wave'), ('4,8', 'wave'),
                                                 ('4,8', 'workgroup')]] +
            ['foldin reduce %s %s' % (i, f) for i, f in [('1,4', 'wave'), ('1,4', 'workgroup'), ('4,1', 'wave'), ('4,1', 'workgroup'),
                                                         ('4,2', 'workgroup'), ('4,5', 'wave'), ('4,5', 'workgroup'), ('4,8', 'wave'),
                                                         ('4,8', 'workgroup')]] +
            # the loglinear fold-in: the label form, the creator, the window bucket of llf_row / llf_row_csr
            ['llf %s plain n<=%d' % (lab, b) for lab in ('int', 'csr') for b in (8, 16, 32)] +
            ['llf int refresh n<=8', 'llf csr refresh n<=8'] +
            # the word fold-in, from WordFoldIn.plan(): wfold <project> <loss> <segsum> <train|eval>
            ['wfold vector per_candidate rows32 train', 'wfold vector per_candidate none train', 'wfold vector per_candidate none eval',
             'wfold scalar scalar scalar train', 'wfold scalar scalar none eval'] +
            # the loglinear word fold-in, from LlWordFoldIn.plan(): llw <form> <vec|scalar> <labels> <segsum> <gemm_g> <split|whole>
            # <train|eval> -- split: G = dZ W^T cut into k ranges by gemm_long_k (ve4100: its K >= 4096 rule)
            ['llw %s %s %s' % (fv, lab, rest) for lab in ('int', 'rows') for fv, rest in
             [('reg scalar', 'none f32_tile128 whole train'), ('reg scalar', 'scalar f32_tile128 whole train'),
              ('reg scalar', 'none none whole eval'), ('reg vec', 'rows64 f32_tile128 whole train'),
              ('reg vec', 'rows64 f32_tile128 split train'), ('reg vec', 'none none whole eval'),
              ('stream scalar', 'scalar f32_tile128 split train'), ('stream scalar', 'none none whole eval'),
              ('stream vec', 'rows64 f32_tile128 split train'), ('stream vec', 'none none whole eval')]])


def run_engine(out, tag, eng, kind, uploads, form):
    from sert_amd import _capi as C
    from tests import util as U
    for split, kw in uploads:
        eng.upload_dataset(split, **kw)
    forms = []
    for step, call in enumerate([lambda: eng.train_batch(0), lambda: eng.train_batch(1),
                                 lambda: eng.eval_batch(C.SPLIT_TRAIN, 0), lambda: eng.eval_batch(C.SPLIT_VALIDATE, 0)]):
        out['%s/loss%d' % (tag, step)] = np.float32(call())
        out['%s/rowloss%d' % (tag, step)] = eng.get_tensor(C.T_ACT_ROWLOSS)
        forms.append(form(eng))
    for k, v in U.engine_state(eng).items():
        out['%s/%s' % (tag, k)] = v
    for name, which in (('g.R_w', C.T_GRAD_RW), ('g.R_e', C.T_GRAD_RE), ('g.W', C.T_GRAD_W), ('g.b', C.T_GRAD_B),
                        ('act.T', C.T_ACT_T), ('act.DA', C.T_ACT_DA)):
        if kind != C.KIND_LOGLINEAR or name in ('g.R_w', 'g.W', 'g.b'):
            out['%s/%s' % (tag, name)] = eng.get_tensor(which)
    eng.close()
    return forms


def ll_form(eng):
    f = eng.ll_loss_form()
    name = f['form'] + str(f['param'])
    if f['form'] == 'fused_row':
        name += ' train' if f['train'] else ' eval'
    return name, 'slots' if f['slots'] else 'tokens'


def run_ll(out, tag, p, b, n, labels):
    from sert_amd import _capi as C
    from tests import util as U
    eng = U.ll_engine(p, b, n, 0.0 if 'plant' in tag else 0.01)
    lab = (lambda sl: dict(y_int=p['y'][sl])) if labels == 'int' else (lambda sl: dict(csr=p['y'][sl]))
    tr, va = slice(0, 2 * b), slice(2 * b, 3 * b)
    forms = run_engine(out, tag, eng, C.KIND_LOGLINEAR, [(C.SPLIT_TRAIN, dict(x=p['X'][tr], w=p['w'][tr], **lab(tr))),
                                                        (C.SPLIT_VALIDATE, dict(x=p['X'][va], w=p['w'][va], **lab(va)))], ll_form)
    return ['ll %s %s %s' % (name, labels, mode) for name, mode in forms]


def run_vs(out, tag, p, z, kind=None):
    from sert_amd import _capi as C
    from tests import util as U
    n = p['X'].shape[1]
    if kind is None:
        eng = U.vs_engine(p, B, n, z, 0.01)
    else:
        eng = C.Engine(kind=kind, batch_size=B, global_batch_size=B, window_size=n, vocab_size=p['Rw'].shape[0],
                       num_entities=p['Re'].shape[0], word_dim=p['Rw'].shape[1], entity_dim=p['Re'].shape[1], num_negatives=0,
                       id_bytes=p['X'].dtype.itemsize, device=0, keep_grads=1, deterministic=1, lambda_=0.01, lr=1e-3,
                       beta1=0.9, beta2=0.999, eps=1e-8, seed=1)
        for which, key in ((C.T_RW, 'Rw'), (C.T_RE, 'Re'), (C.T_W, 'W'), (C.T_B, 'b')):
            eng.set_tensor(which, p[key])
    tr, va = slice(0, 2 * B), slice(2 * B, 3 * B)

    def form(e):
        if kind is not None:
            V = p['Re'].shape[0]
            return 'fs epl%d' % (16 if V <= 1024 else 32 if V <= 2048 else 0)     # (no hook: the rule of fs_forward)
        f = e.nce_form()
        return 'nce %s%s %s' % (f['form'], f['maxc'] if f['form'] == 'regs' else '', 'train' if f['train'] else 'eval')
    return run_engine(out, tag, eng, C.KIND_VECTORSPACE, [(C.SPLIT_TRAIN, dict(x=p['X'][tr], y_int=p['y'][tr], w=p['w'][tr])),
                                                         (C.SPLIT_VALIDATE, dict(x=p['X'][va], y_int=p['y'][va], w=p['w'][va]))], form)


def run_foldin(out, tag, p, z, refresh):
    from sert_amd import _capi as C
    from tests import util as U
    n, (Ve, de) = p['X'].shape[1], p['Re'].shape
    eng = U.vs_engine(p, 8, n, 2, 0.01, keep_grads=0)
    rng = np.random.RandomState(7)
    new = 5
    f = C.FoldIn(eng, (0.1 * rng.randn(new, de)).astype(np.float32), B, z, 0.01, seed=3,
                 refresh_ids=np.array([3, Ve - 1, 10], dtype=np.int32) if refresh else None)
    f.upload(p['X'][:2 * B].astype(np.int32), rng.randint(0, f.num_rows, 2 * B).astype(np.int32), p['w'][:2 * B])
    forms = []
    for step, call in enumerate([lambda: f.train_batch(0), lambda: f.train_batch(1), lambda: f.eval_batch(0)]):
        out['%s/loss%d' % (tag, step)] = np.float32(call())
        pl = f.plan()
        forms.append('foldin %s %s %s' % (pl['loss'], 'map' if f.table()['map'] else 'two_part', 'train' if pl['train'] else 'eval'))
    for name, which in (('E', C.FOLDIN_ROWS), ('m', C.FOLDIN_M), ('v', C.FOLDIN_V)):
        out['%s/%s' % (tag, name)] = f.get_rows(which)
    f.close()
    eng.close()
    return forms


def run_egrad_case(out, name, sort):
    """Two steps of a case of tests/egrad_key_cases.py with keep_grads = 1; sort: SERT_EGRAD_SORT=1 (read at sert_create)."""
    from sert_amd import _capi as C
    from tests import egrad_key_cases as K
    from tests import util as U
    c, p = K.case_problem(name)
    os.environ.pop('SERT_EGRAD_SORT', None)
    if sort:
        os.environ['SERT_EGRAD_SORT'] = '1'
    tag = 'egrad_%s_%s' % (name, 'sorted' if sort else 'bucket')
    eng = U.vs_engine(p, c['B'], K.N, c['z'], K.LAM, keep_grads=1)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    forms = []
    for s in range(K.STEPS):
        out['%s/loss%d' % (tag, s)] = np.float32(eng.train_batch(s, p['neg'][s] if p['neg'][s].shape[1] else None))
        out['%s/g.R_e%d' % (tag, s)] = eng.get_tensor(C.T_GRAD_RE)
        pl = eng.egrad_plan()
        assert pl['path'] == ('sorted' if sort else 'bucket'), (name, pl)
        if sort:
            forms.append('egrad %d,%d %s' % (pl['vec'], pl['nch'], pl['fixup']))
    out[tag + '/R_e'] = eng.get_tensor(C.T_RE)
    eng.close()
    return forms


def run_foldin_case(out, tag, c, init_rows, seed, refresh_ids):
    """Two steps of a case of tests/foldin_key_cases.py or tests/refresh_cases.py on the case's explicit negatives."""
    from sert_amd import _capi as C
    eng = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=8, global_batch_size=8, window_size=c['n'], vocab_size=c['Vw'],
                   num_entities=c['Ve'], word_dim=c['dw'], entity_dim=c['de'], num_negatives=2, id_bytes=4, device=0, keep_grads=0,
                   deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=99)
    for which, key in ((C.T_RW, 'Rw'), (C.T_RE, 'Re'), (C.T_W, 'W'), (C.T_B, 'b')):
        eng.set_tensor(which, c[key])
    f = C.FoldIn(eng, init_rows, c['B'], c['z'], c['lam'], lr=c['lr'], seed=seed, refresh_ids=refresh_ids)
    f.upload(c['X'], c['y'], c['w_upload'])
    forms = []
    for s, b in enumerate(c['batches']):
        out['%s/loss%d' % (tag, s)] = np.float32(f.train_batch(b, c['neg'][s]))
        pl = f.plan()
        forms.append('foldin reduce %d,%d %s' % (pl['vec'], pl['nch'], pl['fixup']))
        for name, which in (('E', C.FOLDIN_ROWS), ('m', C.FOLDIN_M), ('v', C.FOLDIN_V)):
            out['%s/%s%d' % (tag, name, s)] = f.get_rows(which)
    f.close()
    eng.close()
    return forms


def chain_child(out):
    from tests import egrad_key_cases as EK
    from tests import foldin_cases as FC
    from tests import foldin_key_cases as FK
    from tests import refresh_cases as RC
    forms = []
    for name in EK.CASES:
        forms += run_egrad_case(out, name, True)
        if EK.is_bucket(name):
            forms += run_egrad_case(out, name, False)
    os.environ.pop('SERT_EGRAD_SORT', None)
    for name in FK.CASES:
        c = FK.case_problem(name)
        forms += run_foldin_case(out, 'foldin_keys_' + name, c, c['E0'], FC.SEED, None)
    for name in RC.CASES:
        c = RC.make_case(name)
        forms += run_foldin_case(out, 'refresh_' + name, c, c['New0'], RC.SEED, c['refresh'])
    return forms


def run_fold_steps(out, tag, f, state, form, negs=(None, None), eval_neg=None):
    """Two train_batch steps, train_batches over two batches, one eval_batch; after each: the losses and state(f)."""
    with_neg = lambda call, batch, neg: [call(batch)] if neg is None else [call(batch, neg)]      # (LlFoldIn takes none)
    steps = [('s0', lambda: with_neg(f.train_batch, 0, negs[0])), ('s1', lambda: with_neg(f.train_batch, 1, negs[1])),
             ('s23', lambda: f.train_batches([2, 0])), ('ev', lambda: with_neg(f.eval_batch, 1, eval_neg))]
    forms = []
    for name, call in steps:
        out['%s/loss_%s' % (tag, name)] = np.asarray(call(), dtype=np.float32)
        forms.append(form(name != 'ev'))
        for k, v in state(f).items():
            out['%s/%s_%s' % (tag, k, name)] = v
    f.close()
    return forms


def foldins_child(out):
    from sert_amd import _capi as C
    from tests import ll_foldin_cases as LC
    from tests import ll_foldin_label_cases as LL
    from tests import ll_refresh_cases as RC
    from tests import ll_wfold_cases as LWC
    from tests import ll_wfold_rows_cases as LWR
    from tests import util as U
    from tests import wfold_cases as WC
    forms = []
    ll_tensors = (('W', C.LL_FOLDIN_W), ('b', C.LL_FOLDIN_B), ('accu.W', C.LL_FOLDIN_ACCU_W), ('accu.b', C.LL_FOLDIN_ACCU_B),
                  ('delta.W', C.LL_FOLDIN_DELTA_W), ('delta.b', C.LL_FOLDIN_DELTA_B))
    for mod, prefix in ((LC, 'llf'), (LL, 'llf_labels'), (RC, 'llf_refresh')):
        for name in sorted(mod.CASES):
            c = mod.make_case(name)
            eng = U.ll_engine(dict(Rw=c['Rw'], W=c['W'], b=c['b'], X=c['X']), 8, c['n'], 0.01, keep_grads=0)
            refresh = c.get('refresh')
            f = C.LlFoldIn(eng, c['Wn0'] if c['N'] else None, c['bn0'] if c['N'] else None, c['B'], c['lam'], refresh_ids=refresh)
            eng.close()
            csr = 'indptr' in c
            if csr:
                f.upload_csr(c['X'], c['indptr'], c['indices'], c['data'], c['w'])
            else:
                f.upload(c['X'], c['y'], c['w'])
            # (no hook: the rule of llf_forward)
            family = 'llf %s %s n<=%d' % ('csr' if csr else 'int', 'plain' if refresh is None else 'refresh',
                                          8 if c['n'] <= 8 else 16 if c['n'] <= 16 else 32)
            forms += run_fold_steps(out, '%s_%s' % (prefix, name), f, lambda h: dict((k, h.get_tensor(w)) for k, w in ll_tensors),
                                    lambda train: family)
    for name in sorted(WC.CASES):
        c = WC.make_case(name)
        for drawn in (False, True):
            eng = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=8, global_batch_size=8, window_size=c['n'], vocab_size=c['Vw'],
                           num_entities=c['Ve'], word_dim=c['dw'], entity_dim=c['de'], num_negatives=2, id_bytes=4, device=0,
                           keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=99)
            for which, key in ((C.T_RW, 'Rw'), (C.T_RE, 'Re'), (C.T_W, 'W'), (C.T_B, 'b')):
                eng.set_tensor(which, c[key])
            f = C.WordFoldIn(eng, c['Nv0'], c['B'], c['z'], c['lam'], lr=c['lr'], seed=WC.SEED)
            eng.close()
            f.upload(c['X'], c['y'], c['w'])
            tag = 'wfold_%s_%s' % (name, 'drawn' if drawn else 'explicit')
            out[tag + '/neg_train0'], out[tag + '/neg_eval0'] = f.negatives_of_step(0), f.negatives_of_step(0, True)

            def form(train, f=f):
                pl = f.plan()
                assert pl['train'] == train, pl
                return 'wfold %s %s %s %s' % (pl['project'], pl['loss'], pl['segsum'], 'train' if train else 'eval')
            forms += run_fold_steps(out, tag, f, lambda h: dict((k, h.get_rows(w)) for k, w in
                                                                 (('Nv', C.WFOLD_ROWS), ('m', C.WFOLD_M), ('v', C.WFOLD_V))),
                                    form, negs=(None, None) if drawn else (c['neg'][0], c['neg'][1]),
                                    eval_neg=None if drawn else c['eval_neg'])
    # the loglinear word fold-in on integer labels and on label rows; from LlWordFoldIn.plan():
    # llw <form> <vec|scalar> <labels> <segsum> <gemm_g> <split|whole> <train|eval>
    llw_rows = (('Nv', C.LL_WFOLD_ROWS), ('accu', C.LL_WFOLD_ACCU), ('delta', C.LL_WFOLD_DELTA))
    for mod, prefix in ((LWC, 'llw'), (LWR, 'llw_rows')):
        for name in sorted(mod.CASES):
            c = mod.make_case(name)
            eng = U.ll_engine(dict(Rw=c['Rw'], W=c['W'], b=c['b'], X=c['X']), 8, c['n'], 0.01, keep_grads=0)
            f = C.LlWordFoldIn(eng, c['Nv0'], c['B'], c['lam'])
            eng.close()
            if 'indptr' in c:
                f.upload_csr(c['X'], c['indptr'], c['indices'], c['data'], c['w'])
            else:
                f.upload(c['X'], c['y'], c['w'])

            def form(train, f=f):
                pl = f.plan()
                assert pl['train'] == train, pl
                return 'llw %s %s %s %s %s %s %s' % (pl['form'], 'vec' if pl['vec'] else 'scalar', pl['labels'], pl['segsum'], pl['gemm_g'],
                                                     'split' if pl['splits'] > 1 else 'whole', 'train' if train else 'eval')
            forms += run_fold_steps(out, '%s_%s' % (prefix, name), f, lambda h: dict((k, h.get_rows(w)) for k, w in llw_rows), form)
    return forms


def child(group, path):
    from sert_amd import _capi as C
    from tests import ll_nonfinite_cases as NF
    from tests import util as U
    out, forms = {}, []
    if group in ('chain', 'foldins'):
        out['forms'] = np.array(sorted(set((chain_child if group == 'chain' else foldins_child)(out))))
        np.savez_compressed(path, **out)
        return
    for k, name in enumerate(sorted(LL if group == 'slots' else LL_PER_TOKEN)):
        n, Ve = LL[name]
        for labels in ('int', 'csr'):
            p = U.make_ll_problem(500 + k, 3 * B, n, 150, Ve, 16, labels=labels)
            forms += run_ll(out, 'll_%s_%s_%s' % (group, name, labels), p, B, n, labels)
    if group == 'slots':
        # one input that clips (a bias of -inf: the probability clips to 1e-7) and one planted NaN, loglinear ...
        for plant in (NF.CONTROL, 'nan_word_mid'):
            c, p = NF.case_problem('wave2')
            Rw, W, b, _ = NF.planted('wave2', plant)
            forms += run_ll(out, 'll_plant_%s' % plant, dict(p, Rw=Rw, W=W, b=b), NF.B, c['n'], 'int')
        for k, name in enumerate(sorted(VS)):
            z, de = VS[name]
            forms += run_vs(out, 'vs_' + name, U.make_vs_problem(600 + k, 3 * B, 5, z, 150, 90, 12, de), z)
        # ... and NCE: saturated sigmoids and tanh units (entity rows and W scaled up), a NaN in a word row of batch 0
        for plant in ('clip', 'nan'):
            p = U.make_vs_problem(650, 3 * B, 5, 12, 150, 90, 12, 20)
            if plant == 'clip':
                p['Re'], p['W'] = p['Re'] * np.float32(40), p['W'] * np.float32(30)
            else:
                p['Rw'][int(p['X'][3, 2]), 4] = np.nan
            forms += run_vs(out, 'vs_plant_' + plant, p, 12)
        for k, name in enumerate(sorted(FS)):
            forms += run_vs(out, 'fs_' + name, U.make_vs_problem(700 + k, 3 * B, 5, 0, 150, FS[name], 12, 20), 0,
                            kind=C.KIND_VECTORSPACE_SOFTMAX)
        for k, name in enumerate(sorted(FOLDIN)):
            for refresh in (False, True):
                p = U.make_vs_problem(800 + k, 2 * B, 5, 6, 150, 90, 12, FOLDIN[name])
                forms += run_foldin(out, 'foldin_%s_%d' % (name, refresh), p, 6, refresh)
    out['forms'] = np.array(sorted(set(forms)))
    np.savez_compressed(path, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True)
    ap.add_argument('--lib', help='library to run (SERT_LIB); default: the tree\'s own')
    ap.add_argument('--against', help='an .npz of an earlier run: every array must hold the same bits')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.out)
    merged = {}
    for group in ('slots', 'tokens', 'chain', 'foldins'):
        env = dict(os.environ)
        env.pop('SERT_LL_NODEDUP', None)
        if a.lib:
            env['SERT_LIB'] = os.path.abspath(a.lib)
        if group == 'tokens':
            env['SERT_LL_NODEDUP'] = '1'
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, group + '.npz')
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child', group, '--out', part], env=env, cwd=ROOT, check=True)
            with np.load(part) as z:
                forms = set(merged.get('forms', ())) | set(z['forms'].tolist())
                merged.update({k: z[k] for k in z.files})
                merged['forms'] = np.array(sorted(forms))
    np.savez_compressed(a.out, **merged)
    missing = [f for f in FAMILIES if f not in set(merged['forms'].tolist())]
    print('%d arrays, %d forms' % (len(merged) - 1, len(merged['forms'])))
    if missing:
        print('forms taken:\n  ' + '\n  '.join(merged['forms'].tolist()))
        sys.exit('families not reached: %s' % missing)
    if a.against:
        with np.load(a.against) as z:
            other = {k: z[k] for k in z.files}
        keys = sorted(set(merged) | set(other))
        diff = [k for k in keys if k not in merged or k not in other or merged[k].shape != other[k].shape or
                not np.array_equal(np.ascontiguousarray(merged[k]).view(np.uint8), np.ascontiguousarray(other[k]).view(np.uint8))]
        for k in diff:
            if k in merged and k in other and merged[k].shape == other[k].shape and merged[k].dtype == np.float32:
                x, y = merged[k].ravel().view(np.uint32), other[k].ravel().view(np.uint32)
                print('DIFFERENT %s: %d of %d elements' % (k, int((x != y).sum()), x.size))
            else:
                print('DIFFERENT %s (missing, or another shape)' % k)
        nans = sum(int(np.isnan(v).any()) for k, v in merged.items() if v.dtype == np.float32)
        print('%d arrays compared, %d differ; %d arrays hold a NaN' % (len(keys), len(diff), nans))
        if diff:
            sys.exit(1)


if __name__ == '__main__':
    main()
