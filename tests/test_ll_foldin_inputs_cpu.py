"""CPU: the inputs of the loglinear fold-in tests (tests/ll_foldin_cases.py) have the structure each case is named for,
proved with NumPy and the oracle twin; clip_live meets its clip conditions and tells the factored shortcut from the contract;
the binding lists what include/sert_hip_ll_foldin.h declares."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi
from tests import ll_foldin_cases as LC
from tests.util import ROOT


@pytest.fixture(scope='module', params=sorted(LC.CASES))
def case(request):
    return LC.make_case(request.param)


def test_case_shapes_and_ranges(case):
    c = case
    B, n, N, M = c['B'], c['n'], c['N'], c['M']
    assert M == 3 * B + LC.TRAILING and c['batches'] == M // B >= LC.STEPS
    assert c['X'].shape == (M, n) and c['X'].dtype == np.int32 and c['X'].min() >= 0 and c['X'].max() < c['Vw']
    assert c['y'].shape == (M,) and c['y'].dtype == np.int32 and c['y'].min() >= 0 and c['y'].max() < N
    assert c['w'].shape == (M,) and c['w'].min() >= 0.5 and c['w'].max() <= 2.0
    assert c['Rw'].shape == (c['Vw'], c['d']) and c['W'].shape == (c['d'], c['Ve']) and c['b'].shape == (c['Ve'],)
    assert c['Wn0'].shape == (c['d'], N) and c['bn0'].shape == (N,)
    assert 1 <= n <= 32
    assert LC.make_case(c['name']) is c                     # (generated once: the tests share it and leave it unchanged)


def test_named_structure():
    """Each case's mechanism, from its arrays."""
    C = {k: LC.make_case(k) for k in LC.CASES}
    c = C['base']
    assert (c['N'] - 1) not in c['y'][:c['B']] and (c['N'] - 1) in c['y']
    assert C['wide_ve']['Ve'] == 700 and C['wide_ve']['Ve'] % 256          # (several entities per lane, a ragged last trip)
    assert C['one_new']['N'] == 1 and not C['one_new']['y'].any()
    assert C['many_new']['N'] > 256
    assert (C['n1']['n'], C['n9']['n'], C['n32']['n']) == (1, 9, 32)          # NMAX 8, 16, 32; base has n = 3 (NMAX 8)
    assert C['odd_d']['d'] % 4 and C['d300']['d'] == 300
    c = C['repeated_word']
    B = c['B']
    assert len(set(c['X'][0].tolist())) == 1 and c['n'] > 1
    assert np.bincount(c['X'][:B].ravel(), minlength=c['Vw']).max() > 64
    assert C['batch_of_one']['B'] == 1 and C['batch_of_one']['batches'] == 3 + LC.TRAILING
    assert C['lam0']['lam'] == 0.0 and all(C[k]['lam'] == 0.01 for k in C if k != 'lam0')
    # every batch of every case repeats words (the per-word sums add more than one row) and misses words of the upload
    for c in C.values():
        if c['B'] * c['n'] > 1 and c['name'] != 'batch_of_one':
            counts = np.bincount(c['X'][:c['B']].ravel(), minlength=c['Vw'])
            assert counts.max() > 1, c['name']


def test_twin_is_the_contract():
    """One twin step on `base`: the gradient is the extended oracle's, columns V_e onward; the loss is the data term plus
    lambda / (2B) sum(Wn Wn) over the trainable columns only; Adadelta moves Wn and bn from zero accumulators; the frozen
    tensors stay; evaluation changes nothing."""
    c = LC.make_case('base')
    B, Ve = c['B'], c['Ve']
    before = [c[k].copy() for k in ('Rw', 'W', 'b', 'Wn0', 'bn0')]
    X, y, w = c['X'][:B], Ve + c['y'][:B].astype(np.int64), c['w'][:B]
    Wx, bx = np.concatenate([c['W'], c['Wn0']], axis=1), np.concatenate([c['b'], c['bn0']])
    data, grads, _ = O.LogLinearOracle(B, c['n'], c['Rw'], Wx, bx, 0.0).loss_and_grads(X, y, w)
    tw = LC.LlFoldInTwin(c)
    loss, gW, gb = tw.train_step(0, return_grads=True)
    reg = c['lam'] / (2.0 * B) * float((c['Wn0'].astype(np.float64) ** 2).sum())
    assert abs(float(loss) - (float(data) + reg)) <= 1e-6 * abs(float(loss))
    assert np.allclose(gW, grads[1][:, Ve:] + np.float32(c['lam'] / B) * c['Wn0'], rtol=1e-5, atol=1e-9)
    assert np.array_equal(gb, grads[2][Ve:])                              # the bias is not regularised
    st = tw.state()
    assert np.allclose(st['accu.W'], 0.05 * gW * gW, rtol=1e-5, atol=0) and np.allclose(st['accu.b'][0], 0.05 * gb * gb, rtol=1e-5)
    assert not np.array_equal(tw.Wn, c['Wn0']) and not np.array_equal(tw.bn, c['bn0'])
    for k, b in zip(('Rw', 'W', 'b', 'Wn0', 'bn0'), before):
        assert np.array_equal(c[k], b), k
    W1 = tw.Wn.copy()
    assert np.isfinite(tw.eval_loss(1)) and np.array_equal(tw.Wn, W1)
    # float64: same trajectory to float32 rounding
    t64 = LC.LlFoldInTwin(c, np.float64)
    assert abs(float(t64.train_step(0)) - float(loss)) < 1e-5 * abs(float(loss))


def test_clip_live_conditions():
    """clip_live over its three steps on the float64 twin: frozen and new token probabilities below 1e-7, rows with Q_y below
    1e-7 and rows above it in every step, no P and no Q_y within relative 1e-3 of a clip bound, finite gradients, a non-zero
    Wn gradient."""
    c = LC.make_case('clip_live')
    rep = LC.clip_report(c)
    print('clip_live (seed attempt %d): %d of %d frozen and %d of %d new token probabilities clipped, labels clipped per step %r '
          'of %d, margin %.2e' % (c['attempt'], rep['frozen_clipped'], rep['frozen_total'], rep['new_clipped'], rep['new_total'],
                                  rep['labels_clipped'], c['B'], rep['margin']))
    assert rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0
    assert len(rep['labels_clipped']) == LC.STEPS and all(0 < k < c['B'] for k in rep['labels_clipped'])
    assert rep['margin'] > LC.CLIP_MARGIN
    assert rep['finite'] and rep['grad_nonzero']
    assert LC.clip_ok(rep, c['B'])
    # the other cases are NOT clip cases: nothing of theirs is clipped at step 0
    b = LC.make_case('base')
    f = LC.LlFoldInTwin(b, np.float64).forward(0)
    assert f['P3'].min() > 1e-7 and f['P3'].max() < 1 - 1e-7


def _factored_loss(c, batch):
    """The shortcut the contract forbids, in float64: the frozen entities' share of the joint's normaliser taken as a
    per-instance constant times exp(-sum_t lse_t), i.e. their log-probabilities NOT clipped; the new columns and the label
    handled as the contract says.  -> the unweighted mean loss of the batch."""
    B, Ve = c['B'], c['Ve']
    sl = slice(batch * B, (batch + 1) * B)
    X, y = c['X'][sl], c['y'][sl]
    lo, hi = O.clip_bounds(np.float64)
    Z = c['Rw'].astype(np.float64)[X] @ np.concatenate([c['W'], c['Wn0']], axis=1).astype(np.float64) + \
        np.concatenate([c['b'], c['bn0']]).astype(np.float64)                      # (B, n, V_e + N)
    m = Z.max(axis=2, keepdims=True)
    lse = m + np.log(np.exp(Z - m).sum(axis=2, keepdims=True))
    logp = Z - lse
    J = np.concatenate([logp[:, :, :Ve].sum(axis=1),                                # constant_i - sum_t lse_t, per frozen entity
                        np.clip(logp[:, :, Ve:], np.log(lo), np.log(hi)).sum(axis=1)], axis=1)
    Q = O.softmax_rows(J)
    return float(np.mean(-np.log(np.clip(Q[np.arange(B), Ve + y], lo, hi))))


def test_clip_live_discriminates_the_factored_shortcut():
    """On clip_live the factored shortcut's loss differs from the twin's by more than the GPU test's 1e-5 loss tolerance; on
    base, where nothing is clipped, the two agree -- the shortcut is the contract exactly while no frozen P is below 1e-7."""
    c = LC.make_case('clip_live')
    tw = LC.LlFoldInTwin(c, np.float64)
    diffs = []
    for batch in range(3):
        ref, short = float(tw.eval_loss(batch)), _factored_loss(c, batch)
        diffs.append(abs(short - ref) / abs(ref))
    print('clip_live: relative loss difference of the factored shortcut per batch: %r' % (diffs,))
    # (the GPU test checks the loss of every step, each on its own batch: one batch beyond the tolerance fails a device path
    #  that takes the shortcut; how far a batch moves depends on how many of its window words carry clipped frozen entries)
    assert max(diffs) > 1e-5
    b =LC.make_case('base')
    ref, short = float(LC.LlFoldInTwin(b, np.float64).eval_loss(0)), _factored_loss(b, 0)
    assert abs(short - ref) <= 1e-9 * abs(ref)


def test_binding_lists_the_ll_foldin_symbols(hip_lib):
    """include/sert_hip_ll_foldin.h, which sert_hip.h includes, declares exactly _capi.EXPORTS_LL_FOLDIN; the library exports
    them; the config struct of the binding has the header's size and fields; the build's dependencies name the header."""
    src = open(os.path.join(ROOT, 'include', 'sert_hip_ll_foldin.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(sert_ll_foldin_[a-z_0-9]+)\s*\(', src)))
    assert declared == sorted(_capi.EXPORTS_LL_FOLDIN)
    assert '#include "sert_hip_ll_foldin.h"' in open(os.path.join(ROOT, 'include', 'sert_hip.h')).read()
    assert "'sert_hip_ll_foldin.h'" in open(os.path.join(ROOT, 'sert_amd', '_build.py')).read()
    assert not [s for s in _capi.EXPORTS_LL_FOLDIN if not hasattr(hip_lib, s)]
    assert not set(_capi.EXPORTS_LL_FOLDIN) & set(_capi.EXPORTS + _capi.EXPORTS_FOLDIN)
    assert [f[0] for f in _capi.SertLlFoldInConfig._fields_] == ['struct_size', 'batch_size', 'lambda_', 'lr', 'rho', 'eps',
                                                                 'max_cache_bytes']
    assert ctypes.sizeof(_capi.SertLlFoldInConfig) == 32
    # no device: a null model is refused with a message, and so are null handles
    cfg = _capi.SertLlFoldInConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    h = ctypes.c_void_p()
    assert hip_lib.sert_ll_foldin_create(None, 1, None, None, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'null argument' in hip_lib.sert_last_error()
    assert hip_lib.sert_ll_foldin_num_batches(None) == -1
    assert hip_lib.sert_ll_foldin_train_batch(None, 0, None) != 0
    assert hip_lib.sert_ll_foldin_destroy(None) == 0
