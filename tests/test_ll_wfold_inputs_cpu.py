"""CPU: the inputs of the loglinear word fold-in tests have the structure they exist for (tests/ll_wfold_cases.py), the index
the handle builds (csrc/wfold_index.h, through the host-only sert_debug_wfold_index) is what the contract states, the identity
the device path rests on holds in float64, and the same reassociated form in float32 NumPy stays inside the row bounds.  No
device.

The reassociated form (S_v = sum of dJ over v's occurrences, Rsum_v = <mask_v, S_v>, dZ_v = mask_v S_v - P_v Rsum_v,
G = dZ W^T + lambda / B Nv) in float32 against the float64 twin after the 3 steps, worst row-wise error of Nv / accu / delta per
case (bound: tests.util.ROW_TOL64 = 5e-5 for all three):
    case              Nv       accu     delta
    all_new           5.5e-08  2.6e-07  4.6e-07
    base              4.2e-08  3.7e-07  2.8e-07
    batch_of_one      5.9e-08  2.1e-07  2.0e-07
    chunk65           6.8e-08  5.4e-07  5.4e-07
    clip_live         6.0e-08  5.0e-07  3.9e-07
    d300              4.6e-08  3.9e-07  2.6e-07
    lam0              8.0e-08  3.5e-07  2.5e-07
    many_words        9.3e-08  6.5e-07  3.7e-07
    n1                4.7e-08  3.9e-07  2.1e-07
    n32               2.4e-07  4.9e-07  9.0e-06
    odd_d             8.2e-08  4.5e-07  2.3e-07
    one_word          3.5e-08  2.4e-07  1.4e-07
    three_levels      1.6e-07  6.1e-06  4.0e-06
    ve1024            6.8e-08  3.8e-07  2.4e-07
    ve1025            4.9e-08  3.9e-07  2.5e-07
    ve4100            5.0e-08  6.3e-07  5.3e-07
    ve700             6.1e-08  3.9e-07  2.7e-07
    ve8               5.5e-08  3.2e-07  2.1e-07
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi
from tests import ll_wfold_cases as LW
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LlWordFoldIn = _capi.LlWordFoldIn       # the binding everything here is about: without it there is nothing to prove inputs for


@pytest.fixture(scope='module')
def cases():
    return {name: LW.make_case(name) for name in LW.CASES}


@pytest.mark.parametrize('name', sorted(LW.CASES))
def test_case_has_its_structure(cases, name):
    c = cases[name]
    Vw, Nw, Ve, d, n, B = (c[k] for k in ('Vw', 'Nw', 'Ve', 'd', 'n', 'B'))
    X, tok = c['X'], LW.new_tokens(c)
    assert X.shape == (c['M'], n) and X.min() >= 0 and X.max() < Vw + Nw
    assert c['y'].min() >= 0 and c['y'].max() < Ve and c['Nv0'].shape == (Nw, d)
    assert c['M'] == 3 * B + LW.TRAILING and c['M'] // B == c['batches'] >= LW.STEPS      # a tail that is never visited at B > 5
    assert np.abs(c['Nv0']).max() <= np.sqrt(6.0 / (Vw + d))          # the scale sert_amd.foldin.new_word_rows draws at
    per_batch = [tok[i * B:(i + 1) * B] for i in range(c['batches'])]
    counts = [np.bincount(t[t >= 0], minlength=Nw) for t in per_batch]
    plans = [LW.expected_plan(c, i) for i in range(c['batches'])]
    assert all(p['form'] == ('stream' if name in ('ve1025', 've4100') else 'reg') for p in plans)
    if name == 'base':
        assert counts[0][Nw - 1] == 0 and counts[0][:Nw - 1].min() > 0
        assert any((r < 0).all() for r in per_batch[0])
        assert any(np.bincount(r[r >= 0], minlength=Nw).max() >= 2 for r in per_batch[0])
    elif name == 've8':
        assert Ve % 4 == 0 and plans[0]['vec'] and plans[0]['segsum'] == 'rows64'
    elif name == 've700':
        assert Ve % 4 == 0 and Ve % 256 != 0 and Ve > 256
    elif name == 've1024':
        assert Ve == LW.REG_MAX_VE and plans[0]['vec']
    elif name == 've1025':
        assert Ve == LW.REG_MAX_VE + 1 and not plans[0]['vec'] and plans[0]['segsum'] == 'scalar'
    elif name == 've4100':
        # K = V_e >= 4096 with one output tile: the first rule of gemm_long_k, V_e // 1024 k ranges, the last one ragged
        assert 4096 <= Ve < 4096 + 16 and Ve // 1024 == 4 and Ve % 1024 != 0 and Nw <= 128 and d <= 128 and plans[0]['vec']
    elif name == 'n1':
        assert n == 1
    elif name == 'n32':
        assert n == 32
    elif name == 'all_new':
        assert X.min() >= Vw
    elif name == 'one_word':
        assert Nw == 1 and all(k[0] > 0 for k in counts)
    elif name == 'many_words':
        assert Nw > 256 and all((k == 0).sum() > Nw // 2 for k in counts)
    elif name == 'chunk65':
        assert counts[0][0] == LW.CHUNK and counts[1][0] == LW.CHUNK + 1
        assert plans[0]['levels'] == 1 and plans[1]['levels'] == 2 and plans[1]['items'][1] == 1
    elif name == 'three_levels':
        assert counts[0][0] == LW.CHUNK ** 2 + 1 and B * n >= counts[0][0] and plans[0]['levels'] == 3
        assert plans[0]['items'][1:] == [2, 1]
    elif name == 'odd_d':
        assert d % 4 != 0
    elif name == 'd300':
        assert d == 300
    elif name == 'batch_of_one':
        assert B == 1
    elif name == 'lam0':
        assert c['lam'] == 0.0
    if name not in ('chunk65', 'three_levels'):
        assert all(p['levels'] <= 1 for p in plans)


def reassociated_gradient(c, Nv, batch, dt):
    """The gradient of Nv on `batch` in the association of the device path, restated in NumPy: the distinct words' log
    distributions once, J as a sum of clipped rows, dJ from the label term, S / Rsum / dZ per new word, G = dZ W^T + L2.
    -> (G, data loss)."""
    dt = np.dtype(dt)
    T = dt.type
    lo, hi = O.clip_bounds(dt)
    Vw, Nw, B, lam = c['Vw'], c['Nw'], c['B'], c['lam']
    X = c['X'][batch * B:(batch + 1) * B].astype(np.int64)
    y = c['y'][batch * B:(batch + 1) * B].astype(np.int64)
    w = c['w'][batch * B:(batch + 1) * B].astype(dt)
    W, b = c['W'].astype(dt), c['b'].astype(dt)
    ext = np.concatenate([c['Rw'].astype(dt), np.asarray(Nv, dtype=dt)], axis=0)
    P = O.softmax_rows((ext @ W + b).astype(dt))                    # one row per word of the extended vocabulary
    inside = ((P >= lo) & (P <= hi)).astype(dt)
    Lc = np.log(np.clip(P, lo, hi))
    J = np.zeros((B, W.shape[1]), dtype=dt)
    for j in range(X.shape[1]):
        J += Lc[X[:, j]]
    Q = O.softmax_rows(J)
    Qy = Q[np.arange(B), y]
    Qc = np.clip(Qy, lo, hi)
    g = (w / T(B)).astype(dt)
    qdq = Qy * np.where((Qy >= lo) & (Qy <= hi), -g / Qc, T(0))
    dJ = -Q * qdq[:, None]
    dJ[np.arange(B), y] += qdq
    S = np.zeros((Nw, W.shape[1]), dtype=dt)
    for j in range(X.shape[1]):                                     # a word twice in a window counts dJ_i twice
        new = X[:, j] >= Vw
        np.add.at(S, X[new, j] - Vw, dJ[new])
    Pn, Mn = P[Vw:], inside[Vw:]
    Rsum = (Mn * S).sum(axis=1, dtype=dt)
    dZ = Mn * S - Pn * Rsum[:, None]
    G = (dZ @ W.T).astype(dt)
    if lam > 0.0:
        G = G + T(lam) / T(B) * np.asarray(Nv, dtype=dt)
    loss = T((-np.log(Qc) * w).sum(dtype=dt) / T(B))
    return G.astype(dt), loss


@pytest.mark.parametrize('name', sorted(LW.CASES))
def test_identity_in_float64(cases, name):
    """S, Rsum = <mask, S> and G = dZ W^T equal the twin's gradient (LogLinearOracle on ExtW) in float64 to 1e-12, over the
    three steps of the twin's own trajectory."""
    c = cases[name]
    tw = LW.LlWordFoldInTwin(c, np.float64)
    for s in range(LW.STEPS):
        G, loss = reassociated_gradient(c, tw.Nv, s, np.float64)
        data, g, _ = tw.loss_and_grads(s)
        scale = max(1e-300, float(np.abs(g).max()))
        assert float(np.abs(G - g).max()) <= 1e-12 * scale, (name, s, float(np.abs(G - g).max()), scale)
        assert abs(loss - data) <= 1e-12 * abs(data)
        tw.train_step(s)


def _float32_figures(c):
    t64 = LW.LlWordFoldInTwin(c, np.float64)
    Nv = np.array(c['Nv0'], dtype=np.float32, copy=True)
    opt = O.Adadelta([Nv], lr=1.0, rho=0.95, eps=1e-6)
    for s in range(LW.STEPS):
        G, _ = reassociated_gradient(c, Nv, s, np.float32)
        opt.update([Nv], [G])
        t64.train_step(s)
    ref = t64.state()
    return [U.row_err(a, ref[k])[0] for a, k in ((Nv, 'R_w'), (opt.accu[0], 'accu.R_w'), (opt.delta[0], 'delta.R_w'))]


@pytest.mark.parametrize('name', sorted(LW.CASES))
def test_reassociated_form_in_float32_stays_inside_the_row_bound(cases, name):
    figures = _float32_figures(cases[name])
    print('    %-17s %s' % (name, '  '.join('%.1e' % e for e in figures)))
    assert max(figures) < U.ROW_TOL64, (name, figures)


@pytest.mark.parametrize('name', sorted(LW.CASES))
def test_index_of_every_case(hip_lib, cases, name):
    """Per batch: the entries, their order, the chunking and the levels of the library's builder against the rule restated
    from the case's constants (ll_wfold_cases.index_of_batch)."""
    c = cases[name]
    B, n, Nw = c['B'], c['n'], c['Nw']
    tok = LW.new_tokens(c)[:c['batches'] * B].reshape(c['batches'], B, n)
    for batch in range(c['batches']):
        got = _capi.debug_wfold_index(tok, Nw, batch)
        rows, levels = LW.index_of_batch(c, batch)
        assert got['levels'] == len(levels) and got['item_counts'] == [len(l) for l in levels]
        assert np.array_equal(got['rows'], rows) and len(rows) == int((tok[batch] >= 0).sum())
        assert got['items'].tolist() == [list(it + (0,)) for l in levels for it in l]
        plan = LW.expected_plan(c, batch)
        assert plan['levels'] == got['levels'] and plan['items'] == got['item_counts']


def test_clip_live_report(cases):
    c = cases['clip_live']
    rep = LW.clip_report(c)
    print('clip_live (seed attempt %d): %r' % (c['attempt'], rep))
    assert LW.clip_ok(rep, c['B'])
    assert rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0 and rep['margin'] > LW.CLIP_MARGIN
    assert all(0 < k < c['B'] for k in rep['labels_clipped'])


def test_binding_lists_the_ll_wfold_symbols(hip_lib):
    """include/sert_hip_ll_wfold.h, which sert_hip.h includes, declares exactly _capi.EXPORTS_LL_WFOLD; the library exports
    them; the plan hook lives in sert_hip_debug.h; the ctypes config has the size of the C struct's fields."""
    read = lambda name: open(os.path.join(ROOT, 'include', name)).read()
    declared = sorted(set(re.findall(r'\b(sert_ll_wfold_[a-z_0-9]+)\s*\(', read('sert_hip_ll_wfold.h'))))
    assert declared == sorted(_capi.EXPORTS_LL_WFOLD)
    assert '#include "sert_hip_ll_wfold.h"' in read('sert_hip.h')
    assert "'sert_hip_ll_wfold.h'" in open(os.path.join(ROOT, 'sert_amd', '_build.py')).read()
    assert not [s for s in _capi.EXPORTS_LL_WFOLD if not hasattr(hip_lib, s)]
    assert not set(_capi.EXPORTS_LL_WFOLD) & set(_capi.EXPORTS + _capi.EXPORTS_FOLDIN + _capi.EXPORTS_LL_FOLDIN + _capi.EXPORTS_WFOLD)
    assert 'sert_debug_ll_wfold_plan' in read('sert_hip_debug.h') and 'sert_debug_ll_wfold_plan' not in read('sert_hip_ll_wfold.h')
    assert hasattr(hip_lib, 'sert_debug_ll_wfold_plan') and 'sert_debug_ll_wfold_plan' in _capi.EXPORTS
    assert ctypes.sizeof(_capi.SertLlWFoldConfig) == 32
    # null handles are refused without a device
    cfg = _capi.SertLlWFoldConfig()
    cfg.struct_size = ctypes.sizeof(_capi.SertLlWFoldConfig)
    h = ctypes.c_void_p()
    assert hip_lib.sert_ll_wfold_create(None, 1, None, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'null argument' in hip_lib.sert_last_error()
    assert hip_lib.sert_ll_wfold_num_batches(None) < 0
    v = (ctypes.c_int32 * 16)()
    assert hip_lib.sert_debug_ll_wfold_plan(None, v, 16) != 0 and b'bad argument' in hip_lib.sert_last_error()
