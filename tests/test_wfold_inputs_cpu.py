"""CPU: the inputs of the word fold-in tests have the structure they exist for (tests/wfold_cases.py), the index builder
(csrc/wfold_index.h, through the host-only sert_debug_wfold_index) builds what the contract states, the identity the device
path rests on holds in float64, and the same reassociated form in float32 NumPy stays inside the row bounds.  No device.

The reassociated form (A0 + sum P / n; S W^T with one division by n per word) in float32 against the float64 twin after the 3
steps, worst row-wise error of Nv / m / v per case (bound: tests.util.ROW_TOL64 = 5e-5 for all three):
    case              Nv       m        v
    all_new           7.1e-08  3.0e-07  1.3e-05
    base              7.6e-08  4.0e-07  1.3e-05
    empty_batch       1.7e-07  3.4e-07  1.3e-05
    heavy             4.9e-08  2.1e-07  1.3e-05
    heavy3            8.7e-08  1.2e-06  1.1e-05
    many_cands        1.2e-07  3.3e-07  1.3e-05
    many_words        1.3e-06  5.2e-07  1.3e-05
    odd_de            9.5e-08  2.9e-07  1.3e-05
    odd_dw            1.2e-07  3.0e-07  1.3e-05
    ragged            1.0e-07  2.6e-07  1.3e-05
    twice_in_window   1.0e-07  2.9e-07  1.3e-05
    wide              8.1e-08  3.8e-07  1.3e-05
(v: the float32 rounding of oracle.Adam's own (1 - beta2) g^2 accumulation, the same in every case.)
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi
from tests import util as U
from tests import wfold_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cases():
    return {name: WC.make_case(name) for name in WC.CASES}


@pytest.mark.parametrize('name', sorted(WC.CASES))
def test_case_has_its_structure(cases, name):
    c = cases[name]
    Vw, Nw, Ve, n, z, B = (c[k] for k in ('Vw', 'Nw', 'Ve', 'n', 'z', 'B'))
    X, tok = c['X'], WC.new_tokens(c)
    assert X.shape == (c['M'], n) and X.min() >= 0 and X.max() < Vw + Nw
    assert c['y'].min() >= 0 and c['y'].max() < Ve
    assert c['neg'].shape == (WC.STEPS, B, z) and c['neg'].min() >= 0 and c['neg'].max() < Ve
    assert c['M'] % B != 0 and c['M'] // B == c['batches'] >= WC.STEPS      # a tail that is never visited
    per_batch = [tok[i * B:(i + 1) * B] for i in range(c['batches'])]
    counts = [np.bincount(t[t >= 0], minlength=Nw) for t in per_batch]
    if name == 'base':
        assert X.min() < Vw and X.max() >= Vw
        assert counts[0].max() >= 2
        assert any(len(set(r[r >= 0].tolist())) >= 2 for r in per_batch[0])
        assert any((r < 0).all() for r in per_batch[0])
        assert counts[0][Nw - 1] == 0 and counts[0][:Nw - 1].min() > 0
    elif name == 'ragged':
        assert B % 16 != 0
    elif name == 'wide':
        assert c['de'] % 4 == 0 and c['de'] // 4 > 16
    elif name == 'odd_de':
        assert c['de'] % 4 != 0
    elif name == 'odd_dw':
        assert c['dw'] % 4 != 0 and c['de'] % 4 == 0
    elif name == 'many_cands':
        assert z + 1 > 16
    elif name == 'twice_in_window':
        assert all(any((r >= 0).all() and len(set(r.tolist())) == 1 for r in t) for t in per_batch)
    elif name == 'empty_batch':
        assert counts[1].sum() == 0 and counts[0].sum() > 0 and counts[2].sum() > 0
    elif name == 'all_new':
        assert X.min() >= Vw
    elif name == 'heavy':
        assert Nw == 1 and all((t >= 0).any(axis=1).all() for t in per_batch)
        assert all(WC.CHUNK < k[0] <= WC.CHUNK ** 2 for k in counts)
    elif name == 'heavy3':
        assert Nw == 1 and all(k[0] == B * n > WC.CHUNK ** 2 for k in counts)
        assert (B - 1) * n <= WC.CHUNK ** 2             # B is just large enough
    elif name == 'many_words':
        assert all((k == 0).sum() > Nw // 2 for k in counts)


@pytest.mark.parametrize('name', sorted(WC.CASES))
def test_index_builder_builds_the_stated_index(hip_lib, cases, name):
    """Per batch: the entries, their order, the chunking and the levels of the library's builder against the rule restated
    from the case's constants (wfold_cases.index_of_batch)."""
    c = cases[name]
    B, n, Nw = c['B'], c['n'], c['Nw']
    tok = WC.new_tokens(c)[:c['batches'] * B].reshape(c['batches'], B, n)
    for batch in range(c['batches']):
        got = _capi.debug_wfold_index(tok, Nw, batch)
        rows, levels = WC.index_of_batch(c, batch)
        assert got['levels'] == len(levels) and got['item_counts'] == [len(l) for l in levels]
        assert np.array_equal(got['rows'], rows) and len(rows) == int((tok[batch] >= 0).sum())
        flat = [it + (0,) for l in levels for it in l]
        assert got['items'].tolist() == [list(it) for it in flat]
        # every word of the batch has exactly one final item; a level's partial rows are numbered in item order
        finals = [it[2] for l in levels for it in l if it[2] >= 0]
        assert sorted(finals) == sorted(set(tok[batch][tok[batch] >= 0].tolist()))
        off = 0
        for l, items in enumerate(levels):
            assert got['part_off'][l] == off
            parts = [-(it[2] + 1) for it in items if it[2] < 0]
            assert parts == list(range(len(parts))) and all(0 < it[1] - it[0] <= WC.CHUNK for it in items)
            off += len(parts)
    expect = {'heavy': 2, 'heavy3': 3, 'empty_batch': 1}.get(name, 1)
    assert _capi.debug_wfold_index(tok, Nw, 0)['levels'] == expect
    if name == 'empty_batch':
        assert _capi.debug_wfold_index(tok, Nw, 1)['levels'] == 0
    if name == 'heavy3':
        assert _capi.debug_wfold_index(tok, Nw, 0)['item_counts'] == [65, 2, 1]


def test_index_hook_refuses_bad_arguments(hip_lib):
    tok = np.zeros((1, 4, 2), np.int32)
    with pytest.raises(_capi.SertError, match='out of range'):
        _capi.debug_wfold_index(tok + 3, 3)
    with pytest.raises(_capi.SertError, match='bad argument'):
        _capi.debug_wfold_index(tok, 3, batch=1)
    v = (ctypes.c_int32 * 16)()
    assert hip_lib.sert_debug_wfold_plan(None, v, 16) != 0 and b'bad argument' in hip_lib.sert_last_error()


def test_index_builder_stand_alone(tmp_path):
    """tools/wfold_index_check.cpp -- the builder's header alone, walked the way the segmented-sum kernels walk it, over random
    token arrays with one, two and three levels -- built with -fsanitize=address,undefined where the host compiler links it."""
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    out = str(tmp_path / 'wfold_index_check')
    base = [cxx, '-std=c++17', '-O1', '-g', '-I', os.path.join(ROOT, 'sert_amd', 'csrc'),
            os.path.join(ROOT, 'tools', 'wfold_index_check.cpp'), '-o', out]
    # The build is chosen on the program's trivial "probe" run alone: whether a sanitized binary links and starts here.  (The
    # sanitizer runtimes linked statically first: the program must run whatever else the environment loads into a process.)
    # The full run of the chosen build is then held to exit status 0, so a sanitizer report fails the test.
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    for extra, mode in ((san + ['-static-libasan', '-static-libubsan'], 'address,undefined'), (san, 'address,undefined'),
                        ([], 'none')):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode == 0 and subprocess.run([out, 'probe'], stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE).returncode == 0:
            break
    else:
        raise AssertionError('tools/wfold_index_check.cpp does not build or start: %s' % r.stdout.decode()[-2000:])
    print('sanitizers: %s' % mode)
    run = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == b'ok', (mode, run.stdout, run.stderr[-2000:])


def _reassociated(c, Nv, batch, neg, dt):
    """One step's loss (data term) and data gradient of Nv in the form the device path computes, in dtype dt.  The NCE maths is
    the oracle's: a surrogate VectorSpaceOracle whose window is one token, whose word table is the pre-activation a itself and
    whose projection is the identity has a = a @ I + 0 exactly, and its dh = da @ I is da."""
    dt = np.dtype(dt)
    B, n, Vw, de = c['B'], c['n'], c['Vw'], c['de']
    sl = slice(batch * B, (batch + 1) * B)
    X, y, w = c['X'][sl], c['y'][sl], c['w'][sl]
    tok = np.where(X >= Vw, X - Vw, -1)
    Rw0 = np.concatenate([c['Rw'], np.zeros((1, c['dw']), np.float32)]).astype(dt)
    hf = Rw0[np.where(tok < 0, X, Vw)[:, 0]].copy()
    for j in range(1, n):
        hf += Rw0[np.where(tok < 0, X, Vw)[:, j]]
    hf = (hf / dt.type(n)).astype(dt)
    A0 = (hf @ c['W'].astype(dt) + c['b'].astype(dt)).astype(dt)
    P = (Nv.astype(dt) @ c['W'].astype(dt)).astype(dt)
    s = np.zeros((B, de), dt)
    for j in range(n):                                   # positions ascending
        s += np.where((tok[:, j] >= 0)[:, None], P[np.maximum(tok[:, j], 0)], dt.type(0))
    a = (A0 + s / dt.type(n)).astype(dt)
    sur = O.VectorSpaceOracle(B, 1, c['z'], a, c['Re'], np.eye(de), np.zeros(de), 0.0, dtype=dt)
    data, _, f = sur.loss_and_grads(np.arange(B)[:, None], y, w, neg)
    S = np.zeros((c['Nw'], de), dt)
    r, j = np.nonzero(tok >= 0)
    np.add.at(S, tok[r, j], f['dh'][r])                  # (sequential: ascending by (row, position) per word)
    S = (S / dt.type(n)).astype(dt)
    return a, data, (S @ c['W'].astype(dt).T).astype(dt)


@pytest.mark.parametrize('name', sorted(WC.CASES))
def test_identity_holds_in_float64(cases, name):
    """A0 + (1/n) sum P against the oracle's a, and (sum DA / n) W^T against the data term of grads[1][V_w:]: 1e-12 relative."""
    c = cases[name]
    B, Vw = c['B'], c['Vw']
    tw = WC.WordFoldInTwin(c, np.float64)
    for s in range(WC.STEPS):
        a, data, G = _reassociated(c, tw.Nv, s, c['neg'][s], np.float64)
        X, y, w = tw._batch(s)
        ref_data, grads, f = tw._oracle(0.0).loss_and_grads(X, y, w, c['neg'][s])
        assert np.abs(a - f['a']).max() <= 1e-12 * np.abs(f['a']).max()
        ref = grads[1][Vw:]
        assert np.abs(G - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
        assert abs(data - ref_data) <= 1e-12 * abs(ref_data)
        if name == 'empty_batch' and s == 1:
            assert not ref.any() and not G.any()
        tw.train_step(s, c['neg'][s])


def reassociated_figures(c):
    """The 3 steps in the reassociated form in float32 (oracle.Adam on Nv) against the float64 twin: row errors of Nv, m, v."""
    lam, B = c['lam'], c['B']
    Nv = np.array(c['Nv0'], np.float32)
    opt = O.Adam([Nv], lr=c['lr'])
    t64 = WC.WordFoldInTwin(c, np.float64)
    for s in range(WC.STEPS):
        _, _, G = _reassociated(c, Nv, s, c['neg'][s], np.float32)
        opt.update([Nv], [(G + np.float32(lam / B) * Nv).astype(np.float32)])
        t64.train_step(s, c['neg'][s])
    return (U.row_err(Nv, t64.Nv)[0], U.row_err(opt.m[0], t64.m)[0], U.row_err(opt.v[0], t64.v)[0])


@pytest.mark.parametrize('name', sorted(WC.CASES))
def test_reassociated_float32_form_meets_the_row_bounds(cases, name):
    e_p, e_m, e_v = reassociated_figures(cases[name])
    print('%s: Nv %.1e m %.1e v %.1e' % (name, e_p, e_m, e_v))
    assert e_p < U.ROW_TOL64 and e_m < U.ROW_TOL64 and e_v < U.ROW_TOL64, (name, e_p, e_m, e_v)


def test_twin_follows_the_contract(cases):
    """The twin on the base case against a direct use of the oracle on the extended word table: the gradient of the trained
    rows is dropped, the new rows' is the oracle's, the loss is the data term plus lambda / (2B) sum(Nv Nv), frozen inputs are
    not written, and a row no token touched still moves."""
    c = cases['base']
    tw = WC.WordFoldInTwin(c)
    keys = ('Rw', 'Re', 'W', 'b', 'Nv0')
    before = [c[k].copy() for k in keys]
    B, Vw = c['B'], c['Vw']
    ext = np.concatenate([c['Rw'], c['Nv0']])
    ora = O.VectorSpaceOracle(B, c['n'], c['z'], ext, c['Re'], c['W'], c['b'], 0.0)
    data, grads, _ = ora.loss_and_grads(c['X'][:B], c['y'][:B], c['w'][:B], c['neg'][0])
    loss = tw.train_step(0, c['neg'][0])
    reg = c['lam'] / (2.0 * B) * float((c['Nv0'].astype(np.float64) ** 2).sum())
    assert abs(float(loss) - (float(data) + reg)) <= 1e-6 * abs(float(loss))
    g = grads[1][Vw:] + np.float32(c['lam'] / B) * c['Nv0']
    assert np.allclose(tw.m, 0.1 * g, rtol=1e-5, atol=1e-9)             # Adam's first moment after one step from zero
    assert not grads[1][Vw + c['Nw'] - 1].any()                          # the word absent from batch 0: no data term ...
    assert not np.array_equal(tw.Nv[-1], c['Nv0'][-1])                   # ... and it moved all the same
    for k, b in zip(keys, before):
        assert np.array_equal(c[k], b), k
    Nv1 = tw.Nv.copy()
    assert np.isfinite(tw.eval_loss(1, c['eval_neg'])) and np.array_equal(tw.Nv, Nv1)


def test_binding_lists_the_wfold_symbols(hip_lib):
    """include/sert_hip_wfold.h, which sert_hip.h includes, declares exactly _capi.EXPORTS_WFOLD; the library exports them;
    the two hooks are in the debug header only; the config struct of the binding has the header's size."""
    read = lambda f: re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', f)).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(sert_wfold_[a-z_0-9]+)\s*\(', read('sert_hip_wfold.h'))))
    assert declared == sorted(_capi.EXPORTS_WFOLD)
    assert '#include "sert_hip_wfold.h"' in read('sert_hip.h')
    assert "'sert_hip_wfold.h'" in open(os.path.join(ROOT, 'sert_amd', '_build.py')).read()
    assert not [s for s in _capi.EXPORTS_WFOLD if not hasattr(hip_lib, s)]
    assert not set(_capi.EXPORTS_WFOLD) & set(_capi.EXPORTS + _capi.EXPORTS_FOLDIN + _capi.EXPORTS_LL_FOLDIN)
    for hook in ('sert_debug_wfold_plan', 'sert_debug_wfold_index'):
        assert hook in read('sert_hip_debug.h') and hook not in read('sert_hip_wfold.h')
        assert hook in _capi.EXPORTS and hasattr(hip_lib, hook)
    assert ctypes.sizeof(_capi.SertWFoldConfig) == 40
    # no device: a null model is refused with a message
    cfg = _capi.SertWFoldConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    h = ctypes.c_void_p()
    assert hip_lib.sert_wfold_create(None, 1, None, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'null argument' in hip_lib.sert_last_error()
    assert hip_lib.sert_wfold_num_batches(None) < 0
