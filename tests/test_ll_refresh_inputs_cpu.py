"""CPU: the inputs of the refreshing loglinear fold-in tests (tests/ll_refresh_cases.py) have the structure each case is named
for; their label rows are canonical CSR; clip_live meets its clip conditions; the twin agrees in float64 with the existing
LlFoldInTwin on the column-deleted problem; the host remap of label rows (csrc/ll_label_remap.h) passes a stand-alone
sanitizer build; the binding, the debug hook and the command line have the new entry points."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

from sert_amd import _capi
from tests import ll_foldin_cases as LC
from tests import ll_foldin_label_cases as LL
from tests import ll_refresh_cases as RC
from tests.util import ROOT


@pytest.fixture(scope='module', params=sorted(RC.CASES))
def case(request):
    return RC.make_case(request.param)


def _row(c, i):
    a, b = c['indptr'][i], c['indptr'][i + 1]
    return c['indices'][a:b], c['data'][a:b]


def test_shapes_and_slots(case):
    c = case
    B, n, M, Ve, N, R, d = c['B'], c['n'], c['M'], c['Ve'], c['N'], c['R'], c['d']
    assert M == 3 * B + RC.TRAILING and c['batches'] == M // B >= RC.STEPS
    assert c['refresh'].dtype == np.int32 and c['refresh'].shape == (R,) and np.unique(c['refresh']).size == R
    assert R >= 1 and c['refresh'].min() >= 0 and c['refresh'].max() < Ve
    assert c['Nt'] == R + N >= 1 and c['Vf'] == Ve - R >= 0
    assert c['ext_of_slot'].tolist() == c['refresh'].tolist() + list(range(Ve, Ve + N))
    assert c['W'].shape == (d, Ve) and c['b'].shape == (Ve,) and c['Wn0'].shape == (d, N) and c['bn0'].shape == (N,)
    assert c['X'].shape == (M, n) and c['X'].dtype == np.int32 and c['X'].min() >= 0 and c['X'].max() < c['Vw']
    io = RC.internal_of(c)
    assert sorted(io.tolist()) == list(range(Ve + N))                      # a bijection of the public columns
    frozen = np.setdiff1d(np.arange(Ve), c['refresh'])
    assert io[frozen].tolist() == list(range(c['Vf']))                     # frozen: ascending trained index
    assert io[c['ext_of_slot']].tolist() == list(range(c['Vf'], c['Vf'] + c['Nt']))     # slot s -> V_f + s
    if RC.is_csr(c):
        V = Ve + N
        indptr, indices, data = c['indptr'], c['indices'], c['data']
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
        assert indptr.shape == (M + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all() and indptr[-1] == indices.size == data.size
        assert indices.min() >= 0 and indices.max() < V and np.isfinite(data).all()
        for i in range(M):
            assert (np.diff(_row(c, i)[0]) > 0).all(), (c['name'], i)
        Y = scipy.sparse.csr_matrix((data, indices, indptr), shape=(M, V))
        assert Y.has_canonical_format and np.array_equal(Y.toarray(), c['Ydense'])
        # the column-deleted rows are canonical too, hold the same (column, value) pairs, and keep the frozen prefix
        p = RC.deleted(c)
        assert np.array_equal(p['indptr'], indptr)
        for i in range(M):
            cols, vals = _row(p, i)
            assert (np.diff(cols) > 0).all()
            pub, pv = _row(c, i)
            assert sorted(zip(io[pub].tolist(), pv.tolist())) == sorted(zip(cols.tolist(), vals.tolist()))
    else:
        assert c['y'].dtype == np.int32 and c['y'].shape == (M,) and c['y'].min() >= 0 and c['y'].max() < c['Nt']
    assert RC.make_case(c['name']) is c                     # (generated once: the tests share it and leave it unchanged)


def test_named_structure():
    """Each case's mechanism, from its arrays and the twin."""
    C = {k: RC.make_case(k) for k in RC.CASES}
    c = C['mixed']
    assert (c['Ve'], c['N']) == (7, 3) and c['refresh'].tolist() == [5, 1] and (np.diff(c['refresh']) < 0).any()
    assert set(np.unique(c['y'][:c['B']]).tolist()) == set(range(c['Nt']))            # every slot is a label of batch 0
    c = C['first_last']
    assert c['refresh'].tolist() == [0, c['Ve'] - 1]
    c = C['refresh_only']
    assert c['N'] == 0 and c['Nt'] == c['R'] == 3 and c['Wn0'].size == 0
    assert C['one_frozen']['Vf'] == 1
    c = C['all_refreshed']
    assert c['Vf'] == 0 and c['N'] == 2 and sorted(c['refresh'].tolist()) == list(range(c['Ve']))
    assert c['refresh'].tolist() != sorted(c['refresh'].tolist())
    for k in ('wide', 'csr_wide'):
        c = C[k]
        assert (c['Ve'], c['R'], c['N']) == (700, 300, 5) and {0, 699} <= set(c['refresh'].tolist())
        assert c['Nt'] == 305 > 256 and c['Vf'] == 400 and c['Vf'] % 256
    # unvisited_slot: no instance of any batch is labelled slot 2, and the slot moves in the twin's first step all the same
    c = C['unvisited_slot']
    assert c['R'] == 3 and not (c['y'] == 2).any() and set(c['y'].tolist()) == {0, 1, 3, 4}
    tw = RC.LlRefreshTwin(c)
    before = tw.Wt[:, 2].copy(), tw.bt[2].copy()
    _, gW, gb = tw.train_step(0, return_grads=True)
    data_g = gW[:, 2] - np.float32(c['lam'] / c['B']) * before[0]               # (without the L2 term)
    print('unvisited_slot: |gW[:, 2]|max %.3e (data term %.3e), gb[2] %.3e' % (np.abs(gW[:, 2]).max(), np.abs(data_g).max(), gb[2]))
    assert np.abs(data_g).max() > 1e-4 and abs(gb[2]) > 1e-4
    assert not np.array_equal(tw.Wt[:, 2], before[0]) and tw.bt[2] != before[1]
    # csr_mixed
    c = C['csr_mixed']
    B, Ve = c['B'], c['Ve']
    refreshed, frozen = set(c['refresh'].tolist()), set(range(Ve)) - set(c['refresh'].tolist())
    io = RC.internal_of(c)
    for batch in range(3):
        r = [_row(c, batch * B + k) for k in range(7)]
        kinds = lambda cols: (bool(set(cols) & frozen), bool(set(cols) & refreshed), bool((np.asarray(cols) >= Ve).any()))
        assert kinds(r[0][0].tolist()) == (True, True, True)
        pub = [e for e in r[0][0].tolist() if e in refreshed]
        assert pub == [1, 5] and io[pub].tolist() == [c['Vf'] + 1, c['Vf'] + 0]         # ascending in public, descending in slot
        assert r[1][0].tolist() == [1, 5] and r[2][0].size == 0
        assert r[3][1][0] == 0.0 and r[3][0][0] in frozen
        assert r[6][0].tolist() == list(range(Ve + c['N']))
    assert _row(c, B)[1][2] == 0.0 and _row(c, B)[0][2] in refreshed                    # a stored zero on a refreshed column
    # csr_wide: row 0 of every batch
    c = C['csr_wide']
    refreshed = set(c['refresh'].tolist())
    for batch in range(3):
        cols = _row(c, batch * c['B'])[0]
        nf = sum(1 for e in cols.tolist() if e < c['Ve'] and e not in refreshed)
        nr = sum(1 for e in cols.tolist() if e in refreshed)
        assert (nf, nr, int((cols >= c['Ve']).sum())) == RC.WIDE_ROW and cols.size >= 257 and cols.size - nf > 256
    c = C['csr_all_refreshed']
    assert c['Vf'] == 0 and c['indptr'][3] == c['indptr'][2] and (RC.deleted(c)['indices'] >= 0).all()


def test_clip_live_conditions():
    c = RC.make_case('clip_live')
    rep = RC.clip_report(c)
    print('clip_live (seed attempt %d): clipped token probabilities frozen %d of %d, refreshed %d of %d, new %d of %d; labels '
          'clipped per step %r of %d; margin %.2e' %
          (c['attempt'], rep['frozen_clipped'], rep['frozen_total'], rep['refreshed_clipped'], rep['refreshed_total'],
           rep['new_clipped'], rep['new_total'], rep['labels_clipped'], c['B'], rep['margin']))
    assert c['attempt'] < 400 and np.abs(c['W']).max() > 5
    assert rep['frozen_clipped'] > 0 and rep['refreshed_clipped'] > 0 and rep['new_clipped'] > 0
    assert len(rep['labels_clipped']) == RC.STEPS and all(0 < k < c['B'] for k in rep['labels_clipped'])
    assert rep['margin'] > RC.CLIP_MARGIN and rep['finite'] and rep['grad_nonzero']
    assert RC.clip_ok(rep, c['B'])


def test_twin_agrees_with_the_plain_twin_on_the_column_deleted_case(case):
    """float64: LlRefreshTwin on the case = LlFoldInTwin (LlLabelTwin for label rows) on the model of the frozen columns alone
    with Wn0 = [W[:, refresh], new] and remapped labels, in loss and state to 1e-10 relative over three steps -- only the
    order of the sum over the columns differs."""
    c = case
    p = RC.deleted(c)
    if c['Vf'] == 0:
        # (the plain twin concatenates a (d, 0) W: nothing else is special)
        assert p['W'].shape == (c['d'], 0) and p['b'].shape == (0,)
    a = RC.LlRefreshTwin(c, np.float64)
    b = (LL.LlLabelTwin if RC.is_csr(c) else LC.LlFoldInTwin)(p, np.float64)
    for s in range(RC.STEPS):
        la, lb = float(a.train_step(s)), float(b.train_step(s))
        assert abs(la - lb) <= 1e-10 * abs(lb), (c['name'], s, la, lb)
        ea, eb = float(a.eval_loss((s + 1) % 3)), float(b.eval_loss((s + 1) % 3))
        assert abs(ea - eb) <= 1e-10 * abs(eb), (c['name'], s, ea, eb)
    sa, sb = a.state(), b.state()
    for k in sa:
        scale = max(float(np.abs(sb[k]).max()), 1e-300)
        assert float(np.abs(sa[k] - sb[k]).max()) <= 1e-10 * scale, (c['name'], k)


def test_twin_restates_no_maths():
    """The twin's gradient is the extended oracle's, columns ext_of_slot; its extended tensors are W / b with the slots written
    to their columns."""
    from oracle import sert_oracle as O
    c = RC.make_case('mixed')
    B, ext = c['B'], c['ext_of_slot']
    tw = RC.LlRefreshTwin(c)
    Wx, bx = tw.extended()
    assert np.array_equal(Wx[:, :c['Ve']], c['W']) and np.array_equal(Wx[:, c['Ve']:], c['Wn0']) and np.array_equal(bx[c['Ve']:], c['bn0'])
    _, grads, _ = O.LogLinearOracle(B, c['n'], c['Rw'], Wx, bx, c['lam']).loss_and_grads(c['X'][:B], ext[c['y'][:B]], c['w'][:B])
    _, gW, gb = tw.train_step(0, return_grads=True)
    assert np.array_equal(gW, grads[1][:, ext]) and np.array_equal(gb, grads[2][ext])


# ---- the host remap under a sanitizer: a stand-alone program, on the CPU -------------------------------------------------

def _remap_program(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        return None, 'no host C++ compiler'
    out = str(tmp_path_factory.mktemp('ll_remap') / 'll_label_remap_check')
    base = [cxx, '-std=c++17', '-O1', '-g', '-I', os.path.join(ROOT, 'sert_amd', 'csrc'),
            os.path.join(ROOT, 'tools', 'll_label_remap_check.cpp'), '-o', out]
    # (the sanitizer runtimes linked statically: the program must run whatever else the environment loads into a process)
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        if r.returncode == 0 and subprocess.run([out], input=b'1 0 0 0 0', stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE).returncode == 0:
            return out, 'address,undefined'
    r = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)     # (no sanitizer runtime to link: plain)
    assert r.returncode == 0, r.stdout.decode()
    return out, 'none'


@pytest.fixture(scope='module')
def remap_program(tmp_path_factory):
    return _remap_program(tmp_path_factory)


def _run_remap(program, Ve, N, refresh, indptr, indices, data):
    text = ' '.join(str(int(v)) for v in [Ve, N, len(refresh), len(indptr) - 1] + list(refresh) + list(indptr) + list(indices) +
                    list(np.asarray(data, np.float32).view(np.uint32)))
    r = subprocess.run([program], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split('\n')
    return int(lines[0]), [np.array(line.split(), dtype=np.int64) for line in lines[1:4]]


def test_host_remap_stand_alone(remap_program):
    """tools/ll_label_remap_check.cpp, built with -fsanitize=address,undefined where the host compiler links it, over the rows
    of every CSR case: the layout and the remapped rows are NumPy's; bad ids are reported, not indexed with."""
    program, sanitizers = remap_program
    if program is None:
        pytest.skip(sanitizers)
    print('sanitizers: %s' % sanitizers)
    for name in RC.CSR_CASES:
        c = RC.make_case(name)
        status, (io, cols, bits) = _run_remap(program, c['Ve'], c['N'], c['refresh'], c['indptr'], c['indices'], c['data'])
        p = RC.deleted(c)
        assert status == 0 and np.array_equal(io, RC.internal_of(c))
        assert np.array_equal(cols, p['indices']) and np.array_equal(bits.astype(np.uint32), p['data'].view(np.uint32))
    # nothing refreshed: the identity
    c = LL.make_case('mixed')
    status, (io, cols, bits) = _run_remap(program, c['Ve'], c['N'], [], c['indptr'], c['indices'], c['data'])
    assert status == 0 and np.array_equal(io, np.arange(c['Ve'] + c['N'])) and np.array_equal(cols, c['indices'])
    assert np.array_equal(bits.astype(np.uint32), c['data'].view(np.uint32))
    # an id out of range on either side, a duplicate
    assert _run_remap(program, 7, 2, [7], [0], [], [])[0] == 1
    assert _run_remap(program, 7, 2, [-1], [0], [], [])[0] == 1
    assert _run_remap(program, 7, 2, [3, 3], [0], [], [])[0] == 2


# ---- the entry points (these fail on the parent commit) ------------------------------------------------------------------

def test_binding_has_create_refresh(hip_lib):
    """The header declares sert_ll_foldin_create_refresh with the issue's prototype, the binding lists it with eight
    arguments, the library exports it; a null model is refused with `null argument`."""
    src = open(os.path.join(ROOT, 'include', 'sert_hip_ll_foldin.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    assert ('int sert_ll_foldin_create_refresh(sert_model* m, const int32_t* refresh_ids, int32_t num_refresh, int32_t num_new, '
            'const float* init_new_W, const float* init_new_b, const sert_ll_foldin_config* cfg, sert_ll_foldin** out);') in flat
    assert 'refreshing trained columns' not in src                      # (no longer out of scope)
    assert 'sert_ll_foldin_create_refresh' in _capi.EXPORTS_LL_FOLDIN and hasattr(hip_lib, 'sert_ll_foldin_create_refresh')
    fn = _capi.load().sert_ll_foldin_create_refresh
    assert len(fn.argtypes) == 8 and fn.argtypes[2] is ctypes.c_int32 and fn.argtypes[3] is ctypes.c_int32
    cfg = _capi.SertLlFoldInConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    h = ctypes.c_void_p()
    assert fn(None, None, 0, 1, None, None, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'null argument' in hip_lib.sert_last_error() and not h
    import inspect
    params = inspect.signature(_capi.LlFoldIn.__init__).parameters
    assert 'refresh_ids' in params and params['refresh_ids'].default is None
    from sert_amd import foldin
    assert inspect.signature(foldin.LogLinearFoldIn.__init__).parameters['refresh'].default is None
    assert callable(foldin.refresh_ll_dump) and callable(foldin.LogLinearFoldIn.get_refreshed_dense)


def test_debug_hook_is_declared_in_the_debug_header_only(hip_lib):
    name = 'sert_debug_ll_foldin_layout'
    read = lambda f: open(os.path.join(ROOT, 'include', f)).read()
    assert name in read('sert_hip_debug.h')
    assert all(name not in read(f) for f in ('sert_hip.h', 'sert_hip_ll_foldin.h', 'sert_hip_foldin.h'))
    assert name in _capi.EXPORTS and name not in _capi.EXPORTS_LL_FOLDIN and hasattr(hip_lib, name)
    hip_lib.sert_debug_ll_foldin_layout.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                    ctypes.c_void_p, ctypes.c_int64]
    assert hip_lib.sert_debug_ll_foldin_layout(None, None, None, None, 0) != 0
    assert b'null argument' in hip_lib.sert_last_error()


def test_refresh_ll_dump_replaces_and_appends():
    from sert_amd import foldin, models
    rng = np.random.RandomState(0)
    d, Ve = 4, 5
    W, b, Rw = rng.randn(d, Ve).astype(np.float32), rng.randn(Ve).astype(np.float32), rng.randn(6, d).astype(np.float32)
    trained = models.LogLinearPredictFn(R_w=Rw, W=W, b=b, window_size=3)
    Wr, br, Wn, bn = rng.randn(d, 2).astype(np.float32), rng.randn(2).astype(np.float32), rng.randn(d, 1).astype(np.float32), np.ones(1, np.float32)
    args, fn, R_w = foldin.refresh_ll_dump('args', trained, Rw, [3, 0], Wr, br, Wn, bn)
    assert args == 'args' and R_w is Rw and fn.W.shape == (d, Ve + 1) and fn.b.shape == (Ve + 1,)
    assert np.array_equal(fn.W[:, [3, 0]], Wr) and np.array_equal(fn.b[[3, 0]], br)
    assert np.array_equal(fn.W[:, [1, 2, 4]], W[:, [1, 2, 4]]) and np.array_equal(fn.b[[1, 2, 4]], b[[1, 2, 4]])
    assert np.array_equal(fn.W[:, Ve:], Wn) and np.array_equal(fn.b[Ve:], bn)
    assert np.array_equal(trained.W, W) and np.array_equal(trained.b, b)            # (the trained predict_fn is not modified)
    _, fn, _ = foldin.refresh_ll_dump('args', trained, Rw, [2], Wr[:, :1], br[:1], np.zeros((d, 0), np.float32), np.zeros(0, np.float32))
    assert fn.W.shape == (d, Ve) and np.array_equal(fn.W[:, 2], Wr[:, 0])


def test_parser_has_unfreeze_known():
    sys.path.insert(0, os.path.join(ROOT, 'bin'))
    try:
        import importlib
        fold_in = importlib.import_module('fold_in')
    finally:
        sys.path.pop(0)
    parser = fold_in.build_parser()
    flags = [s for a in parser._actions for s in a.option_strings]
    assert '--unfreeze_known' in flags and '--refresh' in flags and '--label_distributions' in flags
    common = ['--meta', __file__, '--model', __file__, '--new_meta', __file__, '--data', __file__, '--iterations', '1',
              '--model_output', os.path.join(ROOT, 'no_such_dir', 'm'), '--meta_output', os.path.join(ROOT, 'no_such_dir', 'n')]
    assert parser.parse_args(common).unfreeze_known is False
    assert parser.parse_args(common + ['--unfreeze_known']).unfreeze_known is True
