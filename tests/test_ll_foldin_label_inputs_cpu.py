"""CPU: the inputs of the loglinear fold-in tests on label rows (tests/ll_foldin_label_cases.py) are canonical CSR and have the
structure each case is named for, proved with NumPy and the oracle twin; clip_live_labels meets its clip conditions; label rows
are not their one-hot expansion; the binding has sert_ll_foldin_upload_csr with the header's prototype."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse

from oracle import sert_oracle as O
from sert_amd import _capi, training
from tests import ll_foldin_cases as LC
from tests import ll_foldin_label_cases as LL
from tests.util import ROOT


@pytest.fixture(scope='module', params=sorted(LL.CASES))
def case(request):
    return LL.make_case(request.param)


def _row(c, i):
    a, b = c['indptr'][i], c['indptr'][i + 1]
    return c['indices'][a:b], c['data'][a:b]


def test_rows_are_canonical_csr(case):
    c = case
    B, n, M, V = c['B'], c['n'], c['M'], c['Ve'] + c['N']
    assert M == 3 * B + LL.TRAILING and c['batches'] == M // B >= LL.STEPS and 1 <= n <= 32
    assert c['X'].shape == (M, n) and c['X'].dtype == np.int32 and c['X'].min() >= 0 and c['X'].max() < c['Vw']
    assert c['w'].shape == (M,) and c['Wn0'].shape == (c['d'], c['N']) and c['bn0'].shape == (c['N'],)
    indptr, indices, data = c['indptr'], c['indices'], c['data']
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.shape == (M + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all() and indptr[-1] == indices.size == data.size
    assert indices.size == 0 or (indices.min() >= 0 and indices.max() < V)
    for i in range(M):
        assert (np.diff(_row(c, i)[0]) > 0).all(), (c['name'], i)            # strictly increasing: sorted, no duplicate
    assert np.isfinite(data).all()
    # scipy agrees that this is canonical, and the dense rows the twin uses are these rows
    Y = scipy.sparse.csr_matrix((data, indices, indptr), shape=(M, V))
    assert Y.has_canonical_format and np.array_equal(Y.toarray(), c['Ydense'])
    assert LL.make_case(c['name']) is c                     # (generated once: the tests share it and leave it unchanged)


def test_named_structure():
    """Each case's mechanism, from its arrays and the twin."""
    C = {k: LL.make_case(k) for k in LL.CASES}
    counts = lambda c: np.diff(c['indptr'])
    # mixed
    c = C['mixed']
    Ve, N, B = c['Ve'], c['N'], c['B']
    V = Ve + N
    assert counts(c).tolist() == [V if k is None else k for k in (LL.MIXED_COUNTS * c['M'])[:c['M']]]
    for batch in range(3):
        assert set(counts(c)[batch * B:(batch + 1) * B].tolist()) == {0, 1, 2, 3, V}
    assert c['data'].min() >= 0.1 and c['data'].max() <= 1.0
    sums = c['Ydense'].sum(axis=1)
    assert (np.abs(sums[counts(c) > 0] - 1) > 1e-3).all()                    # no row is a distribution
    first = [_row(c, i)[0].tolist() for i in range(B)]
    assert any(len(r) == 1 and r[0] < Ve for r in first) and any(len(r) == 1 and r[0] >= Ve for r in first)
    assert [Ve - 1, Ve] in first and [0, V - 1] in first
    # frozen_only: batch 0 on trained columns alone, and a gradient of the new columns all the same
    c = C['frozen_only']
    assert c['indices'][:c['indptr'][c['B']]].max() < c['Ve'] and (counts(c)[:c['B']] > 0).all()
    _, gW, gb = LL.LlLabelTwin(c).train_step(0, return_grads=True)
    data_gW = gW - np.float32(c['lam'] / c['B']) * c['Wn0']                  # (without the L2 term)
    print('frozen_only: |gW|max %.3e (data term %.3e), |gb|max %.3e' % (np.abs(gW).max(), np.abs(data_gW).max(), np.abs(gb).max()))
    assert np.abs(data_gW).max() > 1e-3 and np.abs(gb).max() > 1e-3
    # no_labels: the twin's loss of batch 0 is exactly 0 and its step leaves Wn, bn alone
    c = C['no_labels']
    assert c['lam'] == 0.0 and c['indptr'][c['B']] == 0 and (counts(c)[c['B']:] > 0).all()
    tw = LL.LlLabelTwin(c)
    assert float(tw.train_step(0)) == 0.0 and np.array_equal(tw.Wn, c['Wn0']) and np.array_equal(tw.bn, c['bn0'])
    # one_hot: the integer case `base`, as rows
    c, b = C['one_hot'], LC.make_case('base')
    assert (counts(c) == 1).all() and (c['data'] == 1).all() and np.array_equal(c['indices'], b['Ve'] + b['y'])
    assert all(c[k] is b[k] for k in ('Rw', 'W', 'b', 'Wn0', 'bn0', 'X', 'w'))
    for s in range(LL.STEPS):
        assert float(LL.LlLabelTwin(c).train_step(s)) == float(LC.LlFoldInTwin(b).train_step(s))
    # wide
    c = C['wide']
    Ve, B = c['Ve'], c['B']
    assert (Ve, c['N']) == (700, 300)
    for batch in range(3):
        assert tuple(counts(c)[batch * B:batch * B + 4].tolist()) == LL.WIDE_COUNTS == (255, 256, 257, 600)
        for k in range(4):
            cols = _row(c, batch * B + k)[0]
            assert (cols < Ve).any() and (cols >= Ve).any()                  # both sides of the seam
        assert (_row(c, batch * B + 3)[0] >= Ve).sum() == LL.WIDE_TAIL > 256
    # the NMAX buckets: one trained and one new entry per row
    assert (C['n1']['n'], C['n9']['n'], C['n32']['n']) == (1, 9, 32)
    for k in ('n1', 'n9', 'n32', 'clip_live_labels'):
        c = C[k]
        assert (counts(c) == 2).all() and (c['indices'][0::2] < c['Ve']).all() and (c['indices'][1::2] >= c['Ve']).all()
    assert (C['clip_live_labels']['data'] == 0.5).all()
    assert C['odd_d']['d'] % 4 and C['batch_of_one']['B'] == 1 and C['batch_of_one']['batches'] == 3 + LL.TRAILING
    c = C['stored_zero']
    zero_rows = [i for i in range(c['M']) if (_row(c, i)[1] == 0).any()]
    assert zero_rows and all(i < 3 * c['B'] for i in zero_rows[:3]) and all((counts(c) == 3).tolist())
    assert all(k == 'stored_zero' or (C[k]['data'] != 0).all() for k in C)


def test_twin_overrides_only_the_batch():
    """The twin is LlFoldInTwin with `_batch` replaced: nothing else is defined on it, and its gradient is the extended
    oracle's on the dense rows, columns V_e onward."""
    assert [k for k in vars(LL.LlLabelTwin) if not k.startswith('__')] == ['_batch']
    c = LL.make_case('mixed')
    B, Ve = c['B'], c['Ve']
    Wx, bx = np.concatenate([c['W'], c['Wn0']], axis=1), np.concatenate([c['b'], c['bn0']])
    data, grads, _ = O.LogLinearOracle(B, c['n'], c['Rw'], Wx, bx, 0.0).loss_and_grads(c['X'][:B], c['Ydense'][:B], c['w'][:B])
    loss, gW, gb = LL.LlLabelTwin(c).train_step(0, return_grads=True)
    reg = c['lam'] / (2.0 * B) * float((c['Wn0'].astype(np.float64) ** 2).sum())
    assert abs(float(loss) - (float(data) + reg)) <= 1e-6 * abs(float(loss))
    assert np.allclose(gW, grads[1][:, Ve:] + np.float32(c['lam'] / B) * c['Wn0'], rtol=1e-5, atol=1e-9)
    assert np.array_equal(gb, grads[2][Ve:])


def test_clip_live_labels_conditions():
    """clip_live_labels over its three steps on the float64 twin: in every step some but not all trained label entries and
    some but not all new label entries have Q below the clip bound; frozen and new token probabilities are clipped; no P and
    no label Q within relative 1e-3 of a bound; the gradient is finite and non-zero."""
    c = LL.make_case('clip_live_labels')
    rep = LL.clip_report(c)
    print('clip_live_labels (seed attempt %d): %d of %d frozen and %d of %d new token probabilities clipped; label entries '
          'clipped per step: trained %r, new %r of %d; margin %.2e' %
          (c['attempt'], rep['frozen_clipped'], rep['frozen_total'], rep['new_clipped'], rep['new_total'],
           rep['trained_labels_clipped'], rep['new_labels_clipped'], c['B'], rep['margin']))
    assert c['attempt'] < 400
    assert rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0
    for key in ('trained_labels_clipped', 'new_labels_clipped'):
        assert len(rep[key]) == LL.STEPS and all(0 < k < c['B'] for k in rep[key])
    assert rep['margin'] > LL.CLIP_MARGIN
    assert rep['finite'] and rep['grad_nonzero']
    assert LL.clip_ok(rep, c['B'])


def test_label_rows_are_not_their_one_hot_expansion():
    """mixed, batch 0: the loss of the rows against the loss of their expansion by training.sparse_to_one_hot_multiple (one
    instance of label 1 per stored entry -- what bin/fold_in.py does without --label_distributions; rows without an entry
    have no instance), both summed over the batch's rows and divided by B.  They differ by far more than the GPU test's 1e-5."""
    c = LL.make_case('mixed')
    B, Ve, V = c['B'], c['Ve'], c['Ve'] + c['N']
    Wx, bx = np.concatenate([c['W'], c['Wn0']], axis=1), np.concatenate([c['b'], c['bn0']])
    orc = O.LogLinearOracle(B, c['n'], c['Rw'], Wx, bx, 0.0, dtype=np.float64)
    rows = float(orc.forward(c['X'][:B], c['Ydense'][:B])['loss'].sum()) / B
    Y = scipy.sparse.csr_matrix((c['data'], c['indices'], c['indptr']), shape=(c['M'], V))[:B]
    keep = np.diff(Y.indptr) > 0
    ids, (X,) = training.sparse_to_one_hot_multiple(Y[keep], c['X'][:B][keep])
    assert ids.size == Y.nnz and X.shape == (Y.nnz, c['n'])
    expansion = float(orc.forward(X, ids)['loss'].sum()) / B
    print('mixed batch 0: loss of the rows %.6f, of their one-hot expansion %.6f' % (rows, expansion))
    assert abs(expansion - rows) > 1e-2 * abs(rows)


def test_label_columns_of_a_new_meta():
    """foldin.label_columns: an id the trained meta knows maps to its trained index, an unknown one to V_e + its position among
    the unknown ones; the merged meta keeps every trained index, appends the unknown ids and adds the associations to either
    kind.  foldin.remap_label_columns moves the columns of a sparse label matrix there and leaves canonical CSR."""
    from sert_amd import foldin
    meta = ['args', ['w0', 'w1'], 'tokens', {0: 'a', 1: 'b', 2: 'c'}, {'a': ['d1'], 'b': ['d2'], 'c': ['d3']}]
    ids = ['x', 'c', 'y', 'a']
    merged, columns, new_ids = foldin.label_columns(meta, ids, {'x': ['n1'], 'c': ['n1', 'n2'], 'y': ['n2'], 'a': []})
    assert columns.dtype == np.int32 and columns.tolist() == [3, 2, 4, 0] and new_ids == ['x', 'y']
    assert merged[:3] == meta[:3] and merged[3] == {0: 'a', 1: 'b', 2: 'c', 3: 'x', 4: 'y'}
    assert merged[4] == {'a': ['d1'], 'b': ['d2'], 'c': ['d3', 'n1', 'n2'], 'x': ['n1'], 'y': ['n2']}
    assert meta[3] == {0: 'a', 1: 'b', 2: 'c'} and meta[4]['c'] == ['d3']                      # (the caller's meta is not modified)
    _, columns, new_ids = foldin.label_columns(meta, ['b', 'a'])
    assert columns.tolist() == [1, 0] and new_ids == []                                      # (nothing to fold in)
    with pytest.raises(RuntimeError, match='duplicate'):
        foldin.label_columns(meta, ['x', 'x'])
    # rows over the new meta's four entities -> rows over V_e + N = 5 columns; a stored 0 stays stored
    y = scipy.sparse.csr_matrix((np.array([0.5, 0.5, 1.0, 0.0, 1.0], np.float32), np.array([0, 1, 2, 0, 3]), np.array([0, 2, 3, 3, 5])),
                                shape=(4, 4))
    Y = foldin.remap_label_columns(y, [3, 2, 4, 0], 5)
    assert Y.shape == (4, 5) and Y.has_canonical_format and Y.dtype == np.float32 and Y.nnz == 5
    assert Y.indptr.tolist() == [0, 2, 3, 3, 5] and Y.indices.tolist() == [2, 3, 4, 0, 3]
    assert Y.data.tolist() == [0.5, 0.5, 1.0, 1.0, 0.0]


def test_binding_has_the_csr_upload(hip_lib):
    """The header declares sert_ll_foldin_upload_csr with the issue's prototype, the binding lists it and gives it seven
    arguments, the library exports it; LlFoldIn has upload_csr; a null handle is refused with a message."""
    src = open(os.path.join(ROOT, 'include', 'sert_hip_ll_foldin.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    assert ('int sert_ll_foldin_upload_csr(sert_ll_foldin* f, const int32_t* x, const int64_t* indptr, const int32_t* indices, '
            'const float* data, const float* w, int64_t M);') in flat
    assert 'sert_ll_foldin_upload_csr' in _capi.EXPORTS_LL_FOLDIN and hasattr(hip_lib, 'sert_ll_foldin_upload_csr')
    fn = _capi.load().sert_ll_foldin_upload_csr
    assert len(fn.argtypes) == 7 and fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[-1] is ctypes.c_int64
    assert all(t is ctypes.c_void_p for t in fn.argtypes[1:6])
    assert callable(getattr(_capi.LlFoldIn, 'upload_csr', None))
    assert 'CSR label rows' not in src                      # (no longer out of scope)
    assert fn(None, None, None, None, None, None, 0) != 0
    assert b'bad argument' in hip_lib.sert_last_error()
