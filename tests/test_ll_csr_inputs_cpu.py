"""No GPU: the problems of tests/ll_csr_cases.py are checkable.  For every case, on the oracle alone: no probability is near
a clip bound (engine and oracle cannot part over a mask), the float32 oracle sits within a quarter of every tolerance of
the GPU test from its own float64 evaluation (a failure there belongs to the engine), the gradients are not a
cancelled remainder, and -- for the two cases aimed at it -- a label fix-up list that stopped at four entries per thread of
a 128-thread row would move db by far more than the gradient tolerance.  Last, for the n = 65 case: a window summed term by
term in float32 stays inside the gradient bound and leaves the state bound, so the state check of the GPU test sees it."""
import numpy as np
import pytest

from oracle import sert_oracle as O
from tests import ll_csr_cases as K
from tests import util as U
from tests.test_gpu_parity import ACT_TOL, GRAD_TOL, LOSS_TOL, PARAM_TOL

NAMES = list(K.CASES)


def _rowloss_err(got, ref):
    """the figure _check_rowloss (test_gpu_parity.py) bounds by ACT_TOL"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).mean())).max())


def _db_from_dj(ora, f, dJ):
    """the oracle's backward from dJ to db (LogLinearOracle.loss_and_grads), in its dtype"""
    dt = ora.dtype
    lo, hi = O.clip_bounds(dt)
    P3 = f['P3']
    dP = dJ[:, None, :] * O._clip_mask(P3, lo, hi).astype(dt) / np.clip(P3, lo, hi)
    dZ = (P3 * (dP - O._sum(dP * P3, axis=2, dtype=dt)[:, :, None])).astype(dt)
    db = O._sum(dZ.reshape(-1, dZ.shape[2]), axis=0, dtype=dt)
    if ora.lam > 0.0 and O.UPSTREAM['bias_regularised']:
        db = db + dt.type(ora.lam) / dt.type(ora.B) * ora.b
    return db


@pytest.mark.parametrize('name', NAMES)
def test_case_is_built_as_stated(name):
    c, p = K.case_problem(name)
    y, Bc = p['y'], len(c['counts'])
    assert y.shape == (K.STEPS * Bc, c['Ve']) and p['X'].shape == (K.STEPS * Bc, c['n'])
    assert np.array_equal(np.diff(y.indptr), np.tile(c['counts'], K.STEPS))
    for r in range(y.shape[0]):
        cols = y.indices[y.indptr[r]:y.indptr[r + 1]]
        assert np.all(np.diff(cols) > 0) and (len(cols) == 0 or (cols[0] >= 0 and cols[-1] < c['Ve']))
    sums = np.asarray(y.sum(axis=1)).ravel()
    zr, zc = p['zero_at']
    for r in range(y.shape[0]):
        vals = y.data[y.indptr[r]:y.indptr[r + 1]]
        if r == p['unnormalised_row']:
            assert abs(sums[r] - 2.5) < 1e-4
        elif r == zr:
            assert (vals == 0).sum() == 1 and y.indices[y.indptr[r] + len(vals) // 2] == zc and len(vals) >= 2
        elif len(vals):
            assert abs(sums[r] - 1.0) < 1e-5 and vals.min() > 0
        else:
            assert sums[r] == 0
    assert int((y.data == 0).sum()) == 1                      # the stored zero is stored
    over = max(c['counts']) > K.LABEL_LIMIT
    assert over == (name in ('fallback_scalar', 'fallback_v4', 'stream'))


@pytest.mark.parametrize('name', NAMES)
def test_no_probability_is_near_a_clip_bound(name):
    c, p = K.case_problem(name)
    Bc = len(c['counts'])
    for dtype in (np.float32, np.float64):
        steps, _ = K.case_reference(name, dtype)
        for s, st in enumerate(steps):
            P3, Q = st['f']['P3'], st['f']['Q']
            lab = p['ydense'][s * Bc:(s + 1) * Bc] != 0
            sl = p['y'][s * Bc:(s + 1) * Bc]
            stored = np.zeros_like(lab)
            stored[np.repeat(np.arange(Bc), np.diff(sl.indptr)), sl.indices] = True      # (the stored zero as well)
            assert lab.sum() + (1 if s == 0 else 0) == stored.sum()
            print('%s step %d %s: token P in [%.2e, %.2e], label Q in [%.2e, %.2e]'
                  % (name, s, np.dtype(dtype).name, P3.min(), P3.max(), Q[stored].min(), Q[stored].max()))
            assert 1e-5 <= P3.min() and P3.max() <= 0.5
            assert 1e-5 <= Q[stored].min() and Q[stored].max() <= 0.5


@pytest.mark.parametrize('name', NAMES)
def test_float32_oracle_is_a_quarter_tolerance_from_float64(name):
    c, p = K.case_problem(name)
    Bc = len(c['counts'])
    s32, o32 = K.case_reference(name, np.float32)
    s64, o64 = K.case_reference(name, np.float64)
    # the parameters after the steps: where a tensor is small beside its own update, the parameter bound asks more of the
    # gradient than the gradient bound does -- the references must still agree to a quarter of it
    e_p = [U.rel_err(a, b) for a, b in zip(o32.params(), o64.params())]
    print('%s: oracle32 vs 64 after %d steps R_w %.1e W %.1e b %.1e (%.1e)' % (name, K.STEPS, e_p[0], e_p[1], e_p[2], PARAM_TOL / 4))
    assert max(e_p) < PARAM_TOL / 4
    for s, (a, b) in enumerate(zip(s32, s64)):
        w = p['w'][s * Bc:(s + 1) * Bc].astype(np.float64)
        e_loss = abs(float(a['loss']) - float(b['loss'])) / abs(float(b['loss']))
        e_row = _rowloss_err(w * a['f']['loss'], w * b['f']['loss'])
        e_g = [U.rel_err(x, y) for x, y in zip(a['grads'], b['grads'])]
        print('%s step %d: oracle32 vs 64 loss %.1e (%.1e) rowloss %.1e (%.1e) dRw %.1e dW %.1e db %.1e (%.1e)'
              % (name, s, e_loss, LOSS_TOL / 4, e_row, ACT_TOL / 4, e_g[0], e_g[1], e_g[2], GRAD_TOL / 4))
        assert e_loss < LOSS_TOL / 4
        assert e_row < ACT_TOL / 4
        assert max(e_g) < GRAD_TOL / 4
        # the gradients are no cancelled remainder: a plan with y ~ Q would leave rel_err nothing to price
        floor = 1e-3 * float(p['w'].max()) / Bc
        dRw, dW, db = b['grads']
        assert np.abs(db).max() >= floor and np.abs(dW).max() >= floor, (np.abs(db).max(), np.abs(dW).max(), floor)
        # empty rows: loss 0 and no gradient through J
        empty = np.asarray(c['counts']) == 0
        assert np.all(b['f']['loss'][empty] == 0) and np.all(b['f']['dJ'][empty] == 0)


@pytest.mark.parametrize('name', ['table128_small', 'table128_limit'])
def test_a_dropped_label_fixup_would_be_visible(name):
    """What a 128-thread row with four fix-up entries per thread computes: dJ without the Q_e dQ_e term of the labels at
    position 512 and later of their sorted row (thread t holds positions t, t + 128, t + 256, t + 384) -- s, the loss and the
    row loss are unchanged.  db through the rest of the oracle's backward must then miss the true db by more than ten
    gradient tolerances, or the GPU test could pass over such a kernel."""
    c, p = K.case_problem(name)
    Bc = len(c['counts'])
    assert max(c['counts']) > 512 and max(c['counts']) <= K.LABEL_LIMIT
    for dtype in (np.float32, np.float64):
        steps, _ = K.case_reference(name, dtype)
        ora = O.LogLinearOracle(Bc, c['n'], p['Rw'], p['W'], p['b'], K.LAM, dtype=dtype)   # (step 0: the initial parameters)
        st = steps[0]
        f, dJ = st['f'], st['f']['dJ']
        db_true = st['grads'][2]
        assert U.rel_err(_db_from_dj(ora, f, dJ), db_true) < 1e-6          # the restated backward is the oracle's
        dt = ora.dtype
        lo, hi = O.clip_bounds(dt)
        g = (np.asarray(p['w'][:Bc], dtype=dt) / dt.type(Bc)).astype(dt)
        Q, Qc = f['Q'], f['Qc']
        dQ = -(g[:, None] * p['ydense'][:Bc].astype(dt)) / Qc * O._clip_mask(Q, lo, hi).astype(dt)
        y0 = p['y'][:Bc]
        dropped = dJ.copy()
        ndrop = 0
        for i in range(Bc):
            cols = y0.indices[y0.indptr[i]:y0.indptr[i + 1]][512:]
            dropped[i, cols] -= Q[i, cols] * dQ[i, cols]
            ndrop += len(cols)
        assert ndrop == sum(max(0, k - 512) for k in c['counts'])
        err = U.rel_err(_db_from_dj(ora, f, dropped), db_true)
        print('%s %s: %d entries dropped, db rel_err %.2e (10 GRAD_TOL = %.0e)' % (name, np.dtype(dtype).name, ndrop, err, 10 * GRAD_TOL))
        assert err > 10 * GRAD_TOL


class _SequentialWindowSum(O.LogLinearOracle):
    """The float32 oracle with J_e = sum_k log clip(P_ke) accumulated term by term in float32 -- n roundings at the
    magnitude of the sum -- where the oracle accumulates in float64 and rounds once (sert_oracle._sum)."""

    def forward(self, X, y):
        dt = self.dtype
        lo, hi = O.clip_bounds(dt)
        G, P3 = self.token_distributions(X)
        L = np.log(np.clip(P3, lo, hi)).astype(dt)
        J = np.zeros_like(L[:, 0, :])
        for k in range(L.shape[1]):
            J = (J + L[:, k, :]).astype(dt)
        Q = O.softmax_rows(J)
        Qc = np.clip(Q, lo, hi)
        loss = -O._sum(np.asarray(y).astype(dt) * np.log(Qc), axis=1, dtype=dt)
        return dict(G=G, P3=P3, J=J, Q=Q, Qc=Qc, loss=loss.astype(dt))


def test_a_window_summed_in_float32_would_be_visible_in_the_state():
    """`fusedrow` sums n = 65 log-probabilities of about -log 300 into J near -370, where a float32 ulp is 3e-5.  Summed
    term by term in float32 (what ll_fused_row did for every window before it took float64 for n > kLlTableWindow), every
    Q_e carries 1e-4 of relative error: db stays inside GRAD_TOL (5.7e-6), but Adadelta's squared-update moment of b is
    most sensitive exactly where a db entry is a cancelled remainder near sqrt(eps / (1 - rho)), and leaves TENSOR_TOL
    (3.5e-4 here, 4.8e-4 measured on the device).  The oracle's own sum -- float64, rounded once -- stays inside it against
    its float64 evaluation (3.7e-5), so check_state on this case is a check the engine can and must meet."""
    name = 'fusedrow'
    c, p = K.case_problem(name)
    Bc = len(c['counts'])
    _, o32 = K.case_reference(name, np.float32)
    _, o64 = K.case_reference(name, np.float64)
    seq = _SequentialWindowSum(Bc, c['n'], p['Rw'], p['W'], p['b'], K.LAM)
    for s in range(K.STEPS):
        sl = slice(s * Bc, (s + 1) * Bc)
        loss, grads, _ = seq.loss_and_grads(p['X'][sl], p['ydense'][sl], p['w'][sl])
        e = U.rel_err(grads[2], K.case_reference(name, np.float32)[0][s]['grads'][2])
        print('step %d: db of the sequential float32 sum against the oracle %.2e (GRAD_TOL %.0e)' % (s, e, GRAD_TOL))
        assert e < GRAD_TOL
        seq.opt.update(seq.params(), grads)
    ref32, ref64, got = U.oracle_state(o32), U.oracle_state(o64), U.oracle_state(seq)
    print('\n'.join(U.check_state(ref32, ref32, ref64)))                       # the oracle itself meets the state bounds
    e = U.rel_err(got['delta.b'], ref32['delta.b'])
    print('delta.b of the sequential float32 sum against the oracle %.2e (TENSOR_TOL %.0e)' % (e, U.TENSOR_TOL))
    assert e > 2 * U.TENSOR_TOL
    with pytest.raises(AssertionError, match='delta.b'):
        U.check_state(got, ref32, ref64)
