"""Operand sizes at which a 32-bit byte offset wraps (tests/big_offset_cases.py; the inputs are proved in
tests/test_big_offset_inputs_cpu.py).

A. every GEMM kernel form just under the size guard that admits it (x3_shape_ok, gemm_x3.h: 2^29 elements; gemm_f32_vec,
   gemm.h: a leading dimension of 2^22) and the fp32 kernel that takes the shape at the guard, every element of the
   output against the float64 product under the bounds of test_gpu_gemm.py;
B. loglinear steps whose distinct-word logit table lies between 2^31 and 2^32 bytes (ll_row_wave: its 32-bit row offset
   has wrapped past 2^31) and beyond 2^32 (ll_row_from_table, the streaming kernels with the slot table, the logits GEMM's
   epilogue, the per-word sums, dW, dG), and a validation batch whose per-token logits pass 2^32 bytes.

The GPU work of a case is milliseconds; its wall time is the host's -- building, copying and comparing 2 to 4 GiB.  Every
case prints its route or loss form, its worst error against its bound, its wall time and the process's peak memory."""
import resource
import time

import numpy as np
import pytest

from tests import big_offset_cases as G
from tests import util as U
from tests.util import C

pytestmark = pytest.mark.gpu

LOSS_TOL, ACT_TOL, GRAD_TOL = 1e-5, 2e-5, 1e-4            # tests/test_gpu_parity.py
FORMS = {'plain': C.GEMM_FORM_PLAIN, 'splitk': C.GEMM_FORM_SPLITK, 'longk': C.GEMM_FORM_LONGK}
GEMM_CASES = [(name, side) for name in G.GEMM_ROWS for side in G.SIDES]


def _peak_gib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / float(1 << 20)


@pytest.mark.parametrize('name,side', GEMM_CASES, ids=['%s-%s' % c for c in GEMM_CASES])
def test_gemm_on_either_side_of_its_guard(hip_lib, monkeypatch, name, side):
    monkeypatch.delenv('SERT_GEMM_FP32', raising=False)
    t0 = time.perf_counter()
    row = G.GEMM_ROWS[name]
    M, N, K = row[side]
    # a threshold that moves must fail the case, not let it pass on another kernel
    route = C.debug_gemm_route(FORMS[row['hook']], M, N, K, tb=row['tb'], splits=row['splits'])
    assert route == row['routes'][G.SIDES.index(side)], (name, side, route)
    ops = G.gemm_operands(name)
    A, B = ops.stored(side)
    t1 = time.perf_counter()
    colsum = None
    if row['hook'] == 'plain':
        got = C.debug_gemm(A, B, tb=row['tb'])
    elif row['hook'] == 'splitk':
        got, colsum = C.debug_gemm_splitk(A, B, row['splits'])
    else:
        got = C.debug_gemm_longk(A, B, row['splits'], tb=row['tb'])
    del A, B
    t2 = time.perf_counter()
    finite = bool(np.all(np.isfinite(got))) and (colsum is None or bool(np.all(np.isfinite(colsum))))
    worst, worst_cs = ops.worst_error(side, got, colsum) if finite else (np.inf, np.inf)
    tol = G.bound(row, side)
    if side == G.SIDES[-1]:
        G.release_gemm_operands()
    print('\n%s %s %dx%dx%d tb=%d splits=%d: route %s, worst %.2e%s of %.2e; build %.1f s, hook %.1f s, compare %.1f s, peak %.1f GiB'
          % (name, side, M, N, K, row['tb'], row['splits'], route, worst,
             '' if worst_cs is None else ' (column sums %.2e)' % worst_cs, tol, t1 - t0, t2 - t1, time.perf_counter() - t2, _peak_gib()))
    assert finite                                        # (the hooks pre-fill the output with NaN: every element was written)
    assert worst < tol
    assert worst_cs is None or worst_cs < tol


def _rowloss_err(got, ref):
    """_check_rowloss of tests/test_gpu_parity.py."""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).mean())).max())


def _rowloss_tol(n):
    """ACT_TOL is the row-loss bound of tests/test_gpu_parity.py, whose loglinear windows have n <= 10.  A row's loss is
    lse(J) - J_y with J a float32 sum of n log-probabilities of one magnitude L = log V_e: the partial sums grow to n L, so
    each of the n additions rounds by up to ulp(n L) / 2 and the sum's error grows as n sqrt(n) ulp(L) -- relative to the
    loss (~ L) as n^1.5.  The bound keeps ACT_TOL up to n = 10 and follows that growth beyond (n = 64: sixteen times)."""
    return ACT_TOL * max(1.0, (n / 10.0) ** 1.5)


@pytest.mark.parametrize('name', list(G.LL_TRAIN))
def test_loglinear_step_whose_word_table_passes_a_mark(hip_lib, name):
    """One training step of the tiled problem, lambda = 0: loss, dW, db are the small problem's, dR_w[u] =
    (P / B) dR_small[u mod P n] row by row, the per-row losses of period P and the small problem's."""
    G.release_gemm_operands()
    t0 = time.perf_counter()
    case = G.LL_TRAIN[name]
    small, ref = G.ll_reference(name)
    r32, r64 = ref['float32'], ref['float64']
    big = G.ll_tiled(small, case['c'])
    B, n, P, c = big['B'], big['n'], small['P'], case['c']
    assert case['above'] <= B * n * case['Ve'] * 4 and (case['below'] is None or B * n * case['Ve'] * 4 < case['below'])
    eng = U.ll_engine(big, B, n, 0.0)
    try:
        eng.upload_dataset(C.SPLIT_TRAIN, big['X'], y_int=big['y'], w=big['w'])
        t1 = time.perf_counter()
        loss = eng.train_batch(0)
        t2 = time.perf_counter()
        f = eng.ll_loss_form()
        assert (f['form'], f['param']) == case['form'] and f['train'] and f['slots'], (name, f)
        rowloss = eng.get_tensor(C.T_ACT_ROWLOSS, (B,))
        dW, db = eng.get_tensor(C.T_GRAD_W), eng.get_tensor(C.T_GRAD_B)
        dRw = eng.get_tensor(C.T_GRAD_RW, (B * n, G.D))
    finally:
        eng.close()
    errs = dict(loss=abs(loss - r32['loss']) / abs(r32['loss']),
                period=float(np.abs(rowloss / np.tile(rowloss[:P], c) - 1).max()),
                rowloss=_rowloss_err(rowloss, np.tile(small['w'].astype(np.float64) * r64['rowloss'], c)),
                dW=U.rel_err(dW, r32['grads'][1].ravel()), db=U.rel_err(db, r32['grads'][2].ravel()))
    scale = P / float(B)
    want32 = np.tile(r32['grads'][0], (c, 1)) * np.float32(scale)
    want64 = np.tile(r64['grads'][0], (c, 1)) * scale
    errs['dR_w'] = U.rel_err(dRw, want32)
    print('\n%s B=%d n=%d V_e=%d table %.3e bytes: form %s; %s (bounds: loss and period %.0e, rowloss %.1e, gradients %.0e); '
          'build %.1f s, step %.1f s, compare %.1f s, peak %.1f GiB'
          % (name, B, n, case['Ve'], G.table_bytes(case), f, ', '.join('%s %.2e' % kv for kv in errs.items()), LOSS_TOL,
             _rowloss_tol(n), GRAD_TOL, t1 - t0, t2 - t1, time.perf_counter() - t2, _peak_gib()))
    assert np.isfinite(loss) and errs['loss'] <= LOSS_TOL
    # every row past the mark against its copies below it, then every row against the float64 oracle
    assert errs['period'] <= LOSS_TOL
    assert errs['rowloss'] < _rowloss_tol(n)
    assert errs['dW'] < GRAD_TOL and errs['db'] < GRAD_TOL and errs['dR_w'] < GRAD_TOL
    print(U.check_tensor('dR_w', dRw, want32, want64))


@pytest.mark.parametrize('name', list(G.LL_EVAL))
def test_validation_batch_whose_token_logits_pass_4_gib(hip_lib, name):
    """A validation split has no word index: one logit row per token, 1024 x 10 rows of 106 000 (106 001) floats.  The
    batch loss is the small problem's, and the row losses have period P -- the rows past the 2^32-byte mark (batch rows
    1013 and up) agree with their copies below it."""
    G.release_gemm_operands()
    t0 = time.perf_counter()
    case = G.LL_EVAL[name]
    small, ref = G.ll_reference(name)
    r32, r64 = ref['float32'], ref['float64']
    big = G.ll_tiled(small, case['c'], distinct=False)
    B, n, P, c = big['B'], big['n'], small['P'], case['c']
    assert B * n * case['Ve'] * 4 >= case['above']
    first_past = G.MARK32 // (case['Ve'] * 4) // n           # the batch row whose tokens straddle the mark
    assert P <= first_past < B - 1                           # (copies below the mark, whole rows past it)
    eng = U.ll_engine(big, B, n, 0.0)
    try:
        eng.upload_dataset(C.SPLIT_VALIDATE, big['X'], y_int=big['y'])
        t1 = time.perf_counter()
        ev = eng.eval_batch(C.SPLIT_VALIDATE, 0)
        t2 = time.perf_counter()
        f = eng.ll_loss_form()
        assert (f['form'], f['param']) == case['form'] and not f['train'] and not f['slots'], (name, f)
        rowloss = eng.get_tensor(C.T_ACT_ROWLOSS, (B,))
    finally:
        eng.close()
    err = abs(ev - r32['eval_loss']) / abs(r32['eval_loss'])
    period = float(np.abs(rowloss / np.tile(rowloss[:P], c) - 1).max())
    oracle = _rowloss_err(rowloss, np.tile(r64['rowloss'], c))
    print('\n%s B=%d n=%d V_e=%d logits %.3e bytes: form %s; loss %.2e, period %.2e (bound %.0e), rows against the oracle %.2e '
          '(bound %.0e); build %.1f s, evaluation %.1f s, compare %.1f s, peak %.1f GiB'
          % (name, B, n, case['Ve'], G.table_bytes(case), f, err, period, LOSS_TOL, oracle, _rowloss_tol(n), t1 - t0, t2 - t1,
             time.perf_counter() - t2, _peak_gib()))
    assert np.isfinite(ev) and err <= LOSS_TOL
    assert period <= LOSS_TOL
    assert oracle < _rowloss_tol(n)
