"""-m gpu: a non-finite parameter that a loglinear batch reads makes that batch's loss non-finite, in every loss form
(tests/ll_nonfinite_cases.py; tests/test_ll_nonfinite_inputs_cpu.py proves the inputs and that a min/max clip would return a
finite loss for every plant).  The oracle is the reference for WHERE the non-finite values are -- loss, row losses, parameters
after the step -- and, in the rows and the control problem that stay finite, for their values.  The form every launch took is
asked of the engine, as in test_gpu_ll_csr.py."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import ll_nonfinite_cases as K
from tests import util as U
from tests.test_gpu_parity import ACT_TOL, LOSS_TOL, VARIANTS_BUILD

pytestmark = pytest.mark.gpu


def _engine(name, plant, keep):
    c, p = K.case_problem(name)
    Rw, W, b, info = K.planted(name, plant)
    eng = U.ll_engine(dict(Rw=Rw, W=W, b=b, X=p['X']), K.B, c['n'], K.LAM, keep_grads=keep)
    tr, va = slice(0, K.B * K.NB), slice(K.B * K.NB, K.N)
    if c.get('labels') == 'csr':
        eng.upload_dataset(C.SPLIT_TRAIN, p['X'][tr], csr=p['y'][tr], w=p['w'][tr])
        eng.upload_dataset(C.SPLIT_VALIDATE, p['X'][va], csr=p['y'][va])
    else:
        eng.upload_dataset(C.SPLIT_TRAIN, p['X'][tr], y_int=p['y'][tr], w=p['w'][tr])
        eng.upload_dataset(C.SPLIT_VALIDATE, p['X'][va], y_int=p['y'][va])
    return eng, info


def _same_loss(got, ref, what, bad):
    """non-finite where the oracle's is; where both are finite (the control), within 1e-5 of it -- absolute: the losses here
    are between 5 and 12, so this asks more than the suite's relative LOSS_TOL"""
    if np.isfinite(ref) and np.isfinite(got):
        print('%s: %.7f, oracle %.7f, apart %.1e (%.1e of it)' % (what, got, ref, abs(got - float(ref)), abs(got - float(ref)) / abs(float(ref))))
    if np.isfinite(ref) != np.isfinite(got):
        bad.append('%s: %r, the oracle has %r' % (what, got, ref))
    elif np.isfinite(ref) and not (abs(float(ref)) > 1.0 and abs(got - float(ref)) <= LOSS_TOL):
        bad.append('%s: %r is %.1e from the oracle\'s %r' % (what, got, abs(got - float(ref)) / abs(float(ref)), ref))


def _run_plant(name, plant, keep, bad, forms=None, check_forms=True):
    """One fresh engine: both evaluations at the initial parameters, then two training steps.  Findings go to `bad`."""
    c, p = K.case_problem(name)
    forms = forms or c['forms']
    ref = K.reference(name, plant, np.float32)
    eng, info = _engine(name, plant, keep)
    tag = '%s %s keep=%d' % (name, plant, keep)

    def form_is(key):
        if check_forms and eng.ll_loss_form() != forms[key]:
            bad.append('%s: %s took %r, expected %r' % (tag, key, eng.ll_loss_form(), forms[key]))

    # evaluation, before any step
    _same_loss(eng.eval_batch(C.SPLIT_TRAIN, 0), ref['ev_train'], tag + ' eval_batch(training split)', bad)
    form_is('ev_train')
    _same_loss(eng.eval_batch(C.SPLIT_VALIDATE, 0), ref['ev_valid'], tag + ' eval_batch(validation split)', bad)
    form_is('ev_valid')
    for s in range(K.NB):
        st = ref['steps'][s]
        _same_loss(eng.train_batch(s), st['loss'], tag + ' train_batch(%d)' % s, bad)
        form_is('train_keep%d' % keep)
        if keep:
            # w_i * loss_i: non-finite in exactly the oracle's rows, the others at the row-loss bound of test_gpu_ll_csr.py
            want = np.asarray(p['w'][s * K.B:(s + 1) * K.B], np.float64) * np.asarray(st['rowloss'], np.float64)
            got = eng.get_tensor(C.T_ACT_ROWLOSS, (K.B,))
            if not np.array_equal(np.isfinite(got), np.isfinite(want)):
                bad.append('%s step %d: row losses non-finite in rows %s, the oracle\'s in %s'
                           % (tag, s, np.nonzero(~np.isfinite(got))[0].tolist(), np.nonzero(~np.isfinite(want))[0].tolist()))
            ok = np.isfinite(want) & np.isfinite(got)
            if ok.any():
                err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-3 * np.abs(want[ok]).mean())
                if not err.max() < ACT_TOL:
                    bad.append('%s step %d: row loss %.2e from the oracle (ACT_TOL %.0e)' % (tag, s, err.max(), ACT_TOL))
        if plant == K.CONTROL:
            continue
        # the parameters after the step: W and b without a finite element, R_w non-finite in the oracle's rows
        Rw, W, b = st['params']
        got_Rw = eng.get_tensor(C.T_RW, Rw.shape)
        for key, got, want in (('W', eng.get_tensor(C.T_W, W.shape), W), ('b', eng.get_tensor(C.T_B, b.shape), b)):
            assert not np.isfinite(want).any()                   # (tests/test_ll_nonfinite_inputs_cpu.py)
            if np.isfinite(got).any():
                bad.append('%s after step %d: %d of %d elements of %s are finite, none of the oracle\'s'
                           % (tag, s, int(np.isfinite(got).sum()), got.size, key))
        rows_got = np.nonzero(~np.isfinite(got_Rw).all(axis=1))[0].tolist()
        rows_want = np.nonzero(~np.isfinite(Rw).all(axis=1))[0].tolist()
        if rows_got != rows_want:
            bad.append('%s after step %d: non-finite rows of R_w %s, the oracle\'s %s' % (tag, s, rows_got, rows_want))
    if plant == K.CONTROL:
        # finite throughout: the whole state against the oracle, b[e] = -inf apart
        e = info['entity']
        o64 = K.reference(name, plant, np.float64)['ora']
        got, r32, r64 = U.engine_state(eng), dict(U.oracle_state(ref['ora'])), dict(U.oracle_state(o64))
        assert r32['b'].shape == (1, c['Ve']) and r32['b'][0, e] == -np.inf and r64['b'][0, e] == -np.inf
        if got['b'][0, e] != -np.inf:
            bad.append('%s: b[%d] = %r after the steps, it must stay -inf (its gradient is 0)' % (tag, e, got['b'][0, e]))
        for state in (got, r32, r64):
            state['b'] = np.delete(state['b'], e, axis=1)
        try:
            print('\n'.join(U.check_state(got, r32, r64, prefix=tag + ' ')))
        except AssertionError as err:
            bad.append('%s state: %s' % (tag, err))
    eng.close()


@pytest.mark.parametrize('keep', [1, 0])
@pytest.mark.parametrize('name', list(K.CASES))
def test_loglinear_step_keeps_a_non_finite_value(hip_lib, name, keep):
    """Every plant of a case, each in a fresh engine; all findings of the case are reported together.
    Measured on the MI355X with the loss kernels' clips written as fminf(fmaxf(x, lo), hi): all twenty tests failed, every
    NaN / +Inf plant in every form.  Both evaluations returned finite losses (the figures the CPU test's min/max restatement
    gives: wave1 nan_word 5.589267 / 6.347976), the row losses were finite in every row, train_batch(0) returned a finite
    loss for the b and W plants (wave1: 6.784241), and R_w came out non-finite in the planted word's row only (the oracle's:
    every word of the batch row).  The training loss of the word plants and every second step were non-finite even so: the
    loss finalisation multiplies sum(p^2) by lambda / 2B = 0, and 0 x NaN carried it.  The control failed as well, at its
    second step: adadelta_elem added 0 x b[e] = 0 x -inf = NaN to the gradient of the unregularised bias.  With the select-form
    clips (common.h clip_prob / clip_logp) and no L2 term where l2k = 0, every test passes, each within 0.3 s; the control's
    losses are at most 6.2e-6 (absolute) from the oracle's."""
    bad = []
    for plant in K.PLANTS:
        _run_plant(name, plant, keep, bad)
    assert not bad, '\n'.join(bad)


if VARIANTS_BUILD:
    # the row-wise cross-check (ll_softmax_rows + ll_window) exists in a variants build only: so does this test id
    def test_rowwise_cross_check_keeps_a_non_finite_value(hip_lib):
        """SERT_LL_ROWWISE is read once per process, at the first loglinear forward: the case runs in a child process of its
        own with the knob set (this module's _rowwise_child)."""
        import os
        import subprocess
        import sys
        env = dict(os.environ, SERT_LL_ROWWISE='1')
        r = subprocess.run([sys.executable, '-c', 'from tests import test_gpu_ll_nonfinite as T; T._rowwise_child()'],
                           cwd=U.ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _rowwise_child():
    """`stream_scalar` with SERT_LL_ROWWISE=1: a split beyond the LDS slab goes to the row-wise kernels, per token (no
    distinct-word table), in training and in evaluation."""
    name = 'stream_scalar'
    row = dict(form='rowwise', param=0, segments=3)
    forms = dict(train_keep1=dict(row, train=True, slots=False), ev_train=dict(row, train=False, slots=False),
                 ev_valid=dict(row, train=False, slots=False))
    bad = []
    for plant in K.PLANTS:
        _run_plant(name, plant, 1, bad, forms=forms)
    assert not bad, '\n'.join(bad)


def test_language_model_stops_on_a_nan_word_row(hip_lib):
    """Through the Python surface, lambda = 0: a NaN in a word row that every batch reads.  train() raises from the epoch
    loop's non-finite check (models.py:372-379), and so do train_error() and validation_error() -- the error passes walk
    their split through the same check, as the vectorspace model's do (test_gpu_parity.py,
    test_model_with_empty_validation_and_short_data)."""
    from sert_amd import models
    B, n, Vw, Ve, d = 16, 3, 50, 40, 8
    p = U.make_ll_problem(44, B * 3, n, Vw, Ve, d, 'int')
    X = p['X'].copy()
    word = Vw - 1
    X[X == word] = 0
    X[::B, 1] = word                                   # one row of every batch
    Rw = p['Rw'].copy()
    Rw[word, 2] = np.nan
    m = models.LanguageModel(batch_size=B, window_size=n, representations_init=Rw, output_layer_size=Ve,
                             regularization_lambda=0.0, training_set=(X[:2 * B], p['y'][:2 * B], p['w'][:2 * B]),
                             validation_set=(X[2 * B:], p['y'][2 * B:]))
    with pytest.raises(RuntimeError, match='NaN or infinity'):
        m.train_error()
    with pytest.raises(RuntimeError, match='NaN or infinity'):
        m.validation_error()
    with pytest.raises(RuntimeError, match='NaN or infinity'):
        m.train()
