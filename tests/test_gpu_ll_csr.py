"""-m gpu: the loglinear step on CSR label rows at every loss kernel's label limits (tests/ll_csr_cases.py), against the
oracle at the tolerances of test_gpu_parity.py.  The kernel form every call took is asked of the engine
(Engine.ll_loss_form, sert_debug_ll_loss_form): a case that a moved threshold takes off its kernel fails here instead of
passing for the wrong reason.  tests/test_ll_csr_inputs_cpu.py proves the inputs: nothing near a clip bound, the float32
oracle a quarter tolerance from float64, and the missing label entries of a too-short fix-up list worth 40 GRAD_TOL."""
import types

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import ll_csr_cases as K
from tests import util as U
from tests.test_gpu_parity import GRAD_TOL, LOSS_TOL, PARAM_TOL, _check_rowloss

pytestmark = pytest.mark.gpu


def _form(eng):
    f = eng.ll_loss_form()
    return (f['form'], f['param']), f


@pytest.mark.parametrize('keep', [1, 0])
@pytest.mark.parametrize('name', list(K.CASES))
def test_loglinear_csr_label_rows(hip_lib, name, keep):
    """Measured on the MI355X: every case meets every bound with either keep_grads (worst over the cases: loss 8.1e-7, dW
    1.2e-6, db 1.9e-6, dR_w 2.3e-6, parameters 5.6e-6, all on `fusedrow`; the n = 3 cases 1e-7 ... 7e-7).  The entry with the
    least room is `fusedrow`'s delta.b in check_state: 4.5e-5 against the float32 oracle (TENSOR_TOL 1e-4), where the float32
    oracle is itself 3.7e-5 off its float64 evaluation -- J_e sums 65 log-probabilities to about -370, one fp32 ulp is 3e-5
    there, and Adadelta's squared-update moment of b multiplies what that leaves on Q (test_ll_csr_inputs_cpu.py prices
    it).  With J summed term by term in fp32, as ll_fused_row summed every window before, the same entry was 4.8e-4 and this
    case failed: windows longer than kLlTableWindow are now summed in float64, as the reference sums them."""
    c, p = K.case_problem(name)
    Bc, n = len(c['counts']), c['n']
    ref32, ora = K.case_reference(name, np.float32)
    eng = U.ll_engine(p, Bc, n, K.LAM, keep_grads=keep)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], csr=p['y'], w=p['w'])
    empty = np.asarray(c['counts']) == 0
    worst = dict(loss=0.0, dW=0.0, db=0.0, dRw=0.0)
    for s in range(K.STEPS):
        sl = slice(s * Bc, (s + 1) * Bc)
        st = ref32[s]
        loss = eng.train_batch(s)
        form, full = _form(eng)
        assert form == c['train'] and full['train'] and full['slots'], (name, 'training step', full, c['train'])
        assert full['segments'] == c.get('segments', 0), (name, full)
        e = abs(loss - st['loss']) / abs(st['loss'])
        worst['loss'] = max(worst['loss'], e)
        assert e <= LOSS_TOL, (name, s, loss, st['loss'])
        if not keep:
            continue
        _check_rowloss(eng, st['f'], p['w'][sl])
        rowloss = eng.get_tensor(C.T_ACT_ROWLOSS, (Bc,))
        assert np.all(rowloss[empty] == 0.0), (name, 'row loss of a row without labels', rowloss[empty])
        for key, tid, g in (('dW', C.T_GRAD_W, st['grads'][1]), ('db', C.T_GRAD_B, st['grads'][2]),
                            ('dRw', C.T_GRAD_RW, st['grads'][0])):
            e = U.rel_err(eng.get_tensor(tid), g.ravel())
            worst[key] = max(worst[key], e)
            print('%s keep=%d step %d %s rel_err %.2e' % (name, keep, s, key, e))
            assert e < GRAD_TOL, (name, s, key, e)
    for key, tid, ref in (('R_w', C.T_RW, ora.R_w), ('W', C.T_W, ora.W), ('b', C.T_B, ora.b)):
        e = U.rel_err(eng.get_tensor(tid), ref.ravel())
        worst[key] = e
        assert e < PARAM_TOL, (name, key, e)
    if not keep:
        _, o64 = K.case_reference(name, np.float64)
        print('\n'.join(U.check_state(U.engine_state(eng), U.oracle_state(ora), U.oracle_state(o64))))
    # evaluation after training, both against the oracle's eval_loss of the first batch: over the training split (the
    # distinct-word table through the per-token slots) and over the same rows as a validation split (no index: per token)
    ev_ref = ora.eval_loss(p['X'][:Bc], p['ydense'][:Bc])
    ev = eng.eval_batch(C.SPLIT_TRAIN, 0)
    form_t, full = _form(eng)
    assert form_t == c['ev_train'] and not full['train'] and full['slots'], (name, 'evaluation, training split', full)
    worst['eval_train'] = abs(ev - ev_ref) / abs(ev_ref)
    assert abs(ev - ev_ref) <= LOSS_TOL * abs(ev_ref), (name, ev, ev_ref)
    eng.upload_dataset(C.SPLIT_VALIDATE, p['X'][:Bc], csr=p['y'][:Bc])
    ev = eng.eval_batch(C.SPLIT_VALIDATE, 0)
    form_v, full = _form(eng)
    assert form_v == c['ev_valid'] and not full['train'] and not full['slots'], (name, 'evaluation, validation split', full)
    worst['eval_valid'] = abs(ev - ev_ref) / abs(ev_ref)
    assert abs(ev - ev_ref) <= LOSS_TOL * abs(ev_ref), (name, ev, ev_ref)
    eng.close()
    print('%s keep=%d forms: train %s eval(train split) %s eval(validation split) %s; worst %s'
          % (name, keep, c['train'], form_t, form_v, ' '.join('%s %.1e' % kv for kv in worst.items())))


def test_rows_do_not_depend_on_the_label_counts_of_other_rows(hip_lib):
    """The loss form goes by the longest row of the whole SPLIT.  The rows of table128_limit with at most four labels,
    trained once in a split of their own (a fused form) and once in a split whose LATER batch holds a 1025-label row (the
    streaming form): step 0 of both against the oracle, and the two forms as the engine reports them."""
    c, p = K.case_problem('table128_limit')
    n, Ve = c['n'], c['Ve']
    few = np.nonzero(p['counts'] <= 4)[0]
    assert len(few) >= 2
    Bs = len(few)
    X, w, y = p['X'][few], p['w'][few], p['y'][few]
    long_row = K.make_ll_csr_problem(7, (K.LABEL_LIMIT + 1,) + (1,) * (Bs - 1), n, K.VW, Ve, K.D, steps=1, zero_entry=False)
    import scipy.sparse as sp
    X2, w2, y2 = np.concatenate([X, long_row['X']]), np.concatenate([w, long_row['w']]), sp.vstack([y, long_row['y']]).tocsr()
    assert np.array_equal(np.diff(y2.indptr)[:Bs], p['counts'][few]) and np.diff(y2.indptr)[Bs] == K.LABEL_LIMIT + 1
    ora = O.LogLinearOracle(Bs, n, p['Rw'], p['W'], p['b'], K.LAM)
    loss_ref, (dRw, dW, db), f = ora.loss_and_grads(X, np.asarray(y.todense(), dtype=np.float32), w)
    forms = []
    for Xs, ws, ys in ((X, w, y), (X2, w2, y2)):
        eng = U.ll_engine(p, Bs, n, K.LAM, keep_grads=1)
        eng.upload_dataset(C.SPLIT_TRAIN, Xs, csr=ys, w=ws)
        loss = eng.train_batch(0)
        forms.append(_form(eng)[0])
        assert abs(loss - loss_ref) <= LOSS_TOL * abs(loss_ref), (forms[-1], loss, loss_ref)
        _check_rowloss(eng, f, w)
        assert U.rel_err(eng.get_tensor(C.T_GRAD_W), dW.ravel()) < GRAD_TOL, forms[-1]
        assert U.rel_err(eng.get_tensor(C.T_GRAD_B), db.ravel()) < GRAD_TOL, forms[-1]
        assert U.rel_err(eng.get_tensor(C.T_GRAD_RW), dRw.ravel()) < GRAD_TOL, forms[-1]
        eng.close()
    assert forms == [('table', 128), ('stream', 0)], forms


def test_upload_refuses_csr_rows_that_are_not_canonical(hip_lib):
    """include/sert_hip.h: the columns of a CSR row are strictly increasing.  A duplicate column and a descending pair are
    refused by sert_upload_dataset with the row named (two label entries of one column would be added to dJ by two threads
    without atomics); the canonical rows and an empty row upload.  The arrays go to the C ABI as they are: a plain
    namespace, not a scipy matrix (Engine.upload_dataset sorts what scipy knows to be unsorted)."""
    p = U.make_ll_problem(5, 8, 2, 10, 6, 4, 'int')
    eng = U.ll_engine(p, 4, 2, 0.0)
    indptr = np.array([0, 2, 2, 3, 5, 6, 7, 8, 9], dtype=np.int64)

    def csr(indices):
        return types.SimpleNamespace(indptr=indptr, indices=np.array(indices, dtype=np.int32),
                                     data=np.full(len(indices), 0.5, dtype=np.float32))

    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], csr=csr([1, 4, 0, 2, 5, 3, 3, 3, 3]), w=p['w'])     # canonical, row 1 empty
    with pytest.raises(C.SertError, match='row 3'):
        eng.upload_dataset(C.SPLIT_TRAIN, p['X'], csr=csr([1, 4, 0, 2, 2, 3, 3, 3, 3]), w=p['w'])  # duplicate column in row 3
    with pytest.raises(C.SertError, match='row 0'):
        eng.upload_dataset(C.SPLIT_TRAIN, p['X'], csr=csr([4, 1, 0, 2, 5, 3, 3, 3, 3]), w=p['w'])  # descending pair in row 0
    with pytest.raises(C.SertError, match='row 3'):
        eng.upload_dataset(C.SPLIT_VALIDATE, p['X'], csr=csr([1, 4, 0, 5, 2, 3, 3, 3, 3]))         # ... on the other split
    # a scipy matrix with unsorted (duplicate-free) rows is sorted on the way in
    import scipy.sparse as sp
    unsorted = sp.csr_matrix((np.full(9, 0.5, np.float32), np.array([4, 1, 0, 5, 2, 3, 3, 3, 3], np.int32), indptr), shape=(8, 6))
    assert not unsorted.has_sorted_indices
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], csr=unsorted, w=p['w'])
    assert np.isfinite(eng.train_batch(0))
    eng.close()
