"""-m gpu: dR_w, the word-table gradient, at every occurrence count and tree shape of tests/wgrad_cases.py -- the vectorspace
tree with its dense heavy words (word_grad_segsum) and the loglinear per-distinct-word sums (dzu_from_dj) -- row by row against
the float64 oracle.  What every step launched is asked of the engine (Engine.wgrad_plan, sert_debug_wgrad_plan): a case that a
moved dispatch threshold takes off its kernels fails here instead of passing for the wrong reason.
tests/test_wgrad_inputs_cpu.py proves the inputs: the tokens are the stated counts, the index and the dispatch give the stated
plans, the cases produce every event of K.EVENTS between them, the float32 oracle alone is within U.ROW_TOL64 of the float64 one
and no touched row is small enough for the floor of U.row_err to hide it."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import util as U
from tests import wgrad_cases as K

pytestmark = pytest.mark.gpu


def _engine(name, keep, monkeypatch, knob):
    """An engine of the case with its dataset uploaded; knob: SERT_DENSE_HEAVY (read at upload), None = unset."""
    c, p = K.case_problem(name)
    if knob is None:
        monkeypatch.delenv('SERT_DENSE_HEAVY', raising=False)
    else:
        monkeypatch.setenv('SERT_DENSE_HEAVY', knob)
    if K.is_ll(name):
        eng = U.ll_engine(p, c['B'], c['n'], K.LAM, keep_grads=keep)
    else:
        eng = U.vs_engine(p, c['B'], c['n'], K.VS_Z, K.LAM, keep_grads=keep)
    assert eng.wgrad_plan() == {'path': 'none'}, (name, 'before the first backward')
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    return eng


def _train(eng, name, step):
    _, p = K.case_problem(name)
    if K.is_ll(name):
        eng.train_batch(step)
    else:
        eng.train_batch(step, p['neg'][step])
    return eng.wgrad_plan()


def _check_plan(name, step, got, want):
    assert got == want, (name, 'step', step, 'the backward launched', got, 'the case is there for', want)


def _gradient_steps(name, monkeypatch, knob, plans, tag=''):
    """Both steps of a case on a fresh engine with keep_grads = 1: [dR_w (V_w, d) of step 0, of step 1], each checked row by row
    over the touched rows against the float64 oracle; the plan of each step asserted.  Returns (gradients, worst row error)."""
    c, p = K.case_problem(name)
    g32, _ = K.case_reference(name, np.float32)
    g64, _ = K.case_reference(name, np.float64)
    Vw, d = p['Rw'].shape
    l2k = np.float32(K.LAM) / np.float32(c['B'])       # csrc/host/optimizer_and_loss.inc: lambda / B, in float
    eng = _engine(name, 1, monkeypatch, knob)
    out, worst = [], 0.0
    for s in range(K.STEPS):
        Rw = eng.get_tensor(C.T_RW, (Vw, d)).copy()     # the table this step reads (step 1: after the engine's own update)
        plan = _train(eng, name, s)
        _check_plan(name, s, plan, plans[s])
        got = eng.get_tensor(C.T_GRAD_RW, (Vw, d)).copy()
        counts = K.step_counts(name, s)
        touched = np.nonzero(counts > 0)[0]
        err, row = U.row_err(got, K.word_grad(name, g64[s]), rows=touched)
        worst = max(worst, err)
        print('%s step %d%s: plan %s; dR_w worst row error against float64 %.2e (word %d, %d occurrences)'
              % (name, s, tag, plan, err, row, counts[row]))
        assert err < U.ROW_TOL64, (name, 'step', s, 'row_err against the float64 oracle', err, 'word', row, 'occurrences', int(counts[row]))
        # An absent word's row is EXACTLY zero.  T_GRAD_RW is read behind the optimiser, which adds the L2 term (lambda / B) R_w
        # to the stored gradient in float with contraction off (kernels_opt.h: adam_elem / adadelta_elem, g = g + l2k * p), so a
        # row the batch does not touch holds exactly fl(l2k * R_w) -- 0.0 + x = x -- and anything left of an earlier step's
        # rows, or of another word's partial rows, shows as a difference in the last bit.
        absent = np.nonzero(counts == 0)[0]
        data = got[absent] - l2k * Rw[absent]
        bad = np.nonzero(np.any(data != 0.0, axis=1))[0]
        assert len(bad) == 0, (name, 'step', s, 'rows of absent words that are not exactly zero', absent[bad][:10], data[bad][:3])
        if K.is_ll(name):
            Ve = c['Ve']
            for tname, tid, shape, k in (('dW', C.T_GRAD_W, (d, Ve), 1), ('db', C.T_GRAD_B, (1, Ve), 2)):
                line = U.check_tensor(tname, eng.get_tensor(tid, shape), np.asarray(g32[s][k]).reshape(shape),
                                      np.asarray(g64[s][k]).reshape(shape))
                print('%s step %d: %s' % (name, s, line))
        out.append(got)
    eng.close()
    return out, worst


@pytest.mark.parametrize('name', list(K.CASES))
def test_word_gradient_row_by_row(hip_lib, monkeypatch, name):
    """keep_grads = 1.  Two steps with different plans on one engine, each dR_w within U.ROW_TOL64 of the float64 oracle row by
    row over the touched rows -- the message names the word and its count -- and exactly fl(l2k R_w) where the word is absent,
    the plan of each step as the case states it; a second engine bit for bit; the cases with dense words also under
    SERT_DENSE_HEAVY=0, the two results within 2 ROW_TOL64 of each other row by row (each is within ROW_TOL64 of float64) and
    the dense words' rows different in bits (the pass ran); loglinear: dW and db through U.check_tensor.

    Measured on the MI355X, worst touched row against float64 over both steps (the bound is 5e-5): lens_d128 4.3e-7, lens_d256
    4.8e-7, lens_d256_dense 4.6e-7, w_d200 5.0e-7, w_d200_dense 3.0e-7, w_d260 3.0e-7, w_d300 4.3e-7, w_d388 3.0e-7, w_d516 3.5e-7,
    w_d6 3.9e-7, w_d70 7.4e-7, four_levels_d132 4.9e-7 (the float32 oracle alone: 2.1e-5), upper_bounds_d8 4.8e-7, rows128_d4
    4.0e-7, rows256_d8 7.3e-7, eighth_d4 1.3e-6, ll_v24 5.0e-7, ll_v260 1.3e-6, ll_v23 1.1e-6, ll_v75 1.3e-6; the dense pass
    against the plain tree at most 1.7e-7 apart (the word of 5000 occurrences of rows128_d4); loglinear dW and db at most 1.4e-6
    row by row against float64.  As a check of this test (not kept): with the 1-3 entry tail of segsum_rows_body leaving out
    its last entry (the loads unchanged) the sixteen cases that run that body fail -- lens_d128, lens_d256, lens_d256_dense,
    w_d200 ... w_d516, four_levels_d132, upper_bounds_d8, rows256_d8, ll_v24, ll_v260 in step 0 with a row error of 1.0 on a word of
    1 occurrence (lens_d128: word 1790), rows128_d4 in step 1 with 0.57 on word 166 of 3 occurrences, eighth_d4 in step 0 with
    0.90 on word 324 of 50 occurrences -- and the four that run segsum_rows_scalar (w_d6, w_d70, ll_v23, ll_v75) pass."""
    c, _ = K.case_problem(name)
    first, worst = _gradient_steps(name, monkeypatch, c.get('knob'), c['plan'])
    again, _ = _gradient_steps(name, monkeypatch, c.get('knob'), c['plan'])
    for s in range(K.STEPS):
        assert U.same_bits(first[s], again[s]), (name, 'step', s, 'a second engine differs', U.row_err(again[s], first[s]))
    if name in K.dense_cases():
        tree_only = dict(c, knob='0')
        plans = [K.plan_from_dispatch(tree_only, K.step_counts(name, s)) for s in range(K.STEPS)]
        assert all(pl['dense_cnt'] == 0 and pl['heavy'] == 'none' for pl in plans), plans
        plain, _ = _gradient_steps(name, monkeypatch, '0', plans, tag=' SERT_DENSE_HEAVY=0')
        for s in range(K.STEPS):
            counts = K.step_counts(name, s)
            touched = np.nonzero(counts > 0)[0]
            err, row = U.row_err(first[s], plain[s], rows=touched)
            print('%s step %d: dense pass against the plain tree, worst row %.2e (word %d, %d occurrences)' % (name, s, err, row, counts[row]))
            assert err < 2 * U.ROW_TOL64, (name, 'step', s, 'dense pass against the plain tree', err, 'word', row, int(counts[row]))
            dense = K.dense_words(counts, c['B'] * c['n'], K.dense_enabled(c))
            assert len(dense) == c['plan'][s]['dense_cnt']
            same = [w for w in dense if U.same_bits(first[s][w], plain[s][w])]
            assert not same, (name, 'step', s, 'dense words whose rows have the plain tree\'s bits: the dense pass did not run', same)
    print('%s: worst row error over both steps %.2e' % (name, worst))


@pytest.mark.parametrize('name', list(K.CASES))
def test_tables_after_the_product_steps(hip_lib, monkeypatch, name):
    """keep_grads = 0, the product path: the gradient table is not zeroed, the rows a batch touches are flagged by the batch's
    bits and the word table is updated lazily.  Nothing is read between the two steps (the plan hook touches no device); then
    every parameter and both of its moments against the float32 and the float64 oracle's train_step, globally and row by row."""
    c, _ = K.case_problem(name)
    _, o32 = K.case_reference(name, np.float32)
    _, o64 = K.case_reference(name, np.float64)
    eng = _engine(name, 0, monkeypatch, c.get('knob'))
    for s in range(K.STEPS):
        _check_plan(name, s, _train(eng, name, s), c['plan'][s])
    log = U.check_state(U.engine_state(eng), U.oracle_state(o32), U.oracle_state(o64))
    eng.close()
    print('%s keep_grads=0: %s' % (name, '; '.join(log)))
