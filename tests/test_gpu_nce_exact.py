"""-m gpu: the exact-count instances of the NCE score / loss / gradient kernel, vs_nce_regs<NCH, TRAIN, 11> (z = 10), training
and evaluating, against the float64 oracle -- the companion of tests/test_gpu_nce_forms.py for tests/nce_exact_cases.py.  Which
kernel every forward launched is asked of the engine (Engine.nce_form): z = 10 must report MAXC = 11 at every width of the regs
form, z = 9 and z = 11 still MAXC = 12.  tests/test_nce_exact_inputs_cpu.py proves the inputs: the float32 oracle alone is within
a quarter of every bound below, no sigmoid mask is near a score, and a reference that drops candidate 10 or counts it twice
misses the bounds by a factor of 10 at least.

One case is saturated (two of every three columns of the projection scaled until units clip in every batch): da must be EXACTLY 0
on every unit whose t is beyond the clip bound, in the instance the default settings train with (d_e = 128, z = 10).

The bounds are those of tests/test_gpu_nce_forms.py, unchanged: K.LOSS_TOL, K.ACT_TOL, U.ROW_TOL64."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import nce_cases as K
from tests import nce_exact_cases as X
from tests import util as U

pytestmark = pytest.mark.gpu


def _check_form(name, eng, c, train, what):
    wg, partials = K.launch_shape(c, train)
    assert wg == -(-c['B'] // 16)
    want = dict(c['form'], train=train, workgroups=wg, loss_partials=partials)
    got = eng.nce_form()
    assert got == want, (name, what, 'the forward launched', got, 'the case is there for', want)
    return got


def _check_rowloss(name, what, got, ref):
    err, row = K.rowloss_err(got, ref)
    assert err < K.ACT_TOL, (name, what, 'row loss', row, err, got[row], ref[row])
    return err


@pytest.mark.parametrize('name', list(X.ALL))
def test_exact_count_instance_against_float64(hip_lib, name):
    """keep_grads = 1.  Two training steps on one engine, then the evaluation of a third batch (tests/test_gpu_nce_forms.py).
    Every step: the reported form is the stated instance (MAXC = 11 for z = 10, 12 for z = 9 and z = 11), in its training or
    evaluating build, with ceil(B / 16) workgroups and as many loss partials in training, none in evaluation; the step loss
    within LOSS_TOL, the row losses and t within ACT_TOL of the float64 oracle.  Training steps: da and dR_e within U.ROW_TOL64
    row by row; the row of weight 0 has a da and a row loss of exactly 0.  The saturated case: da is exactly 0 on every unit
    that is clipped for sure (|a| >= 10 on the oracle; the engine's t is +-1 there) and on every unit whose t, as the engine
    holds it, is beyond 1 - 2^-23; the units inside the clip answer to the row bound.

    Measured on the MI355X, worst over the eleven cases and their three steps (the bounds: loss 1e-5, row loss and t 2e-5, da and
    dR_e 5e-5): loss 1.5e-7, row loss 3.5e-7, t 1.2e-6 (the saturated case; 3.0e-7 elsewhere), da 2.9e-7, dR_e 2.4e-7.  The
    saturated case: 290 and 307 units clipped for sure in its two training steps, 488 and 521 beyond the bound in the engine's t,
    every one with da = 0."""
    c, p = X.case_problem(name)
    ref = X.case_reference(name, np.float64)
    B, z, de = c['B'], c['z'], c['de']
    eng = U.vs_engine(p, B, K.N, z, K.LAM, keep_grads=1)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    zero = K.zero_weight_row(B)
    worst = dict(loss=0.0, rowloss=0.0, t=0.0, da=0.0, dRe=0.0)
    forms = []
    for s in range(K.TRAIN_STEPS):
        st, what = ref[s], 'training step %d' % s
        loss = eng.train_batch(s, p['neg'][s])
        forms.append(_check_form(name, eng, c, True, what))
        e_loss = abs(float(loss) - float(st['loss'])) / abs(float(st['loss']))
        rl = eng.get_tensor(C.T_ACT_ROWLOSS, (B,)).copy()
        T = eng.get_tensor(C.T_ACT_T, (B, de)).copy()
        DA = eng.get_tensor(C.T_ACT_DA, (B, de)).copy()
        gRe = eng.get_tensor(C.T_GRAD_RE, (K.VE, de)).copy()
        e_t = U.rel_err(T, st['t'])
        e_da, r_da = U.row_err(DA, st['da'])
        e_re, r_re = U.row_err(gRe, st['dRe'])
        print('%s %s: loss %.6f (oracle %.6f) error %.1e; t %.1e; da worst row %.1e (row %d); dR_e worst row %.1e (entity %d)'
              % (name, what, loss, st['loss'], e_loss, e_t, e_da, r_da, e_re, r_re))
        assert e_loss <= K.LOSS_TOL, (name, what, 'loss', loss, st['loss'])
        e_rl = _check_rowloss(name, what, rl, st['rowloss'])
        assert e_t < K.ACT_TOL, (name, what, 't: rel_err against the float64 oracle', e_t)
        assert e_da < U.ROW_TOL64, (name, what, 'da: row_err against the float64 oracle', e_da, 'row', r_da)
        assert e_re < U.ROW_TOL64, (name, what, 'dR_e: row_err against the float64 oracle', e_re, 'entity', r_re)
        assert not DA[zero].any() and rl[zero] == 0, (name, what, 'the row of weight 0', DA[zero][:4], rl[zero])
        if c.get('saturated'):
            sure = X.surely_clipped(st)
            beyond = np.abs(T) > K.HI
            print('%s %s: %d units clipped for sure, %d beyond the bound in the engine\'s t' % (name, what, sure.sum(), beyond.sum()))
            assert sure.any() and np.all(np.abs(T[sure]) == 1), (name, what, 't of the units with |a| >= 10')
            assert np.all(beyond[sure]) and not DA[beyond].any(), (name, what, 'da of a clipped unit', np.abs(DA[beyond]).max())
            live = ~beyond
            live[zero] = False
            assert np.count_nonzero(DA[live]) > 0.99 * live.sum(), (name, what, 'units inside the clip without a gradient')
        else:
            assert np.all(np.abs(T) < K.HI)
        for k, v in (('loss', e_loss), ('rowloss', e_rl), ('t', e_t), ('da', e_da), ('dRe', e_re)):
            worst[k] = max(worst[k], v)
    # evaluation: the TRAIN = false build of the same instance
    st, what = ref[K.TRAIN_STEPS], 'evaluation'
    Re, Rw = eng.get_tensor(C.T_RE).copy(), eng.get_tensor(C.T_RW).copy()
    loss = eng.eval_batch(C.SPLIT_TRAIN, K.TRAIN_STEPS, p['neg'][K.TRAIN_STEPS])
    forms.append(_check_form(name, eng, c, False, what))
    e_loss = abs(float(loss) - float(st['loss'])) / abs(float(st['loss']))
    assert e_loss <= K.LOSS_TOL, (name, what, 'loss', loss, st['loss'])
    e_rl = _check_rowloss(name, what, eng.get_tensor(C.T_ACT_ROWLOSS, (B,)), st['rowloss'])
    e_t = U.rel_err(eng.get_tensor(C.T_ACT_T, (B, de)), st['t'])
    assert e_t < K.ACT_TOL, (name, what, 't', e_t)
    assert U.same_bits(eng.get_tensor(C.T_RE), Re) and U.same_bits(eng.get_tensor(C.T_RW), Rw), (name, 'the evaluation changed a table')
    worst['loss'], worst['rowloss'], worst['t'] = max(worst['loss'], e_loss), max(worst['rowloss'], e_rl), max(worst['t'], e_t)
    eng.close()
    f = forms[0]
    print('%s: B %d z %d d_e %d -> %s<%d, %d> train %s, worst errors: %s' % (
        name, B, z, de, f['form'], f['param'], f['maxc'], [int(x['train']) for x in forms],
        ', '.join('%s %.1e' % kv for kv in worst.items())))
