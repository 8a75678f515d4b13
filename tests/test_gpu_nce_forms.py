"""-m gpu: the NCE score / loss / gradient kernel of the vectorspace step in every template instance, training and evaluating
(tests/nce_cases.py), against the float64 oracle.  Which kernel every forward launched is asked of the engine
(Engine.nce_form, sert_debug_nce_form): a case that a moved dispatch threshold takes off its instance fails here by name
instead of passing for the wrong reason.  tests/test_nce_inputs_cpu.py proves the inputs: the cases cover the 24 instances,
the float32 oracle alone is within a quarter of every bound below, no clip mask is near any score or unit, and a reference
that drops the last chunk, the last candidate or the last row misses the bounds by a factor of 10 at least.

The bounds are the project's own: LOSS_TOL and ACT_TOL of tests/test_gpu_parity.py, U.ROW_TOL64 for the gradients."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import nce_cases as K
from tests import util as U

pytestmark = pytest.mark.gpu


def _check_form(name, eng, c, train, what):
    wg, partials = K.launch_shape(c, train)
    want = dict(c['form'], train=train, workgroups=wg, loss_partials=partials)
    got = eng.nce_form()
    assert got == want, (name, what, 'the forward launched', got, 'the case is there for', want)
    return got


def _check_rowloss(name, what, got, ref):
    err, row = K.rowloss_err(got, ref)
    assert err < K.ACT_TOL, (name, what, 'row loss', row, err, got[row], ref[row])
    return err


@pytest.mark.parametrize('name', list(K.CASES))
def test_nce_instance_against_float64(hip_lib, name):
    """keep_grads = 1.  Two training steps on one engine (the second reads the tables the engine updated itself), then the
    evaluation of a third batch.  Every step: the reported form is the stated instance, in its training or evaluating build,
    with ceil(B / 16) (scalar: ceil(B / 4)) workgroups and the matching count of loss partials; the step loss within LOSS_TOL and
    the row losses within ACT_TOL of the float64 oracle, row by row (w * loss in a training step; unweighted after eval_batch,
    which leaves them readable in T_ACT_ROWLOSS).  Training steps: da and dR_e -- the only place coef and cand show -- within
    U.ROW_TOL64 row by row; the row of weight 0 has a da and a row loss of exactly 0.  The evaluation leaves R_e and R_w bit for
    bit as they were.

    Measured on the MI355X, worst over a family's cases and their three steps (the bounds: loss 1e-5, row loss 2e-5, da and dR_e
    5e-5) -- regs: loss 2.5e-7, row loss 2.7e-7, da 8.8e-6 (regs2x6_de128_z1: with z = 1 the rows whose target is also their
    negative cancel; da of every case with z != 1 is at most 4.5e-7 off), dR_e 5.2e-7; per_candidate: 1.9e-7, 3.1e-7, 2.5e-6, 4.9e-7; scalar: 1.7e-7, 3.0e-7,
    1.4e-6, 4.4e-7.  All 24 instances were reported, each with train 1, 1, 0.  As a check of this test (not kept), a library with
    three planted faults -- `l < z` for `l <= z` in vs_nce_regs<3, ., 12>, the last chunk of the entity rows left out of the dot
    product in vs_nce<7>, the clamped rows of a ragged workgroup added to the loss partial in vs_nce<2> -- fails exactly the six
    cases of those three instances, each in training step 0, with loss errors of 8.6e-2 and 1.4e-1, 1.5e-4 and 3.1e-4, 1.3e-1
    and 3.0e-1, and passes the other 42."""
    c, p = K.case_problem(name)
    ref = K.case_reference(name, np.float64)
    B, z, de = c['B'], c['z'], c['de']
    eng = U.vs_engine(p, B, K.N, z, K.LAM, keep_grads=1)
    assert eng.nce_form() == dict(form='none', param=0, maxc=0, train=False, workgroups=0, loss_partials=0), (name, 'before the first forward')
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    zero = K.zero_weight_row(B)
    worst = dict(loss=0.0, rowloss=0.0, da=0.0, dRe=0.0)
    forms = []
    for s in range(K.TRAIN_STEPS):
        st, what = ref[s], 'training step %d' % s
        loss = eng.train_batch(s, p['neg'][s] if z else None)
        forms.append(_check_form(name, eng, c, True, what))
        e_loss = abs(float(loss) - float(st['loss'])) / abs(float(st['loss']))
        rl = eng.get_tensor(C.T_ACT_ROWLOSS, (B,)).copy()
        DA = eng.get_tensor(C.T_ACT_DA, (B, de)).copy()
        gRe = eng.get_tensor(C.T_GRAD_RE, (K.VE, de)).copy()
        e_da, r_da = U.row_err(DA, st['da'])
        e_re, r_re = U.row_err(gRe, st['dRe'])
        print('%s %s: loss %.6f (oracle %.6f) error %.1e; da worst row %.1e (row %d); dR_e worst row %.1e (entity %d)'
              % (name, what, loss, st['loss'], e_loss, e_da, r_da, e_re, r_re))
        assert e_loss <= K.LOSS_TOL, (name, what, 'loss', loss, st['loss'])
        e_rl = _check_rowloss(name, what, rl, st['rowloss'])
        assert e_da < U.ROW_TOL64, (name, what, 'da: row_err against the float64 oracle', e_da, 'row', r_da)
        assert e_re < U.ROW_TOL64, (name, what, 'dR_e: row_err against the float64 oracle', e_re, 'entity', r_re)
        assert not DA[zero].any() and rl[zero] == 0, (name, what, 'the row of weight 0', DA[zero][:4], rl[zero])
        for k, v in (('loss', e_loss), ('rowloss', e_rl), ('da', e_da), ('dRe', e_re)):
            worst[k] = max(worst[k], v)
    # evaluation: the TRAIN = false build of the same instance
    st, what = ref[K.TRAIN_STEPS], 'evaluation'
    Re, Rw = eng.get_tensor(C.T_RE).copy(), eng.get_tensor(C.T_RW).copy()
    loss = eng.eval_batch(C.SPLIT_TRAIN, K.TRAIN_STEPS, p['neg'][K.TRAIN_STEPS] if z else None)
    forms.append(_check_form(name, eng, c, False, what))
    e_loss = abs(float(loss) - float(st['loss'])) / abs(float(st['loss']))
    assert e_loss <= K.LOSS_TOL, (name, what, 'loss', loss, st['loss'])
    e_rl = _check_rowloss(name, what, eng.get_tensor(C.T_ACT_ROWLOSS, (B,)), st['rowloss'])
    assert U.same_bits(eng.get_tensor(C.T_RE), Re) and U.same_bits(eng.get_tensor(C.T_RW), Rw), (name, 'the evaluation changed a table')
    worst['loss'], worst['rowloss'] = max(worst['loss'], e_loss), max(worst['rowloss'], e_rl)
    eng.close()
    f = forms[0]
    print('%s: B %d z %d d_e %d -> %s<%d%s> train %s, worst errors: %s' % (
        name, B, z, de, f['form'], f['param'], ', %d' % f['maxc'] if f['maxc'] else '', [int(x['train']) for x in forms],
        ', '.join('%s %.1e' % kv for kv in worst.items())))
