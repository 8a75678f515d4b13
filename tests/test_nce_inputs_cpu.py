"""No GPU: the problems of tests/nce_cases.py are what they claim, and the bounds of tests/test_gpu_nce_forms.py can tell a
wrong instance from a right one.

  1. Coverage: the stated forms are what the dispatch table gives for (d_e, z), they cover all 24 template instances between
     them (every case runs the training and the evaluating build), each instance at its smallest and its largest d_e, and z
     stands on both sides of every threshold.
  2. The oracle against itself: on every case and every step the float32 oracle is within a QUARTER of every bound of the GPU
     test of the float64 oracle -- the condition that makes those bounds meaningful.
  3. No mask is near: every sigmoid(u) lies strictly inside (1e-7, 1 - 2^-23), every |t| strictly inside the clip, by at least
     ten times the float32 oracle's own error of the scores -- the engine (another summation order) and the oracle cannot part
     over a mask.  A condition on the inputs: a seed that misses it is not used.
  4. The bounds have teeth: a reference with the last float4 chunk (scalar: the last 64-column slice) left out of the dot
     products and of da, one with the last candidate left out, and one with the last row of the batch left out of the loss
     each miss the row-loss or the da bound by at least a factor of 10."""
import numpy as np
import pytest

from tests import nce_cases as K
from tests import util as U

NAMES = list(K.CASES)


def test_cases_cover_every_instance():
    assert len(K.INSTANCES) == 24 == len(set(K.INSTANCES))
    by_instance = {}
    for name, c in K.CASES.items():
        assert c['form'] == K.dispatch(c['de'], c['z']), (name, c['form'], K.dispatch(c['de'], c['z']))
        assert c['B'] in K.BATCH_SIZES and 1 <= c['de'] <= 512
        by_instance.setdefault(K.instance_of(c), []).append(c)
    missing = [i for i in K.INSTANCES if i not in by_instance]
    assert not missing, 'template instances that no case of tests/nce_cases.py reaches: %s' % (missing,)
    assert set(by_instance) == set(K.INSTANCES)
    for (form, param, maxc), cs in by_instance.items():
        des = sorted(c['de'] for c in cs)
        scalar = form == 'scalar'
        # the smallest width of the instance: one lane alone in the last chunk / slice (d_e = 5 for NPL = 1: the smallest width
        # that is no multiple of 4 and not below it); the largest: every lane full (scalar: all but the last)
        lo = 64 * (param - 1) + ((5 if param == 1 else 1) if scalar else 4)
        hi = 64 * param - (1 if scalar else 0)
        assert des[0] == lo and des[-1] == hi, ((form, param, maxc), des, lo, hi)
        assert len({c['B'] for c in cs}) >= 2, ((form, param, maxc), 'one batch size only')
        small, large = min(cs, key=lambda c: c['de']), max(cs, key=lambda c: c['de'])
        assert K.last_slice_columns(small) == lo - 64 * (param - 1) and K.last_slice_columns(large) == (63 if scalar else 4)
    # z on both sides of every threshold of the dispatch, and 0, in each family that has the threshold
    regs = [c for c in K.CASES.values() if c['form']['form'] == 'regs']
    assert {0, 5} <= {c['z'] for c in regs if c['form']['maxc'] == 6} and {6, 11} <= {c['z'] for c in regs if c['form']['maxc'] == 12}
    low = [c for c in K.CASES.values() if c['form']['form'] == 'per_candidate' and c['form']['param'] <= 4]
    assert low and all(c['z'] + 1 >= 13 for c in low) and any(c['z'] == 12 for c in low)
    high = [c for c in K.CASES.values() if c['form']['form'] == 'per_candidate' and c['form']['param'] >= 5]
    assert {0, 5, 6, 11, 12} <= {c['z'] for c in high}
    assert {c['z'] for c in K.CASES.values() if c['form']['form'] == 'scalar'} == set(K.SCALAR_Z)
    # every form sees a batch below one workgroup, exactly one workgroup and a ragged last workgroup
    for form in ('regs', 'per_candidate', 'scalar'):
        assert {c['B'] for c in K.CASES.values() if c['form']['form'] == form} == set(K.BATCH_SIZES), form


@pytest.mark.parametrize('name', NAMES)
def test_plants(name):
    c, p = K.case_problem(name)
    B, z = c['B'], c['z']
    assert p['X'].shape == (K.BATCHES * B, K.N) and p['y'].shape == (K.BATCHES * B,) and p['Re'].shape == (K.VE, c['de'])
    zero, own = K.zero_weight_row(B), K.self_negative_row(B)
    assert len({0, zero, own, B - 1}) == 4
    for b in range(K.BATCHES):
        sl = K.batch_slice(c, b)
        y, w, neg = p['y'][sl], p['w'][sl], p['neg'][b]
        assert neg.shape == (B, z) and neg.dtype == np.int64 and (z == 0 or (neg.min() >= 0 and neg.max() < K.VE))
        assert y[0] == 0 and y[-1] == K.VE - 1
        assert z == 0 or y[own] in neg[own]
        if b < K.TRAIN_STEPS:
            assert w[zero] == 0 and np.count_nonzero(w == 0) == 1 and np.all(np.delete(w, zero) >= 0.5)
    assert not np.array_equal(p['neg'][0], p['neg'][1]) or z == 0


def _step_errors(name, s, got, ref):
    """The GPU test's measures of one step, each as a fraction of its bound: {measure: (error / bound, error)}."""
    out = {}
    out['loss'] = abs(float(got['loss']) - float(ref['loss'])) / abs(float(ref['loss']))
    out['rowloss'] = K.rowloss_err(got['rowloss'], ref['rowloss'])[0]
    bounds = dict(loss=K.LOSS_TOL, rowloss=K.ACT_TOL, da=U.ROW_TOL64, dRe=U.ROW_TOL64)
    if s < K.TRAIN_STEPS:
        out['da'] = U.row_err(got['da'], ref['da'])[0]
        out['dRe'] = U.row_err(got['dRe'], ref['dRe'])[0]
    return {k: (v / bounds[k], v) for k, v in out.items()}


@pytest.mark.parametrize('name', NAMES)
def test_reference_alone_meets_a_quarter_of_every_bound(name):
    r32, r64 = K.case_reference(name, np.float32), K.case_reference(name, np.float64)
    for s in range(K.BATCHES):
        e = _step_errors(name, s, r32[s], r64[s])
        print('%s step %d: float32 oracle against float64, error / bound: %s'
              % (name, s, ', '.join('%s %.3f (%.1e)' % ((k,) + v) for k, v in e.items())))
        for k, (frac, err) in e.items():
            assert frac < 0.25, (name, 'step', s, k, err)
        assert all(np.all(np.isfinite(a)) for a in r32[s].values() if isinstance(a, np.ndarray))
    # the zero-weight row is exactly zero in the reference too; every other row of da is not
    c, _ = K.case_problem(name)
    zero = K.zero_weight_row(c['B'])
    for s in range(K.TRAIN_STEPS):
        assert not r64[s]['da'][zero].any() and r64[s]['rowloss'][zero] == 0
        assert np.all(np.abs(np.delete(r64[s]['da'], zero, axis=0)).max(axis=1) > 0)


@pytest.mark.parametrize('name', NAMES)
def test_no_mask_is_near(name):
    r32, r64 = K.case_reference(name, np.float32), K.case_reference(name, np.float64)
    for s in range(K.BATCHES):
        sig, t = r32[s]['sig'], r32[s]['t']
        assert np.all((sig > K.LO) & (sig < K.HI)) and np.all(np.abs(t) < K.HI), (name, s)
        err, mu, mt = K.mask_margins(r32[s], r64[s])
        print('%s step %d: err %.1e, margin of the scores %.2f, of t %.1e' % (name, s, err, mu, mt))
        assert 0 < err < 1e-5 and mu >= 10 * err and mt >= 10 * err, (name, s, err, mu, mt)


@pytest.mark.parametrize('name', NAMES)
def test_bounds_have_teeth(name):
    c, p = K.case_problem(name)
    r64 = K.case_reference(name, np.float64)
    for s in range(K.TRAIN_STEPS):
        st = r64[s]
        w = p['w'][K.batch_slice(c, s)]
        # the restated contract is the oracle's
        rl, da = K.nce_rows(st['t'], st['Re'], st['cand'], w)
        assert K.rowloss_err(rl, st['rowloss'])[0] < 1e-9 and U.row_err(da, st['da'])[0] < 1e-9, name
        no_last_row = st['rowloss'].copy()
        no_last_row[-1] = 0
        wrong = {
            'last chunk dropped': K.nce_rows(st['t'], st['Re'], st['cand'], w, drop_columns=K.last_slice_columns(c)),
            'last candidate dropped': K.nce_rows(st['t'], st['Re'], st['cand'], w, drop_last_candidate=True),
            'last row not in the loss': (no_last_row, st['da']),
        }
        for what, (wrl, wda) in wrong.items():
            e_rl = K.rowloss_err(wrl, st['rowloss'])[0] / K.ACT_TOL
            e_da = U.row_err(wda, st['da'])[0] / U.ROW_TOL64
            print('%s step %d, %s: row loss misses its bound %.0f times, da %.0f times' % (name, s, what, e_rl, e_da))
            assert max(e_rl, e_da) >= 10, (name, s, what, e_rl, e_da)
