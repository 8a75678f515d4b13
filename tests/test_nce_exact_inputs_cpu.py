"""No GPU: the problems of tests/nce_exact_cases.py are what they claim, and the bounds of tests/test_gpu_nce_exact.py can tell a
wrong exact-count instance from a right one.  The companion of tests/test_nce_inputs_cpu.py.

  1. Coverage: the stated forms are what the dispatch table gives for (d_e, z); the cases reach vs_nce_regs<NCH, ., 11> for
     every NCH at its smallest and its largest d_e; z = 9 and z = 11 stay on MAXC = 12, and every case of tests/nce_cases.py
     keeps the instance it states; B covers less than a workgroup, exactly one, and ragged.
  2. The oracle against itself: on every case and every step the float32 oracle is within a QUARTER of every bound of the GPU
     test of the float64 oracle.
  3. No sigmoid mask is near any score (ten of the float32 oracle's own errors at least); no clip of t is near any unit -- but
     in the saturated case, where the clip is the point: there every batch has units that are clipped for sure (|a| >= 10),
     units that are live for sure, and the float64 oracle's da is exactly 0 on the former.
  4. The bounds have teeth: a reference with the eleventh candidate dropped and one with candidate 10 counted twice -- what a
     twelve-slot body without the mask of its idle slot would compute -- each miss the row-loss or the da bound by a factor of 10
     at least, in every z = 10 case."""
import numpy as np
import pytest

from tests import nce_cases as K
from tests import nce_exact_cases as X
from tests import util as U

NAMES = list(X.ALL)
EXACT = list(X.CASES) + list(X.SATURATED)


def test_cases_cover_every_exact_instance():
    by_instance = {}
    for name, c in X.ALL.items():
        assert c['form'] == X.dispatch(c['de'], c['z']), (name, c['form'], X.dispatch(c['de'], c['z']))
        assert c['B'] in K.BATCH_SIZES
        by_instance.setdefault(K.instance_of(c), []).append(c)
    assert set(X.INSTANCES) <= set(by_instance)
    for form, nch, maxc in X.INSTANCES:
        cs = [c for c in by_instance[(form, nch, maxc)] if not c.get('saturated')]
        assert all(c['z'] == 10 for c in cs)
        des = sorted(c['de'] for c in cs)
        assert des == [64 * (nch - 1) + 4, 64 * nch], ((form, nch, maxc), des)       # one lane alone in the last chunk | every lane full
        assert len({c['B'] for c in cs}) == 2
    assert {c['B'] for c in X.CASES.values()} == set(K.BATCH_SIZES)
    # on either side of the exact count, and everywhere else, the rule is the old one
    assert [c['z'] for c in X.NEIGHBOURS.values()] == [9, 11]
    assert all(c['de'] == 128 and c['form'] == dict(form='regs', param=2, maxc=12) for c in X.NEIGHBOURS.values())
    for de in (4, 128, 256, 260, 130):
        for z in range(0, 14):
            if z != 10:
                assert X.dispatch(de, z) == K.dispatch(de, z)
    assert all(X.dispatch(c['de'], c['z']) == c['form'] for c in K.CASES.values()), 'a case of tests/nce_cases.py moved'
    (s,) = X.SATURATED.values()
    assert (s['z'], s['de'], s['B']) == (10, 128, 37) and s['form'] == dict(form='regs', param=2, maxc=11)


@pytest.mark.parametrize('name', NAMES)
def test_plants(name):
    c, p = X.case_problem(name)
    B, z = c['B'], c['z']
    assert p['X'].shape == (K.BATCHES * B, K.N) and p['y'].shape == (K.BATCHES * B,) and p['Re'].shape == (K.VE, c['de'])
    assert p['Rw'].shape == (K.VW, K.DW)
    zero, own = K.zero_weight_row(B), K.self_negative_row(B)
    assert len({0, zero, own, B - 1}) == 4
    for b in range(K.BATCHES):
        sl = K.batch_slice(c, b)
        y, w, neg = p['y'][sl], p['w'][sl], p['neg'][b]
        assert neg.shape == (B, z) and neg.dtype == np.int64 and neg.min() >= 0 and neg.max() < K.VE
        assert y[0] == 0 and y[-1] == K.VE - 1
        assert y[own] in neg[own]
        if b < K.TRAIN_STEPS:
            assert w[zero] == 0 and np.count_nonzero(w == 0) == 1 and np.all(np.delete(w, zero) >= 0.5)
    assert not np.array_equal(p['neg'][0], p['neg'][1])


def _step_errors(s, got, ref):
    """The GPU test's measures of one step, each as a fraction of its bound: {measure: (error / bound, error)}."""
    out = {}
    out['loss'] = abs(float(got['loss']) - float(ref['loss'])) / abs(float(ref['loss']))
    out['rowloss'] = K.rowloss_err(got['rowloss'], ref['rowloss'])[0]
    out['t'] = U.rel_err(got['t'], ref['t'])
    bounds = dict(loss=K.LOSS_TOL, rowloss=K.ACT_TOL, t=K.ACT_TOL, da=U.ROW_TOL64, dRe=U.ROW_TOL64)
    if s < K.TRAIN_STEPS:
        out['da'] = U.row_err(got['da'], ref['da'])[0]
        out['dRe'] = U.row_err(got['dRe'], ref['dRe'])[0]
    return {k: (v / bounds[k], v) for k, v in out.items()}


@pytest.mark.parametrize('name', NAMES)
def test_reference_alone_meets_a_quarter_of_every_bound(name):
    r32, r64 = X.case_reference(name, np.float32), X.case_reference(name, np.float64)
    for s in range(K.BATCHES):
        e = _step_errors(s, r32[s], r64[s])
        print('%s step %d: float32 oracle against float64, error / bound: %s'
              % (name, s, ', '.join('%s %.3f (%.1e)' % ((k,) + v) for k, v in e.items())))
        for k, (frac, err) in e.items():
            assert frac < 0.25, (name, 'step', s, k, err)
        assert all(np.all(np.isfinite(a)) for a in r32[s].values() if isinstance(a, np.ndarray))
    c, _ = X.case_problem(name)
    zero = K.zero_weight_row(c['B'])
    for s in range(K.TRAIN_STEPS):
        assert not r64[s]['da'][zero].any() and r64[s]['rowloss'][zero] == 0
        assert np.all(np.abs(np.delete(r64[s]['da'], zero, axis=0)).max(axis=1) > 0)


@pytest.mark.parametrize('name', NAMES)
def test_no_mask_is_near(name):
    c, _ = X.case_problem(name)
    r32, r64 = X.case_reference(name, np.float32), X.case_reference(name, np.float64)
    for s in range(K.BATCHES):
        sig, t = r32[s]['sig'], r32[s]['t']
        assert np.all((sig > K.LO) & (sig < K.HI)), (name, s)
        err, mu, mt = K.mask_margins(r32[s], r64[s])
        print('%s step %d: err %.1e, margin of the scores %.2f, of t %.1e' % (name, s, err, mu, mt))
        assert 0 < err < 1e-5 and mu >= 10 * err, (name, s, err, mu)
        if not c.get('saturated'):
            assert np.all(np.abs(t) < K.HI) and mt >= 10 * err, (name, s, err, mt)


@pytest.mark.parametrize('name', list(X.SATURATED))
def test_saturated_case_clips_in_every_batch(name):
    """Every batch: units that are clipped whoever computes tanh (|a| >= 10: t is +-1 in float32), in rows that carry a
    gradient; both oracles mask them (da exactly 0, t beyond their clip bound); and units that are live for sure (|a| <= 5)
    with a non-zero da, so that `da == 0 on the clipped units` cannot be met by a kernel that zeroes everything."""
    c, p = X.case_problem(name)
    r32, r64 = X.case_reference(name, np.float32), X.case_reference(name, np.float64)
    zero = K.zero_weight_row(c['B'])
    for s in range(K.BATCHES):
        sure = X.surely_clipped(r64[s])
        assert np.array_equal(sure, np.abs(r32[s]['a']) >= X.SURE_A), (name, s, 'the two oracles part over |a| >= 10')
        assert np.all(np.abs(r32[s]['t'][sure]) == 1) and np.all(np.abs(r32[s]['t'][sure]) > K.HI)
        live_rows = np.delete(np.arange(c['B']), zero) if s < K.TRAIN_STEPS else np.arange(c['B'])
        n_sure = int(sure[live_rows].sum())
        print('%s step %d: %d of %d units clipped for sure (sW = %g), in %d rows' % (
            name, s, n_sure, sure[live_rows].size, p['sW'], int(sure[live_rows].any(axis=1).sum())))
        assert n_sure >= 1, (name, s, 'no unit clips')
        # both halves of a row's lanes and both chunks of a lane hold clipped units somewhere in the batch
        cols = np.nonzero(sure[live_rows].any(axis=0))[0]
        assert cols.min() < 64 <= cols.max(), (name, s, cols)
        if s < K.TRAIN_STEPS:
            assert not r64[s]['da'][sure].any() and not r32[s]['da'][sure].any()
            live = (np.abs(r64[s]['a']) <= 5.0)[live_rows]
            assert live.any() and np.all(r64[s]['da'][live_rows][live] != 0)


@pytest.mark.parametrize('name', EXACT)
def test_bounds_have_teeth(name):
    c, p = X.case_problem(name)
    r64 = X.case_reference(name, np.float64)
    for s in range(K.TRAIN_STEPS):
        st = r64[s]
        w = p['w'][K.batch_slice(c, s)]
        if c.get('saturated'):
            # (nce_rows restates the contract for units inside the clip: compared there, the rest is set to 0 on both sides)
            inside = np.abs(st['t']) <= np.float64(K.HI)
        else:
            inside = np.ones(st['t'].shape, bool)
        ref_da = np.where(inside, st['da'], 0.0)
        rl, da = K.nce_rows(st['t'], st['Re'], st['cand'], w)
        if not c.get('saturated'):      # (the float64 oracle's own clip bound is 1 - 1e-7: p differs from nce_rows' by 2e-8 there)
            assert K.rowloss_err(rl, st['rowloss'])[0] < 1e-9 and U.row_err(da, st['da'])[0] < 1e-9, name
        else:
            assert K.rowloss_err(rl, st['rowloss'])[0] < 1e-6 and U.row_err(np.where(inside, da, 0.0), ref_da)[0] < 1e-6, name
        wrong = {
            'candidate 10 dropped': K.nce_rows(st['t'], st['Re'], st['cand'], w, drop_last_candidate=True),
            'candidate 10 counted twice': K.nce_rows(st['t'], st['Re'], X.last_candidate_twice(st['cand']), w),
        }
        for what, (wrl, wda) in wrong.items():
            e_rl = K.rowloss_err(wrl, st['rowloss'])[0] / K.ACT_TOL
            e_da = U.row_err(np.where(inside, wda, 0.0), ref_da)[0] / U.ROW_TOL64
            print('%s step %d, %s: row loss misses its bound %.0f times, da %.0f times' % (name, s, what, e_rl, e_da))
            assert e_rl >= 10 and e_da >= 10, (name, s, what, e_rl, e_da)
