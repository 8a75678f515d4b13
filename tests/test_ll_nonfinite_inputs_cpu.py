"""No GPU: the problems of tests/ll_nonfinite_cases.py are checkable.  On the oracle alone, for every case: the clean problem is
tame (float32 and float64 losses agree to half the loss tolerance, no probability within a factor two of a clip bound); every
NaN / +Inf plant makes the oracle's loss non-finite, training and evaluation, float32 and float64, in exactly the rows that
read the planted value; the -Inf bias is finite throughout; and a restatement of the forward whose clips are
fmin(fmax(x, lo), hi) and whose max is fmax -- what a kernel computes that clips with fminf / fmaxf -- returns a FINITE loss
for every one of those plants, so each input tells the two behaviours apart."""
import numpy as np
import pytest

from oracle import sert_oracle as O
from tests import ll_nonfinite_cases as K

NAMES = list(K.CASES)
POISON = tuple(K.WORD_PLANTS) + K.DENSE_PLANTS
HALF_LOSS_TOL = 0.5e-5


def _labels(p, sl):
    """sets of label entities of the rows of a slice"""
    y = p['y']
    if isinstance(y, np.ndarray):
        return [{int(e)} for e in y[sl]]
    rows = y[sl]
    return [set(rows.indices[rows.indptr[r]:rows.indptr[r + 1]].tolist()) for r in range(rows.shape[0])]


@pytest.mark.parametrize('name', NAMES)
def test_case_is_built_as_stated(name):
    c, p = K.case_problem(name)
    n, X = c['n'], p['X']
    assert X.shape == (K.N, n) and K.NB == 2 and K.NV == 1
    batch0, batch1, valid = X[:K.B], X[K.B:2 * K.B], X[2 * K.B:]
    positions = set()
    for which, word in K.PLANT_WORDS.items():
        pos = K.position(which, n)
        assert 0 <= pos < n
        positions.add(pos)
        # once in batch 0 and once in the validation batch, at the stated row and position; never in batch 1
        assert (batch0 == word).sum() == 1 and batch0[K.TRAIN_ROW[which], pos] == word
        assert (valid == word).sum() == 1 and valid[K.VALID_ROW[which], pos] == word
        assert (batch1 == word).sum() == 0
    assert len(set(K.TRAIN_ROW.values())) == 3 and len(set(K.VALID_ROW.values())) == 3
    if n == 7:      # every trip of the row loops: three window rows in flight (ll_row_wave), five (ll_row_from_table)
        assert {q // 3 for q in positions} == {0, 1, 2} and {q // 5 for q in positions} == {0, 1}
    labels = _labels(p, slice(0, K.N))
    assert all(len(s) >= 1 for s in labels)                     # no empty CSR row: its device loss is 0 by construction
    assert all(p['free'] not in s for s in labels) and 0 <= p['free'] < c['Ve']
    counts = [len(s) for s in labels]
    if c.get('labels') == 'csr':
        long_rows = [r for r, k in enumerate(counts) if k > 1024]
        assert long_rows == [0, K.B * K.NB] and counts[0] == K.LONG_ROW_LABELS       # one per split: both splits stream
        y = p['y']
        assert all(np.all(np.diff(y.indices[y.indptr[r]:y.indptr[r + 1]]) > 0) for r in range(K.N))
        assert np.allclose(np.asarray(y.sum(axis=1)).ravel(), 1.0, atol=1e-5) and y.data.min() > 0
    else:
        assert counts == [1] * K.N
    # the forms recorded follow ll_forward's thresholds
    fused = (n + 1) * c['Ve'] * 4 <= 150 * 1024 and max(counts) <= 1024
    f = c['forms']
    assert f['train_keep0'] == f['train_keep1'] and f['train_keep0']['train'] and f['train_keep0']['slots']
    assert not f['ev_train']['train'] and f['ev_train']['slots'] and not f['ev_valid']['train'] and not f['ev_valid']['slots']
    if fused:
        Ve = c['Ve']
        if n > 64:
            want = ('fused_row', 512)
        elif Ve % 4 == 0 and Ve <= 2048:
            e4 = -(-(Ve // 4) // 64)
            want = ('wave', 1 if e4 <= 1 else 2 if e4 <= 2 else 4 if e4 <= 4 else 8)
        else:
            want = ('table', 128 if Ve <= 2048 else 512)
        assert (f['train_keep0']['form'], f['train_keep0']['param']) == want
        assert all((f[k]['form'], f[k]['param'], f[k]['segments']) == ('fused_row', 512, 0) for k in ('ev_train', 'ev_valid'))
        assert f['train_keep0']['segments'] == 0
    else:
        want = ('stream', 1 if c['Ve'] % 4 == 0 else 0, -(-c['Ve'] // 4096))
        assert all((v['form'], v['param'], v['segments']) == want for v in f.values())


@pytest.mark.parametrize('name', NAMES)
def test_clean_problem_is_tame(name):
    c, p = K.case_problem(name)
    r32, r64 = K.reference(name, None, np.float32), K.reference(name, None, np.float64)
    pairs = [('eval train', r32['ev_train'], r64['ev_train']), ('eval valid', r32['ev_valid'], r64['ev_valid'])]
    pairs += [('step %d' % s, a['loss'], b['loss']) for s, (a, b) in enumerate(zip(r32['steps'], r64['steps']))]
    for what, a, b in pairs:
        e = abs(float(a) - float(b)) / abs(float(b))
        print('%s %s: float32 %.7f float64 %.7f rel %.1e' % (name, what, a, b, e))
        assert np.isfinite(a) and np.isfinite(b) and e <= HALF_LOSS_TOL
    # clip margin, as tests/op_sequence_cases.py measures it: every probability the loss clips, as a factor from a bound
    for dtype, ref in ((np.float32, r32), (np.float64, r64)):
        lo, hi = O.clip_bounds(np.float64)
        fs = [st['f'] for st in ref['steps']]
        ora = O.LogLinearOracle(K.B, c['n'], p['Rw'], p['W'], p['b'], K.LAM, dtype=dtype)
        fs += [ora.forward(*K.split(p, which)[:2]) for which in ('train', 'valid')]
        margin = min(min(float(a.min() / lo), float((1.0 - a.max()) / (1.0 - hi))) for f in fs for a in (f['P3'], f['Q']))
        print('%s %s: clip margin %.3g' % (name, np.dtype(dtype).name, margin))
        assert margin > 2.0


@pytest.mark.parametrize('name', NAMES)
def test_every_plant_makes_the_oracle_loss_non_finite_in_the_expected_rows(name):
    c, p = K.case_problem(name)
    for plant in POISON:
        info = K.planted(name, plant)[3]
        for dtype in (np.float32, np.float64):
            ref = K.reference(name, plant, dtype)
            what = (name, plant, np.dtype(dtype).name)
            assert not np.isfinite(ref['steps'][0]['loss']), what
            assert not np.isfinite(ref['steps'][1]['loss']), what         # W and b are all NaN by then
            assert not np.isfinite(ref['ev_train']) and not np.isfinite(ref['ev_valid']), what
            assert np.nonzero(~np.isfinite(ref['steps'][0]['rowloss']))[0].tolist() == info['train_rows'], what
            assert np.nonzero(~np.isfinite(ref['ev_train_rows']))[0].tolist() == info['train_rows'], what
            assert np.nonzero(~np.isfinite(ref['ev_valid_rows']))[0].tolist() == info['valid_rows'], what
            # after one step: dW = G^T dZ and db sum over the NaN row(s) -- no finite element is left in W or b
            Rw1, W1, b1 = ref['steps'][0]['params']
            assert not np.isfinite(W1).any() and not np.isfinite(b1).any(), what
            bad = set(np.nonzero(~np.isfinite(Rw1).all(axis=1))[0].tolist())
            words = set(p['X'][:K.B][info['train_rows']].ravel().tolist())
            if plant in K.WORD_PLANTS:
                words.add(K.PLANT_WORDS[K.WORD_PLANTS[plant][0]])
            assert bad == words, what


@pytest.mark.parametrize('name', NAMES)
def test_the_control_is_finite_and_differs_from_the_clean_problem(name):
    # "differs": by more than 2e-6 of the loss, some twenty float32 ulps -- the entity leaves every token's softmax, which
    # moves the loss by about n / V_e
    c, p = K.case_problem(name)
    e = K.planted(name, K.CONTROL)[3]['entity']
    for dtype in (np.float32, np.float64):
        ref, clean = K.reference(name, K.CONTROL, dtype), K.reference(name, None, dtype)
        for key in ('ev_train', 'ev_valid'):
            assert np.isfinite(ref[key]) and np.isfinite(ref[key + '_rows']).all()
            assert abs(float(ref[key]) - float(clean[key])) > 2e-6 * abs(float(clean[key])), (name, key, ref[key], clean[key])
        for s in range(K.NB):
            a, b = ref['steps'][s], clean['steps'][s]
            assert np.isfinite(a['loss']) and np.isfinite(a['rowloss']).all()
            assert abs(float(a['loss']) - float(b['loss'])) > 2e-6 * abs(float(b['loss'])), (name, s, a['loss'], b['loss'])
            Rw, W, bb = a['params']
            assert np.isfinite(Rw).all() and np.isfinite(W).all()
            assert bb[e] == -np.inf and np.isfinite(np.delete(bb, e)).all()


def _mutant_row_losses(Rw, W, b, X, y, dtype):
    """LogLinearOracle.forward with every clip as fmin(fmax(x, lo), hi) and every max as fmax: both return the operand that
    is not a NaN."""
    dt = np.dtype(dtype)
    lo, hi = O.clip_bounds(dt)

    def clip(a):
        return np.fmin(np.fmax(a, lo), hi)

    def softmax(z):
        m = np.fmax.reduce(z, axis=-1, keepdims=True, initial=-np.inf)
        e = np.exp(z - m)
        return (e / e.sum(axis=-1, keepdims=True)).astype(dt)

    X = np.asarray(X).astype(np.int64)
    Bn, n = X.shape
    G = Rw.astype(dt)[X].reshape(Bn * n, -1)
    P3 = softmax((G @ W.astype(dt) + b.astype(dt)).astype(dt)).reshape(Bn, n, -1)
    J = O._sum(np.log(clip(P3)), axis=1, dtype=dt)
    Qc = clip(softmax(J))
    y = np.asarray(y)
    if y.ndim == 1:
        return -np.log(Qc[np.arange(Bn), y.astype(np.int64)])
    return -O._sum(y.astype(dt) * np.log(Qc), axis=1, dtype=dt)


@pytest.mark.parametrize('name', NAMES)
def test_a_min_max_clip_returns_a_finite_loss_for_every_plant(name):
    c, p = K.case_problem(name)
    for dtype, tol in ((np.float32, 1e-6), (np.float64, 1e-12)):
        clean = K.reference(name, None, dtype)
        for plant in K.PLANTS:
            Rw, W, b, _ = K.planted(name, plant)
            ref = K.reference(name, plant, dtype)
            with np.errstate(all='ignore'):
                X, y, w = K.split(p, 'train')
                rows = _mutant_row_losses(Rw, W, b, X, y, dtype)
                train = float(np.sum(rows.astype(np.float64) * w) / K.B)            # (lambda = 0: no L2 term)
                ev = {'ev_train': float(np.mean(rows.astype(np.float64)))}
                X, y, _ = K.split(p, 'valid')
                ev['ev_valid'] = float(np.mean(_mutant_row_losses(Rw, W, b, X, y, dtype).astype(np.float64)))
            print('%s %-15s %s: mutant train %.6f eval %.6f / %.6f   oracle train %s (clean %.6f)'
                  % (name, plant, np.dtype(dtype).name, train, ev['ev_train'], ev['ev_valid'], ref['steps'][0]['loss'],
                     clean['steps'][0]['loss']))
            assert np.isfinite(train) and np.isfinite(ev['ev_train']) and np.isfinite(ev['ev_valid']), (name, plant)
            if plant == K.CONTROL:              # no NaN anywhere: the two forms of the clip are the same function
                assert abs(train - float(ref['steps'][0]['loss'])) <= tol * abs(train)
                for key in ev:
                    assert abs(ev[key] - float(ref[key])) <= tol * abs(ev[key])
            else:
                assert not np.isfinite(ref['steps'][0]['loss']) and not np.isfinite(ref['ev_train'])
