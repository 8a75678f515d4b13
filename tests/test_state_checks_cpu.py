"""CPU: the state checker of tests/util.py (check_state) against the oracle run twice.

The GPU tests compare the HIP engine's parameters AND both optimiser moments with the oracle (util.check_state),
because the parameters alone do not see how large a gradient is (util.py, above TENSOR_TOL).  This file calibrates
that checker and shows that it bites, without a GPU, with the oracle standing in for the engine:

  (a) the float32 oracle, as the subject, passes check_state against the float64 oracle (used as both references);
      the worst ratio of error to bound -- the margin -- is printed;
  (b) the float32 oracle with one gradient fault injected before an optimiser update fails it: every gradient
      x 1.1 in every step, the sign of one word-table gradient row flipped, one token's contribution to dR_w dropped,
      one candidate's contribution to dR_e dropped, one row of R_w (parameter and moments) left one update behind
      in the last step -- what a lazy row update that missed its flush would leave --, db x 2 and dW x 1.1 in every
      step;
  (c) under Adam, db x 2 passes a check of the parameters alone and fails on m.b and v.b.

Shapes are taken from the GPU matrices of test_gpu_parity.py: vectorspace (Adam), loglinear (Adadelta; int and
CSR labels; it has no entity table, so no candidate mutation) and the additive full softmax (Adam).
"""
import numpy as np
import pytest

from tests import util as U
from tests.util import O

STEPS = 3
LAM = 0.01

VS_DIMS = [
    dict(B=64, n=5, z=4, Vw=500, Ve=37, dw=32, de=48),
    dict(B=17, n=12, z=31, Vw=300, Ve=5, dw=64, de=64),
    dict(B=96, n=3, z=7, Vw=200, Ve=11, dw=30, de=70),
]
LL_DIMS = [
    dict(B=32, n=4, Vw=300, Ve=53, d=24),
    dict(B=33, n=6, Vw=400, Ve=400, d=20),
]
FS_DIMS = [
    dict(B=64, n=5, Vw=500, Ve=37, dw=32, de=48),
    dict(B=96, n=3, Vw=200, Ve=1000, dw=30, de=68),
]
MUTATIONS = ['grads_x1.1', 'row_sign', 'drop_token', 'drop_candidate', 'lazy_row_behind', 'db_x2', 'dW_x1.1']


def _problem(model, dims, labels):
    if model == 'loglinear':
        return U.make_ll_problem(1, dims['B'] * STEPS, dims['n'], dims['Vw'], dims['Ve'], dims['d'], labels)
    return U.make_vs_problem(0 if model == 'vectorspace' else 8, dims['B'] * STEPS, dims['n'], dims.get('z', 0),
                             dims['Vw'], dims['Ve'], dims['dw'], dims['de'], zipf=True)


def _oracle(model, dims, p, dtype):
    B, n = dims['B'], dims['n']
    if model == 'vectorspace':
        return O.VectorSpaceOracle(B, n, dims['z'], p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dtype)
    if model == 'softmax':
        return O.VectorSpaceSoftmaxOracle(B, n, p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dtype)
    return O.LogLinearOracle(B, n, p['Rw'], p['W'], p['b'], LAM, dtype=dtype)


def _rarest(ids):
    """the entry of `ids` (flattened position) whose value occurs least often in it"""
    ids = np.asarray(ids).ravel()
    vals, counts = np.unique(ids, return_counts=True)
    return int(np.flatnonzero(ids == vals[np.argmin(counts)])[0])


def _mutate(model, mutation, ora, X, y, neg, grads, f):
    """Inject one gradient fault (in place) before the optimiser update of the LAST step."""
    i_rw = 1 if model != 'loglinear' else 0          # position of dR_w in the gradient list
    n = X.shape[1]
    if mutation == 'row_sign':
        r = int(X[0, 0])
        grads[i_rw][r] = -grads[i_rw][r]
    elif mutation == 'drop_token':
        k = _rarest(X)
        i, j = divmod(k, n)
        if model == 'loglinear':
            grads[i_rw][X[i, j]] -= f['dG'][k]
        else:
            grads[i_rw][X[i, j]] -= f['dh'][i] / ora.dtype.type(n)
    elif mutation == 'drop_candidate':
        if model == 'vectorspace':
            k = _rarest(f['cand'])
            i, c = divmod(k, f['cand'].shape[1])
            grads[0][f['cand'][i, c]] -= f['du'][i, c] * f['p'][i]
        else:                                         # the full softmax: entity y_i of row i
            i = _rarest(y)
            grads[0][y[i]] -= f['dZ'][i, y[i]] * f['p'][i]
    else:
        assert mutation in ('grads_x1.1', 'lazy_row_behind', 'db_x2', 'dW_x1.1'), mutation


def _run(model, dims, labels, dtype, mutation=None):
    p = _problem(model, dims, labels)
    ora = _oracle(model, dims, p, dtype)
    B = dims['B']
    rng = np.random.RandomState(99)
    y_all = p['ydense'] if model == 'loglinear' else p['y']
    for s in range(STEPS):
        sl = slice(s * B, (s + 1) * B)
        X, y, w = p['X'][sl], y_all[sl], p['w'][sl]
        neg = None
        if model == 'vectorspace':
            neg = rng.randint(0, dims['Ve'], size=(B, dims['z'])).astype(np.int64)
            _, grads, f = ora.loss_and_grads(X, y, w, neg)
        else:
            _, grads, f = ora.loss_and_grads(X, y, w)
        if mutation == 'grads_x1.1':
            grads = [g * ora.dtype.type(1.1) for g in grads]
        elif mutation in ('db_x2', 'dW_x1.1'):                  # one dense gradient scaled in every step
            k, c = (-1, 2.0) if mutation == 'db_x2' else (-2, 1.1)
            grads[k] = grads[k] * ora.dtype.type(c)
        last = s == STEPS - 1
        if last and mutation is not None:
            _mutate(model, mutation, ora, np.asarray(X).astype(np.int64), p['y'][sl], neg, grads, f)
            if mutation == 'lazy_row_behind':
                # a row the last batch does not touch but an earlier one did (the lazy update's rows)
                seen = np.unique(p['X'][:s * B])
                cand = np.setdiff1d(seen, np.unique(X))
                r = int(cand[0]) if len(cand) else int(np.setdiff1d(np.arange(dims['Vw']), np.unique(X))[0])
                before = {k: v[r].copy() for k, v in _row_views(ora, model).items()}
        ora.opt.update(ora.params(), grads)
        if last and mutation == 'lazy_row_behind':
            for k, v in _row_views(ora, model).items():
                v[r] = before[k]
    return U.oracle_state(ora)


def _row_views(ora, model):
    """R_w and its two moments (arrays updated in place by the optimiser, rows addressable)."""
    k = 0 if model == 'loglinear' else 1
    if model == 'loglinear':
        return {'p': ora.R_w, 's0': ora.opt.accu[k], 's1': ora.opt.delta[k]}
    return {'p': ora.R_w, 's0': ora.opt.m[k], 's1': ora.opt.v[k]}


CASES = ([('vectorspace', d, 'int') for d in VS_DIMS] +
         [('loglinear', d, lab) for d in LL_DIMS for lab in ('int', 'csr')] +
         [('softmax', d, 'int') for d in FS_DIMS])
IDS = ['%s-%s-B%d' % (m, lab, d['B']) for m, d, lab in CASES]


@pytest.fixture(scope='module')
def references():
    cache = {}

    def get(model, dims, labels):
        key = (model, tuple(sorted(dims.items())), labels)
        if key not in cache:
            cache[key] = (_run(model, dims, labels, np.float32), _run(model, dims, labels, np.float64))
        return cache[key]
    return get


def _margin(got, ref64):
    """worst (error / bound) over the state entries, float32 oracle against the float64 one"""
    worst, where = 0.0, None
    for k in ref64:
        sq = k.rpartition('.')[0] in U.SECOND_MOMENTS
        for e, tol in ((U.rel_err(got[k], ref64[k]), U.TENSOR_TOL),
                       (U.row_err(got[k], ref64[k])[0], (2 if sq else 1) * U.ROW_TOL64)):
            if e / tol > worst:
                worst, where = e / tol, k
    return worst, where


@pytest.mark.parametrize('model,dims,labels', CASES, ids=IDS)
def test_float32_oracle_passes_against_float64(references, model, dims, labels):
    s32, s64 = references(model, dims, labels)
    assert set(s32) == set(s64)
    assert len(s32) == 3 * (3 if model == 'loglinear' else 4)
    log = U.check_state(s32, s64, s64)
    worst, where = _margin(s32, s64)
    print('\n'.join(log))
    print('margin: worst error / bound = %.3f (%s)' % (worst, where))
    assert worst < 1.0


# (loglinear has no entity table: no candidate mutation)
MUT_CASES = [c + (m,) for c in CASES for m in MUTATIONS if not (m == 'drop_candidate' and c[0] == 'loglinear')]
MUT_IDS = ['%s-%s' % (i, m) for i, c in zip(IDS, CASES) for m in MUTATIONS
           if not (m == 'drop_candidate' and c[0] == 'loglinear')]


@pytest.mark.parametrize('model,dims,labels,mutation', MUT_CASES, ids=MUT_IDS)
def test_each_gradient_fault_fails_the_state_check(references, model, dims, labels, mutation):
    s32, s64 = references(model, dims, labels)
    bad = _run(model, dims, labels, np.float32, mutation)
    with pytest.raises(AssertionError):
        U.check_state(bad, s32, s64)


ADAM_CASES = [c for c in CASES if c[0] != 'loglinear']


@pytest.mark.parametrize('model,dims,labels', ADAM_CASES, ids=[IDS[CASES.index(c)] for c in ADAM_CASES])
def test_parameters_alone_miss_a_doubled_bias_gradient(references, model, dims, labels):
    """Why the moments are checked: under Adam, db x 2 in every step leaves every parameter within its bounds
    (m_hat / sqrt(v_hat) does not see a constant factor), while m.b moves by 100 % and v.b by 300 %."""
    s32, s64 = references(model, dims, labels)
    bad = _run(model, dims, labels, np.float32, 'db_x2')
    U.check_state(bad, s32, s64, names=[k for k in s32 if '.' not in k])
    with pytest.raises(AssertionError):
        U.check_state(bad, s32, s64, names=['m.b'])
    with pytest.raises(AssertionError):
        U.check_state(bad, s32, s64, names=['v.b'])
