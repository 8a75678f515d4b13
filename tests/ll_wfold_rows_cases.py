"""Inputs of the loglinear word fold-in tests on label ROWS (tests/test_ll_wfold_rows_inputs_cpu.py proves their structure,
tests/test_gpu_ll_wfold_rows.py runs them) and the oracle twin of such a step.

sert_ll_wfold_upload_csr gives instance i the CSR row i of a matrix Y (M, V_e) over the trained entities as its labels
(include/sert_hip_ll_wfold.h); llw_row_csr (csrc/kernels_ll_wfold.h) is the row kernel that reads them.  The cases build on
ll_wfold_cases.BASE and draw their parameters and tokens as ll_wfold_cases does; each is the smallest shape at which one
mechanism of llw_row_csr is live, `structure` names it, the property is forced by construction and the CPU test proves it from
the arrays.  The twin is ll_wfold_cases.LlWordFoldInTwin with ONE method replaced: a batch's labels are the dense (B, V_e) slice
of the rows, which LogLinearOracle takes as they are (y.ndim == 2).  It restates no maths.
"""
import numpy as np
import scipy.sparse

from oracle import sert_oracle as O
from tests import ll_wfold_cases as LW

STEPS = LW.STEPS
BASE = LW.BASE
TRAILING = LW.TRAILING
REG_MAX_VE = LW.REG_MAX_VE
CLIP_SCALE = LW.CLIP_SCALE
CLIP_MARGIN = LW.CLIP_MARGIN
WG = 256                    # the threads of llw_row_csr's workgroup: entry l of a row belongs to thread (l - l0) % WG
WIDE_COUNTS = (255, 256, 257, 600)

# name -> (overrides of BASE, the structure the case exists for)
CASES = {
    'mixed': (dict(), 'rows of 0, 1, 2, 3 and V_e entries, cycled; values that do not sum to 1; a row on columns 0 and V_e - 1; '
                      'a window with a new word twice; an instance with no new word'),
    've8': (dict(Ve=8), 'register form, 16-byte rows; one row holds the four adjacent columns 4 .. 7: every element of one '
                        "thread's float4 is a label"),
    'wide': (dict(Ve=700), 'rows of 255, 256, 257 and 600 entries in rows 0 .. 3 of every batch: more entries than the workgroup '
                           'is wide; values divided by the count'),
    've1024': (dict(Ve=1024), 'the last V_e of the register form'),
    've1025': (dict(Ve=1025), 'the first V_e of the streaming form, scalar rows; a row with every column and a row with none'),
    've1028': (dict(Ve=1028), 'the streaming form with 16-byte rows; a row with every column and a row with none'),
    'no_labels': (dict(lam=0.0), 'no row of batch 0 has an entry and there is no L2 term: the loss is exactly 0 and nothing moves'),
    'one_hot': (dict(), "one entry of value 1 at y of ll_wfold_cases' base case: the integer upload's instances as rows"),
    'stored_zero': (dict(), 'a stored 0 in every third row'),
    'n1': (dict(n=1), 'window of one token, two entries per row'),
    'n32': (dict(n=32), 'the window limit, two entries per row'),
    'all_new': (dict(), 'every token is a new word: no frozen word, an empty frozen table'),
    'batch_of_one': (dict(B=1), 'a single instance per batch'),
    'clip_live_rows': (dict(), 'W scaled by %g, two entries of 0.5 per row: in every step label entries with Q below 1e-7 and '
                               'entries above it, clipped frozen and new token probabilities, nothing within %g of a clip bound'
                               % (CLIP_SCALE, CLIP_MARGIN)),
}


def _rows(rng, Ve, counts, scale_by_count=False):
    """A canonical CSR matrix (len(counts), Ve) float32: row i holds counts[i] distinct columns, ascending, with values drawn
    from [0.1, 1) -- they do not sum to 1 -- or divided by the count."""
    indptr = np.zeros(len(counts) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(counts)
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    data = rng.uniform(0.1, 1.0, size=indices.size).astype(np.float32)
    for i, k in enumerate(counts):
        indices[indptr[i]:indptr[i + 1]] = np.sort(rng.choice(Ve, int(k), replace=False))
        if scale_by_count and k:
            data[indptr[i]:indptr[i + 1]] /= np.float32(k)
    return indptr, indices, data


def _set_row(indptr, indices, data, i, cols, vals=None):
    """Row i, which must hold len(cols) entries already, gets these columns (and values)."""
    assert indptr[i + 1] - indptr[i] == len(cols)
    indices[indptr[i]:indptr[i + 1]] = cols
    if vals is not None:
        data[indptr[i]:indptr[i + 1]] = vals


def _build(name, seed):
    over, structure = CASES[name]
    if name == 'one_hot':
        c = dict(LW.make_case('base'))
        c['name'], c['structure'] = name, structure
        M = c['M']
        c['indptr'] = np.arange(M + 1, dtype=np.int64)
        c['indices'] = c['y'].astype(np.int32).copy()
        c['data'] = np.ones(M, dtype=np.float32)
        return _finish(c)
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
    rng = np.random.RandomState(seed)
    Vw, Nw, Ve, d, n, B = (c[k] for k in ('Vw', 'Nw', 'Ve', 'd', 'n', 'B'))
    M = 3 * B + TRAILING
    c['M'], c['batches'] = M, M // B
    # parameters, new rows and tokens as ll_wfold_cases draws them
    c['Rw'] = O.glorot_uniform(rng, (Vw, d))
    c['W'] = O.glorot_uniform(rng, (d, Ve))
    c['b'] = (0.1 * rng.randn(Ve)).astype(np.float32)
    bound = np.sqrt(6.0 / (Vw + d))
    c['Nv0'] = rng.uniform(-bound, bound, size=(Nw, d)).astype(np.float32)
    X = rng.randint(0, Vw + Nw, size=(M, n)).astype(np.int32)
    if name == 'mixed':
        X[0] = (Vw, 3, Vw)                              # a new word twice in one window ...
        X[2] = (1, 2, 3)                                # ... an instance with none
    elif name == 'all_new':
        X = rng.randint(Vw, Vw + Nw, size=(M, n)).astype(np.int32)
    c['X'] = X
    c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
    i = np.arange(M)
    if name == 'mixed':
        counts = np.array([0, 1, 2, 3, Ve])[i % 5]
        lab = _rows(rng, Ve, counts)
        _set_row(*lab, i=2, cols=(0, Ve - 1))
    elif name == 've8':
        counts = np.array([1, 4, 2, 3])[i % 4]
        lab = _rows(rng, Ve, counts)
        _set_row(*lab, i=1, cols=(4, 5, 6, 7))
    elif name == 'wide':
        counts = np.where(i % B < 4, np.array(WIDE_COUNTS)[i % B % 4], 1 + i % 3)
        lab = _rows(rng, Ve, counts, scale_by_count=True)
    elif name in ('ve1025', 've1028'):
        counts = np.array([1, 2, 3, 5])[i % 4]
        counts[0], counts[1] = Ve, 0
        lab = _rows(rng, Ve, counts, scale_by_count=True)
    elif name == 've1024':
        counts = np.array([1, 2, 3, 5])[i % 4]
        lab = _rows(rng, Ve, counts)
    elif name == 'no_labels':
        counts = np.where(i < B, 0, 1 + i % 3)
        lab = _rows(rng, Ve, counts)
    elif name == 'stored_zero':
        counts = 1 + i % 3
        lab = _rows(rng, Ve, counts)
        lab[2][lab[0][:-1][::3]] = 0.0                  # the first entry of every third row is a stored 0
    elif name in ('n1', 'n32'):
        lab = _rows(rng, Ve, np.full(M, 2))
    elif name == 'clip_live_rows':
        lab = _rows(rng, Ve, np.full(M, 2))
        lab[2][:] = 0.5
        c['W'] = (c['W'] * np.float32(CLIP_SCALE)).astype(np.float32)
        # With W at this scale most rows' Q is all but one-hot, and a label on such a column sits within CLIP_MARGIN of the
        # upper bound: a row's two columns are drawn among those whose Q at Nv0 is below 0.99 (float64; every row has six).
        ext = np.concatenate([c['Rw'], c['Nv0']], axis=0)
        for b0 in range(0, M - B + 1, B):
            Q = O.LogLinearOracle(B, n, ext, c['W'], c['b'], 0.0, dtype=np.float64).forward(X[b0:b0 + B], np.zeros(B, np.int64))['Q']
            for r in range(B):
                _set_row(*lab, i=b0 + r, cols=np.sort(rng.choice(np.flatnonzero(Q[r] < 0.99), 2, replace=False)))
    else:                                               # all_new, batch_of_one
        lab = _rows(rng, Ve, 1 + i % 3)
    c['indptr'], c['indices'], c['data'] = lab
    return _finish(c)


def _finish(c):
    """The rows as the matrix they are (stored zeros kept) and as the dense slice source of the twin."""
    shape = (c['M'], c['Ve'])
    c['Y'] = scipy.sparse.csr_matrix((c['data'], c['indices'], c['indptr']), shape=shape)
    dense = np.zeros(shape, dtype=np.float32)
    rows = np.repeat(np.arange(c['M']), np.diff(c['indptr']))
    dense[rows, c['indices']] = c['data']               # (columns are distinct within a row: an assignment, no sum)
    c['Ydense'] = dense
    return c


new_tokens = LW.new_tokens
index_of_batch = LW.index_of_batch


def expected_plan(c, batch):
    """What sert_debug_ll_wfold_plan must report after a training step on `batch` of a ROWS upload."""
    plan = LW.expected_plan(c, batch)
    plan['labels'] = 'rows'
    return plan


class LlWordFoldInRowsTwin(LW.LlWordFoldInTwin):
    """ll_wfold_cases.LlWordFoldInTwin on label rows: the labels of a batch are the dense (B, V_e) slice of the rows."""

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], c['Ydense'][sl], c['w'][sl]


def clip_report(c):
    """clip_live_rows' conditions over the three steps (step s trains batch s) and the evaluation of batch 1 after step 0, on
    the float64 twin -> dict of counts and the smallest relative distance of a P or a label's Q from a clip bound."""
    tw = LlWordFoldInRowsTwin(c, np.float64)
    lo, hi = O.clip_bounds(np.float64)
    B, Vw = c['B'], c['Vw']
    rep = dict(frozen_clipped=0, new_clipped=0, frozen_total=0, new_total=0, labels_clipped=[], labels_total=[], margin=np.inf,
               finite=True, grad_nonzero=True)

    def look(batch, count):
        f = tw.forward(batch)
        P, Q = f['P3'], f['Q']
        new = c['X'][batch * B:(batch + 1) * B] >= Vw
        Ql = Q[c['Ydense'][batch * B:(batch + 1) * B] != 0]
        for v in (P, Ql):
            for bound in (lo, hi):
                rep['margin'] = min(rep['margin'], float(np.abs(v - bound).min() / bound))
        if count:
            rep['frozen_clipped'] += int((P[~new] < lo).sum())
            rep['new_clipped'] += int((P[new] < lo).sum())
            rep['frozen_total'] += P[~new].size
            rep['new_total'] += P[new].size
            rep['labels_clipped'].append(int((Ql < lo).sum()))
            rep['labels_total'].append(int(Ql.size))

    for s in range(STEPS):
        look(s, True)
        _, g = tw.train_step(s, return_grads=True)
        rep['finite'] = rep['finite'] and bool(np.isfinite(g).all())
        rep['grad_nonzero'] = rep['grad_nonzero'] and bool(np.abs(g).max() > 0)
        if s == 0:
            look(1, False)
    return rep


def clip_ok(rep):
    return (rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0 and
            all(0 < k < total for k, total in zip(rep['labels_clipped'], rep['labels_total'])) and
            rep['margin'] > CLIP_MARGIN and rep['finite'] and rep['grad_nonzero'])


_made = {}


def make_case(name):
    """The case, generated once per process.  clip_live_rows: the first seed of ll_wfold_cases' fixed sequence (at most 400)
    whose float64 trajectory meets every condition of clip_report (case generation ENFORCES them; the CPU test asserts them
    again)."""
    if name in _made:
        return _made[name]
    seed = 4000 + sorted(CASES).index(name)
    if name != 'clip_live_rows':
        c = _build(name, seed)
    else:
        for attempt in range(400):
            c = _build(name, seed + 100 * attempt)
            if clip_ok(clip_report(c)):
                c['attempt'] = attempt
                break
        else:
            raise RuntimeError('no clip_live_rows input meets its conditions in 400 seeds')
    _made[name] = c
    return c
