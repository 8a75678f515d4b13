"""Inputs of the loglinear fold-in tests on label ROWS (sert_ll_foldin_upload_csr; tests/test_ll_foldin_label_inputs_cpu.py
proves their structure, tests/test_gpu_ll_foldin_labels.py runs them) and the oracle twin of such a step.

The labels of an instance are a CSR row over V_e + N columns: column e < V_e is trained entity e -- a label only, its
parameters stay frozen --, column V_e + j new entity j.  Every case is the smallest shape at which one mechanism of
llf_row_csr (csrc/kernels_ll_foldin.h) is live.  The twin is tests/ll_foldin_cases.LlFoldInTwin with one method replaced: a
batch's labels are the dense (B, V_e + N) slice of the rows, which LogLinearOracle takes as it stands.  It restates no maths.
"""
import numpy as np

from oracle import sert_oracle as O
from tests import ll_foldin_cases as LC

STEPS = LC.STEPS
BASE = LC.BASE
TRAILING = LC.TRAILING
CLIP_SCALE = LC.CLIP_SCALE
CLIP_MARGIN = LC.CLIP_MARGIN
MIXED_COUNTS = (0, 1, 2, 3, None)          # labels per row, cycled; None: every column
WIDE_COUNTS = (255, 256, 257, 600)         # wide: rows 0 .. 3 of every batch
WIDE_TAIL = 290                            # ... of the 600, on new columns: a tail longer than the workgroup is wide

# name -> (overrides of BASE, the structure the case exists for)
CASES = {
    'mixed': (dict(), 'rows of 0, 1, 2, 3 and V_e + N entries whose values do not sum to 1; a row whose only entry is trained, '
                      'one whose only entry is new, a row on the seam (V_e - 1, V_e), a row on columns 0 and V_e + N - 1'),
    'frozen_only': (dict(), 'every entry of batch 0 on a trained column: the new columns still have a gradient'),
    'no_labels': (dict(lam=0.0), 'batch 0 without an entry and lambda = 0: loss exactly 0, Wn and bn keep their bits'),
    'one_hot': (dict(), 'one entry of value 1 at V_e + y per row, from the base case of the integer upload'),
    'wide': (dict(Ve=700, N=300), 'rows of 255, 256, 257 and 600 entries on both sides of the seam: more entries than the '
                                  'workgroup is wide and a new-side tail of %d' % WIDE_TAIL),
    'n1': (dict(n=1), 'the NMAX = 8 bucket at its smallest; one trained and one new entry per row'),
    'n9': (dict(n=9), 'the NMAX = 16 bucket; one trained and one new entry per row'),
    'n32': (dict(n=32), 'the NMAX = 32 bucket; one trained and one new entry per row'),
    'odd_d': (dict(d=7), 'word dimension not a multiple of 4'),
    'batch_of_one': (dict(B=1), 'a single instance per batch'),
    'stored_zero': (dict(), 'a stored 0 among the values of every third row'),
    'clip_live_labels': (dict(), 'W and the initial Wn scaled by %g, one trained and one new entry of 0.5 per row: in every step '
                                 'trained and new label entries with Q below 1e-7 and above it, clipped frozen and new token '
                                 'probabilities, nothing within %g of a clip bound' % (CLIP_SCALE, CLIP_MARGIN)),
}


def _pair(rng, Ve, N):
    """one trained and one new column"""
    return [int(rng.randint(0, Ve)), Ve + int(rng.randint(0, N))]


def _rows(name, c, rng):
    """-> per instance (sorted distinct columns, values)"""
    Ve, N, B, M = c['Ve'], c['N'], c['B'], c['M']
    V = Ve + N
    rows = []
    for i in range(M):
        if name == 'mixed':
            k = MIXED_COUNTS[i % len(MIXED_COUNTS)]
            cols = list(range(V)) if k is None else sorted(rng.choice(V, k, replace=False).tolist())
            # (rows 1, 6, 2 and 7 of batch 0 have 1, 1, 2 and 2 entries)
            cols = {1: [Ve - 2], 6: [Ve + 1], 2: [Ve - 1, Ve], 7: [0, V - 1]}.get(i, cols)
        elif name == 'frozen_only' and i < B:
            cols = sorted(rng.choice(Ve, 1 + i % 2, replace=False).tolist())
        elif name == 'no_labels' and i < B:
            cols = []
        elif name == 'wide' and i % B < len(WIDE_COUNTS):
            k = WIDE_COUNTS[i % B]
            if k == 600:
                cols = sorted(rng.choice(Ve, k - WIDE_TAIL, replace=False).tolist()) + \
                    sorted((Ve + rng.choice(N, WIDE_TAIL, replace=False)).tolist())
            else:
                cols = sorted(rng.choice(V, k, replace=False).tolist())
        elif name in ('odd_d', 'batch_of_one', 'stored_zero'):
            cols = sorted(rng.choice(V, 3, replace=False).tolist())
        else:
            cols = _pair(rng, Ve, N)
        vals = rng.uniform(0.1, 1.0, len(cols))
        if name == 'wide':
            vals = vals / max(len(cols), 1)              # (the mass of a row stays of order 1)
        if name == 'clip_live_labels':
            vals[:] = 0.5
        if name == 'stored_zero' and i % 3 == 0:
            vals[i % len(cols)] = 0.0
        rows.append((cols, vals.astype(np.float32)))
    return rows


def csr_of(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(cols) for cols, _ in rows])
    indices = np.asarray([e for cols, _ in rows for e in cols], np.int32)
    data = np.concatenate([v for _, v in rows] + [np.zeros(0, np.float32)]).astype(np.float32)
    return indptr, indices, data


def densify(indptr, indices, data, width):
    Y = np.zeros((len(indptr) - 1, width), np.float32)
    Y[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = data
    return Y


def _build(name, seed):
    over, structure = CASES[name]
    if name == 'one_hot':
        c = dict(LC.make_case('base'))
        rows = [([c['Ve'] + int(y)], np.ones(1, np.float32)) for y in c['y']]
    else:
        c = dict(BASE)
        c.update(over)
        rng = np.random.RandomState(seed)
        Vw, Ve, N, d, n, B = (c[k] for k in ('Vw', 'Ve', 'N', 'd', 'n', 'B'))
        M = 3 * B + TRAILING
        c['M'], c['batches'] = M, M // B
        c['Rw'] = O.glorot_uniform(rng, (Vw, d))
        c['W'] = O.glorot_uniform(rng, (d, Ve))
        c['b'] = (0.1 * rng.randn(Ve)).astype(np.float32)
        c['Wn0'] = O.glorot_uniform(rng, (d, N))
        c['bn0'] = (0.1 * rng.randn(N)).astype(np.float32)
        c['X'] = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
        c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
        if name == 'clip_live_labels':
            c['W'] = (c['W'] * np.float32(CLIP_SCALE)).astype(np.float32)
            c['Wn0'] = (c['Wn0'] * np.float32(CLIP_SCALE)).astype(np.float32)
        rows = _rows(name, c, rng)
    c['name'], c['structure'] = name, structure
    c['indptr'], c['indices'], c['data'] = csr_of(rows)
    c['Ydense'] = densify(c['indptr'], c['indices'], c['data'], c['Ve'] + c['N'])
    return c


class LlLabelTwin(LC.LlFoldInTwin):
    """LlFoldInTwin whose labels are the dense (B, V_e + N) slice of the case's rows."""

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], c['Ydense'][sl], c['w'][sl]


def clip_report(c):
    """clip_live_labels' conditions over the three steps (step s trains batch s) and the evaluation of batch 1 after step 0,
    on the float64 twin -> counts per step and the smallest relative distance of a P or a label's Q from a clip bound."""
    tw = LlLabelTwin(c, np.float64)
    lo, hi = O.clip_bounds(np.float64)
    Ve, B = c['Ve'], c['B']
    rep = dict(frozen_clipped=0, new_clipped=0, frozen_total=0, new_total=0, trained_labels_clipped=[], new_labels_clipped=[],
               margin=np.inf, finite=True, grad_nonzero=True)

    def look(batch, count):
        f = tw.forward(batch)
        P, Q = f['P3'], f['Q']
        stored = densify(c['indptr'], c['indices'], np.ones_like(c['data']), Ve + c['N'])[batch * B:(batch + 1) * B] > 0
        for v in (P, Q[stored]):
            for bound in (lo, hi):
                rep['margin'] = min(rep['margin'], float(np.abs(v - bound).min() / bound))
        if count:
            rep['frozen_clipped'] += int((P[:, :, :Ve] < lo).sum())
            rep['new_clipped'] += int((P[:, :, Ve:] < lo).sum())
            rep['frozen_total'] += P[:, :, :Ve].size
            rep['new_total'] += P[:, :, Ve:].size
            rep['trained_labels_clipped'].append(int((Q[:, :Ve][stored[:, :Ve]] < lo).sum()))
            rep['new_labels_clipped'].append(int((Q[:, Ve:][stored[:, Ve:]] < lo).sum()))

    for s in range(STEPS):
        look(s, True)
        _, gW, gb = tw.train_step(s, return_grads=True)
        rep['finite'] = rep['finite'] and bool(np.isfinite(gW).all() and np.isfinite(gb).all())
        rep['grad_nonzero'] = rep['grad_nonzero'] and bool(np.abs(gW).max() > 0)
        if s == 0:
            look(1, False)
    return rep


def clip_ok(rep, B):
    """(a row has one trained and one new entry: B of either per step)"""
    return (rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0 and
            all(0 < k < B for k in rep['trained_labels_clipped']) and all(0 < k < B for k in rep['new_labels_clipped']) and
            rep['margin'] > CLIP_MARGIN and rep['finite'] and rep['grad_nonzero'])


_made = {}


def make_case(name):
    """The case, generated once per process.  clip_live_labels: the first seed of a fixed sequence whose float64 trajectory
    meets every condition of clip_report (case generation ENFORCES them; the CPU test asserts them again)."""
    if name in _made:
        return _made[name]
    seed = 3000 + sorted(CASES).index(name)
    if name != 'clip_live_labels':
        c = _build(name, seed)
    else:
        for attempt in range(400):
            c = _build(name, 3000 + 100 * attempt)
            if clip_ok(clip_report(c), c['B']):
                c['attempt'] = attempt
                break
        else:
            raise RuntimeError('no clip_live_labels input meets its conditions in 400 seeds')
    _made[name] = c
    return c
