"""Inputs of the tests of a loglinear fold-in that REFRESHES trained columns (sert_ll_foldin_create_refresh;
tests/test_ll_refresh_inputs_cpu.py proves their structure, tests/test_gpu_ll_refresh.py runs them) and the oracle twin of
such a step.

The trainable columns are slots: slot s < R stands for trained column refresh[s], slot R + j for column V_e + j of the
extended model (include/sert_hip_ll_foldin.h).  Every case is the smallest shape at which one mechanism is live; the shapes
are tests/ll_foldin_cases.BASE's.  The twin restates no maths: it scatters the slots into Wx / bx, asks
oracle.sert_oracle.LogLinearOracle for loss and gradient, picks the gradient's columns ext_of_slot and updates with
oracle.Adadelta.  `deleted(c)` is the same problem as a PLAIN fold-in: a model of the V_f frozen columns alone, into which
[the refreshed columns, the new ones] are folded as Nt new columns -- what the device handle runs.
"""
import numpy as np

from oracle import sert_oracle as O
from tests import ll_foldin_cases as LC
from tests import ll_foldin_label_cases as LL

STEPS = LC.STEPS
BASE = LC.BASE
TRAILING = LC.TRAILING
CLIP_SCALE = LC.CLIP_SCALE
CLIP_MARGIN = LC.CLIP_MARGIN
WIDE_REFRESHED = 300
WIDE_ROW = (40, 260, 3)          # csr_wide, row 0 of every batch: entries on frozen, refreshed and new columns

# name -> (overrides of BASE, refresh ids or a callable rng -> ids, the structure the case exists for)
CASES = {
    'mixed': (dict(N=3), [5, 1], 'slot order is not ascending: slot 0 is column 5, slot 1 column 1'),
    'first_last': (dict(), [0, 6], 'the first and the last trained column are refreshed'),
    'refresh_only': (dict(N=0), [2, 4, 3], 'no new column: N = 0'),
    'one_frozen': (dict(N=2), [6, 0, 2, 1, 5, 4], 'a single frozen column: V_f = 1'),
    'all_refreshed': (dict(N=2), [3, 6, 0, 5, 1, 4, 2], 'every trained column refreshed, ids permuted: V_f = 0, no logit cache'),
    'wide': (dict(Ve=700), 'wide', '300 refreshed ids with 0 and 699 among them: Nt = 305 is wider than a workgroup, V_f = 400 '
                                   'no multiple of 256'),
    'unvisited_slot': (dict(N=2), [5, 1, 3], 'slot 2 (column 3) has no instance in any batch, and moves all the same'),
    'clip_live': (dict(N=3), [5, 1], 'W and the initial new columns scaled by %g: token probabilities below 1e-7 among frozen, '
                                     'refreshed and new columns, labels with Q_y below 1e-7 and labels above it, nothing within '
                                     '%g of a clip bound' % (CLIP_SCALE, CLIP_MARGIN)),
    'csr_mixed': (dict(N=3), [5, 1], 'label rows on frozen, refreshed and new columns; a row whose refreshed entries ascend in '
                                     'public order (1, 5) and descend in slot order (1, 0); a row of refreshed entries only; an '
                                     'empty row; a stored zero'),
    'csr_wide': (dict(Ve=700), 'wide', 'a row of %d + %d + %d entries on frozen, refreshed and new columns: more entries than '
                                       'a workgroup is wide and a trainable tail above 256' % WIDE_ROW),
    'csr_all_refreshed': (dict(N=2), [3, 6, 0, 5, 1, 4, 2], 'label rows with V_f = 0: every entry is in the trainable tail'),
}
CSR_CASES = tuple(sorted(k for k in CASES if k.startswith('csr_')))


def is_csr(c):
    return 'indptr' in c


def internal_of(c):
    """public column -> internal column: the frozen columns in ascending trained index, the refreshed slots, the new columns."""
    Ve, N, refresh = c['Ve'], c['N'], np.asarray(c['refresh'], np.int64)
    out = np.full(Ve + N, -1, np.int64)
    frozen = np.setdiff1d(np.arange(Ve), refresh)
    out[frozen] = np.arange(frozen.size)
    out[refresh] = frozen.size + np.arange(refresh.size)
    out[Ve:] = Ve + np.arange(N)
    return out.astype(np.int32)


def _csr_rows(name, c, rng):
    Ve, N, B, M = c['Ve'], c['N'], c['B'], c['M']
    refresh = list(c['refresh'])
    frozen = [e for e in range(Ve) if e not in set(refresh)]
    new = list(range(Ve, Ve + N))
    rows = []
    for i in range(M):
        k = i % B
        if name == 'csr_mixed':
            fixed = {0: sorted([frozen[0], refresh[1], refresh[0], new[1]]),      # all three kinds; (1, 5): slots (1, 0)
                     1: sorted(refresh),                                         # refreshed entries only
                     2: [],                                                      # an empty row
                     3: sorted([frozen[-1], new[0]]), 4: [refresh[0]], 5: [new[-1]], 6: list(range(Ve + N))}
            cols = fixed[k] if k in fixed else sorted(rng.choice(Ve + N, 1 + k % 4, replace=False).tolist())
        elif name == 'csr_wide' and k == 0:
            nf, nr, nn = WIDE_ROW
            cols = sorted(rng.choice(frozen, nf, replace=False).tolist() + rng.choice(refresh, nr, replace=False).tolist() +
                          rng.choice(new, nn, replace=False).tolist())
        elif name == 'csr_wide':
            cols = sorted({int(rng.choice(frozen)), int(rng.choice(refresh)), int(rng.choice(refresh)), int(rng.choice(new))})
        else:       # csr_all_refreshed
            cols = [] if k == 2 else sorted(rng.choice(Ve + N, 1 + k % 4, replace=False).tolist())
        vals = rng.uniform(0.1, 1.0, len(cols))
        if len(cols) > 16:
            vals = vals / len(cols) * 4          # (the mass of a row stays of order 1)
        if name == 'csr_mixed' and k == 3:
            vals[0] = 0.0                        # a stored zero, on a frozen column
        if name == 'csr_mixed' and k == 0 and i >= B:
            vals[2] = 0.0                        # ... and, from batch 1 on, on a refreshed one
        rows.append((cols, vals.astype(np.float32)))
    return rows


def _build(name, seed):
    over, refresh, structure = CASES[name]
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
    rng = np.random.RandomState(seed)
    Vw, Ve, N, d, n, B = (c[k] for k in ('Vw', 'Ve', 'N', 'd', 'n', 'B'))
    M = 3 * B + TRAILING
    c['M'], c['batches'] = M, M // B
    if isinstance(refresh, str):
        inner = 1 + rng.choice(Ve - 2, WIDE_REFRESHED - 2, replace=False)
        refresh = rng.permutation(np.concatenate([[0, Ve - 1], inner])).tolist()
    c['refresh'] = np.asarray(refresh, np.int32)
    R = c['R'] = len(refresh)
    c['Nt'], c['Vf'] = R + N, Ve - R
    c['ext_of_slot'] = np.concatenate([c['refresh'], Ve + np.arange(N)]).astype(np.int64)
    c['Rw'] = O.glorot_uniform(rng, (Vw, d))
    c['W'] = O.glorot_uniform(rng, (d, Ve))
    c['b'] = (0.1 * rng.randn(Ve)).astype(np.float32)
    c['Wn0'] = O.glorot_uniform(rng, (d, N)) if N else np.zeros((d, 0), np.float32)
    c['bn0'] = (0.1 * rng.randn(N)).astype(np.float32)
    c['X'] = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
    c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
    if name == 'clip_live':
        c['W'] = (c['W'] * np.float32(CLIP_SCALE)).astype(np.float32)
        c['Wn0'] = (c['Wn0'] * np.float32(CLIP_SCALE)).astype(np.float32)
    if name in CSR_CASES:
        c['indptr'], c['indices'], c['data'] = LL.csr_of(_csr_rows(name, c, rng))
        c['Ydense'] = LL.densify(c['indptr'], c['indices'], c['data'], Ve + N)
    else:
        y = rng.randint(0, c['Nt'], size=M).astype(np.int32)
        if name == 'unvisited_slot':
            y[y == 2] = 0
        c['y'] = y
    return c


def deleted(c):
    """The case as a PLAIN fold-in (tests/ll_foldin_cases.LlFoldInTwin, C.LlFoldIn): the model holds the V_f frozen columns
    only, the Nt slots are its new columns, integer labels stay (a slot IS the new column), label rows go to internal columns."""
    if '_deleted' in c:
        return c['_deleted']
    frozen = np.setdiff1d(np.arange(c['Ve']), c['refresh'])
    p = dict(c)
    p.update(Ve=c['Vf'], N=c['Nt'], W=np.ascontiguousarray(c['W'][:, frozen]), b=np.ascontiguousarray(c['b'][frozen]),
             Wn0=np.ascontiguousarray(np.concatenate([c['W'][:, c['refresh']], c['Wn0']], axis=1)),
             bn0=np.concatenate([c['b'][c['refresh']], c['bn0']]).astype(np.float32))
    if is_csr(c):
        io = internal_of(c)
        rows = []
        for i in range(c['M']):
            a, b = c['indptr'][i], c['indptr'][i + 1]
            cols = io[c['indices'][a:b]]
            order = np.argsort(cols, kind='stable')
            rows.append((cols[order].tolist(), c['data'][a:b][order]))
        p['indptr'], p['indices'], p['data'] = LL.csr_of(rows)
        p['Ydense'] = LL.densify(p['indptr'], p['indices'], p['data'], c['Vf'] + c['Nt'])
    c['_deleted'] = p
    return p


class LlRefreshTwin(object):
    """The refreshing loglinear fold-in on the CPU, on oracle objects alone.  dtype: float32 (the reference's) or float64."""

    def __init__(self, c, dtype=np.float32):
        self.c, self.dt = c, np.dtype(dtype)
        self.Wt = np.array(np.concatenate([c['W'][:, c['refresh']], c['Wn0']], axis=1), dtype=self.dt)
        self.bt = np.array(np.concatenate([c['b'][c['refresh']], c['bn0']]), dtype=self.dt)
        self.opt = O.Adadelta([self.Wt, self.bt], lr=1.0, rho=0.95, eps=1e-6)

    def extended(self):
        """Wx (d, V_e + N), bx: concat(W, new) with every slot's current value written to its column."""
        c = self.c
        Wx = np.concatenate([np.asarray(c['W'], dtype=self.dt), np.zeros((c['d'], c['N']), self.dt)], axis=1)
        bx = np.concatenate([np.asarray(c['b'], dtype=self.dt), np.zeros(c['N'], self.dt)])
        Wx[:, c['ext_of_slot']] = self.Wt
        bx[c['ext_of_slot']] = self.bt
        return Wx, bx

    def _oracle(self, lam):
        c = self.c
        Wx, bx = self.extended()
        return O.LogLinearOracle(c['B'], c['n'], c['Rw'], Wx, bx, lam, dtype=self.dt)

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        labels = c['Ydense'][sl] if is_csr(c) else c['ext_of_slot'][c['y'][sl]]
        return c['X'][sl], labels, c['w'][sl]

    def forward(self, batch):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).forward(X, y)

    def train_step(self, batch, return_grads=False):
        """-> the returned loss (before the update): data term + lambda / (2B) sum(Wt Wt); then oracle.Adadelta on [Wt, bt]."""
        c = self.c
        X, y, w = self._batch(batch)
        _, grads, _ = self._oracle(c['lam']).loss_and_grads(X, y, w)
        ext = c['ext_of_slot']
        gW, gb = grads[1][:, ext], grads[2][ext]          # gW includes lambda / B * Wt; the bias is not regularised
        data, _, _ = self._oracle(0.0).loss_and_grads(X, y, w)
        # LogLinearOracle.regularizer() of a model whose only non-zero tensor is Wt
        zero = lambda *shape: np.zeros(shape, dtype=self.dt)
        reg = O.LogLinearOracle(c['B'], c['n'], zero(1, c['d']), self.Wt, zero(c['Nt']), c['lam'], dtype=self.dt).regularizer()
        gW, gb = np.array(gW, dtype=self.dt), np.array(gb, dtype=self.dt)
        self.opt.update([self.Wt, self.bt], [gW, gb])
        loss = self.dt.type(data + reg)
        return (loss, gW, gb) if return_grads else loss

    def eval_loss(self, batch):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).eval_loss(X, y)

    def state(self):
        """name -> (rows, cols) array in slot order, named as tests.util names the loglinear model's state (b as one row)."""
        return {'W': self.Wt, 'b': self.bt.reshape(1, -1), 'accu.W': self.opt.accu[0], 'accu.b': self.opt.accu[1].reshape(1, -1),
                'delta.W': self.opt.delta[0], 'delta.b': self.opt.delta[1].reshape(1, -1)}


def clip_report(c):
    """clip_live's conditions over the three steps (step s trains batch s) and the evaluation of batch 1 after step 0, on the
    float64 twin -> counts per column kind and the smallest relative distance of a P or a Q_y from a clip bound."""
    tw = LlRefreshTwin(c, np.float64)
    lo, hi = O.clip_bounds(np.float64)
    B = c['B']
    kinds = dict(frozen=np.setdiff1d(np.arange(c['Ve']), c['refresh']), refreshed=np.asarray(c['refresh'], np.int64),
                 new=c['Ve'] + np.arange(c['N']))
    rep = dict(labels_clipped=[], margin=np.inf, finite=True, grad_nonzero=True)
    for k in kinds:
        rep[k + '_clipped'], rep[k + '_total'] = 0, 0

    def look(batch, count):
        f = tw.forward(batch)
        P, Q = f['P3'], f['Q']
        Qy = Q[np.arange(B), c['ext_of_slot'][c['y'][batch * B:(batch + 1) * B]]]
        for v in (P, Qy):
            for bound in (lo, hi):
                rep['margin'] = min(rep['margin'], float(np.abs(v - bound).min() / bound))
        if count:
            for k, cols in kinds.items():
                rep[k + '_clipped'] += int((P[:, :, cols] < lo).sum())
                rep[k + '_total'] += P[:, :, cols].size
            rep['labels_clipped'].append(int((Qy < lo).sum()))

    for s in range(STEPS):
        look(s, True)
        _, gW, gb = tw.train_step(s, return_grads=True)
        rep['finite'] = rep['finite'] and bool(np.isfinite(gW).all() and np.isfinite(gb).all())
        rep['grad_nonzero'] = rep['grad_nonzero'] and bool(np.abs(gW).max() > 0)
        if s == 0:
            look(1, False)
    return rep


def clip_ok(rep, B):
    return (rep['frozen_clipped'] > 0 and rep['refreshed_clipped'] > 0 and rep['new_clipped'] > 0 and
            all(0 < k < B for k in rep['labels_clipped']) and rep['margin'] > CLIP_MARGIN and rep['finite'] and
            rep['grad_nonzero'])


_made = {}


def make_case(name):
    """The case, generated once per process.  clip_live: the first seed of a fixed sequence whose float64 trajectory meets
    every condition of clip_report (case generation ENFORCES them; the CPU test asserts them again)."""
    if name in _made:
        return _made[name]
    seed = 4000 + sorted(CASES).index(name)
    if name != 'clip_live':
        c = _build(name, seed)
    else:
        for attempt in range(400):
            c = _build(name, seed + 100 * attempt)
            if clip_ok(clip_report(c), c['B']):
                c['attempt'] = attempt
                break
        else:
            raise RuntimeError('no clip_live input meets its conditions in 400 seeds')
    _made[name] = c
    return c
