"""Inputs of the loglinear fold-in tests (tests/test_ll_foldin_inputs_cpu.py proves their structure,
tests/test_gpu_ll_foldin.py runs them) and the oracle twin of a loglinear fold-in step.

A loglinear fold-in learns N new columns Wn (d, N) and biases bn (N) on top of a frozen loglinear model
(include/sert_hip_ll_foldin.h).  Every case is the smallest shape at which one mechanism of the device path is live;
`structure` names it and the CPU test proves it with NumPy and the twin.  The twin restates no maths: loss and gradient come
from oracle.sert_oracle.LogLinearOracle on the extended tensors concat(W, Wn) / concat(b, bn), the L2 term from a
LogLinearOracle whose only non-zero tensor is Wn, the update from oracle.Adadelta.
"""
import numpy as np

from oracle import sert_oracle as O

STEPS = 3
BASE = dict(Vw=50, Ve=7, N=5, d=12, n=3, B=32, lam=0.01)
TRAILING = 5                # M = 3 B + 5: the trailing M mod B instances are never visited
CLIP_SCALE = 24.0           # clip_live: W and the initial Wn times this
CLIP_MARGIN = 1e-3          # clip_live: no P and no Q_y within this (relative) of a clip bound, on the float64 twin

# name -> (overrides of BASE, the structure the case exists for)
CASES = {
    'base': (dict(), 'a new entity has no instance in batch 0'),
    'wide_ve': (dict(Ve=700), 'several frozen entities per lane; V_e is no multiple of the workgroup width 256'),
    'one_new': (dict(N=1), 'a single new column'),
    'many_new': (dict(N=300), 'more new columns than one workgroup is wide'),
    'n1': (dict(n=1), 'window of one token: the NMAX = 8 bucket at its smallest'),
    'n9': (dict(n=9), 'the NMAX = 16 bucket, just above 8'),
    'n32': (dict(n=32), 'the NMAX = 32 bucket at the limit'),
    'odd_d': (dict(d=7), 'word dimension not a multiple of 4: scalar gathers, GEMMs off their vector paths'),
    'd300': (dict(d=300), 'the W3C dimension'),
    'repeated_word': (dict(), 'a window of one word n times; a word occurring in more than 64 tokens of one batch'),
    'batch_of_one': (dict(B=1), 'a single instance per batch'),
    'lam0': (dict(lam=0.0), 'no L2 term'),
    'clip_live': (dict(), 'W and the initial Wn scaled by %g: frozen and new token probabilities below 1e-7, labels with Q_y '
                          'below 1e-7 and labels above it, nothing within %g of a clip bound' % (CLIP_SCALE, CLIP_MARGIN)),
}


def _build(name, seed):
    over, structure = CASES[name]
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
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
    y = rng.randint(0, N, size=M).astype(np.int32)
    if name == 'base':
        first = y[:B]
        first[first == N - 1] = 0     # the last new entity has no instance in batch 0
    if name == 'repeated_word':
        c['X'][:B, 0] = 3
        c['X'][:B, 1] = 3             # word 3: 64 tokens of batch 0 ...
        c['X'][0, :] = 3              # ... and a 65th: instance 0 is word 3, n times
    c['y'] = y
    c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
    if name == 'clip_live':
        c['W'] = (c['W'] * np.float32(CLIP_SCALE)).astype(np.float32)
        c['Wn0'] = (c['Wn0'] * np.float32(CLIP_SCALE)).astype(np.float32)
    return c


def clip_report(c):
    """clip_live's conditions over the three steps (step s trains batch s) and the evaluation of batch 1 after step 0, on
    the float64 twin -> dict of counts and the smallest relative distance of a P or a Q_y from a clip bound."""
    tw = LlFoldInTwin(c, np.float64)
    lo, hi = O.clip_bounds(np.float64)
    Ve, B = c['Ve'], c['B']
    rep = dict(frozen_clipped=0, new_clipped=0, frozen_total=0, new_total=0, labels_clipped=[], margin=np.inf, finite=True,
               grad_nonzero=True)

    def look(batch, count):
        f = tw.forward(batch)
        P, Q = f['P3'], f['Q']
        Qy = Q[np.arange(B), Ve + c['y'][batch * B:(batch + 1) * B]]
        for v in (P, Qy):
            for bound in (lo, hi):
                rep['margin'] = min(rep['margin'], float(np.abs(v - bound).min() / bound))
        if count:
            rep['frozen_clipped'] += int((P[:, :, :Ve] < lo).sum())
            rep['new_clipped'] += int((P[:, :, Ve:] < lo).sum())
            rep['frozen_total'] += P[:, :, :Ve].size
            rep['new_total'] += P[:, :, Ve:].size
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
    return (rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0 and all(0 < k < B for k in rep['labels_clipped']) and
            rep['margin'] > CLIP_MARGIN and rep['finite'] and rep['grad_nonzero'])


_made = {}


def make_case(name):
    """The case, generated once per process.  clip_live: the first seed of a fixed sequence whose float64 trajectory meets
    every condition of clip_report (case generation ENFORCES them; the CPU test asserts them again)."""
    if name in _made:
        return _made[name]
    seed = 2000 + sorted(CASES).index(name)
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


class LlFoldInTwin(object):
    """The loglinear fold-in on the CPU, on oracle objects alone.  dtype: float32 (the reference's) or float64."""

    def __init__(self, c, dtype=np.float32):
        self.c, self.dt = c, np.dtype(dtype)
        self.Wn = np.array(c['Wn0'], dtype=self.dt, copy=True)
        self.bn = np.array(c['bn0'], dtype=self.dt, copy=True)
        self.opt = O.Adadelta([self.Wn, self.bn], lr=1.0, rho=0.95, eps=1e-6)

    def _oracle(self, lam):
        c = self.c
        Wx = np.concatenate([np.asarray(c['W'], dtype=self.dt), self.Wn], axis=1)
        bx = np.concatenate([np.asarray(c['b'], dtype=self.dt), self.bn])
        return O.LogLinearOracle(c['B'], c['n'], c['Rw'], Wx, bx, lam, dtype=self.dt)

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], c['Ve'] + c['y'][sl].astype(np.int64), c['w'][sl]

    def forward(self, batch):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).forward(X, y)

    def train_step(self, batch, return_grads=False):
        """-> the returned loss (before the update): data term + lambda / (2B) sum(Wn Wn); then oracle.Adadelta on [Wn, bn]."""
        c = self.c
        X, y, w = self._batch(batch)
        _, grads, _ = self._oracle(c['lam']).loss_and_grads(X, y, w)
        gW, gb = grads[1][:, c['Ve']:], grads[2][c['Ve']:]       # gW includes lambda / B * Wn; the bias is not regularised
        data, _, _ = self._oracle(0.0).loss_and_grads(X, y, w)
        # LogLinearOracle.regularizer() of a model whose only non-zero tensor is Wn
        zero = lambda *shape: np.zeros(shape, dtype=self.dt)
        reg = O.LogLinearOracle(c['B'], c['n'], zero(1, c['d']), self.Wn, zero(c['N']), c['lam'], dtype=self.dt).regularizer()
        gW, gb = np.array(gW, dtype=self.dt), np.array(gb, dtype=self.dt)
        self.opt.update([self.Wn, self.bn], [gW, gb])
        loss = self.dt.type(data + reg)
        return (loss, gW, gb) if return_grads else loss

    def eval_loss(self, batch):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).eval_loss(X, y)

    def state(self):
        """name -> (rows, cols) array, named as tests.util names the loglinear model's state (b as one row)."""
        return {'W': self.Wn, 'b': self.bn.reshape(1, -1), 'accu.W': self.opt.accu[0], 'accu.b': self.opt.accu[1].reshape(1, -1),
                'delta.W': self.opt.delta[0], 'delta.b': self.opt.delta[1].reshape(1, -1)}
