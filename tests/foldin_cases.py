"""Inputs of the fold-in tests (tests/test_foldin_inputs_cpu.py proves their structure, tests/test_gpu_foldin.py runs
them) and the oracle twin of a fold-in step.

A fold-in learns N new entity rows E on top of a frozen vectorspace model (include/sert_hip_foldin.h).  Every case is the
smallest shape at which one mechanism of the device path is live; `structure` names it and the CPU test proves it from
y / neg with NumPy.  The twin restates no maths: loss, gradient and update come from
oracle.sert_oracle.VectorSpaceOracle / Adam on the extended table concat(R_e, E).
"""
import numpy as np

from oracle import sert_oracle as O

STEPS = 3
BASE = dict(Vw=50, Ve=7, N=5, dw=12, de=8, n=3, z=4, B=32, batches=3, lam=0.01, lr=0.01)

# name -> (overrides of BASE, the structure the case exists for)
CASES = {
    'base': (dict(), 'explicit negatives mix frozen and new rows; a new row is hit by >= 2 pairs in one batch; a new '
                     'entity has no instance in a batch'),
    'ragged': (dict(B=24), 'B is not a multiple of 16: a ragged last workgroup of the loss kernel'),
    'wide': (dict(de=128), 'two float4 column chunks per lane'),
    'odd_de': (dict(de=6), 'd_e is not a multiple of 4: the scalar loss kernel and the scalar reduction'),
    'many_cands': (dict(z=20), 'z + 1 > 16 candidates per instance'),
    'one_entity': (dict(N=1, B=100), 'every positive and about B z / (V_e + 1) negatives land on one row: its run spans '
                                     'many 16-pair chunks and the sentinel run behind it starts off a chunk boundary'),
    'all_frozen': (dict(), 'every negative is a frozen row: only positives reach the new rows, the rest is one sentinel run'),
    'all_new': (dict(), 'every negative is a new row: no sentinel run at all'),
    'two_digits': (dict(N=2100, de=8, B=64), 'N + 1 > 2048 keys: a second sort pass; most new rows get no pair'),
    'target_as_negative': (dict(), 'a negative of a row equals its own target: both roles add into one row'),
}
# sampler seed of the device-drawn runs
SEED = 20240


def make_case(name):
    over, structure = CASES[name]
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
    rng = np.random.RandomState(1000 + sorted(CASES).index(name))
    Vw, Ve, N, dw, de, n, z, B = (c[k] for k in ('Vw', 'Ve', 'N', 'dw', 'de', 'n', 'z', 'B'))
    M = B * c['batches'] + 5          # (a trailing M mod B = 5 instances are never visited)
    c['M'] = M
    c['Rw'] = O.glorot_uniform(rng, (Vw, dw))
    c['Re'] = O.glorot_uniform(rng, (Ve, de))
    c['W'] = O.glorot_uniform(rng, (dw, de))
    c['b'] = (0.1 * rng.randn(de)).astype(np.float32)
    c['E0'] = O.glorot_uniform(rng, (N, de))
    c['X'] = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
    y = rng.randint(0, N, size=M).astype(np.int32)
    if name == 'base':
        first = y[:B]
        first[first == N - 1] = 0     # the last new entity has no instance in batch 0
    c['y'] = y
    c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
    lo, hi = 0, Ve + N
    if name == 'all_frozen':
        hi = Ve
    elif name == 'all_new':
        lo = Ve
    # explicit negatives of step s (the step trains batch s)
    neg = rng.randint(lo, hi, size=(STEPS, B, z)).astype(np.int64)
    if name == 'target_as_negative':
        for s in range(STEPS):
            rows = np.arange(0, B, 3)
            neg[s, rows, 0] = Ve + y[s * B + rows]
    c['neg'] = neg
    c['eval_neg'] = rng.randint(0, Ve + N, size=(B, z)).astype(np.int64)
    return c


def keys_of_step(c, s):
    """The (B (1 + z)) keys the loss kernel writes for step s, pair-major: new row index, or the sentinel N for a frozen row."""
    B, Ve, N = c['B'], c['Ve'], c['N']
    cand = np.concatenate([(Ve + c['y'][s * B:(s + 1) * B].astype(np.int64))[:, None], c['neg'][s]], axis=1).ravel()
    return np.where(cand >= Ve, cand - Ve, N)


class FoldInTwin(object):
    """The fold-in on the CPU, on oracle objects alone.  dtype: float32 (the reference's) or float64."""

    def __init__(self, c, dtype=np.float32, E0=None):
        self.c, self.dt = c, np.dtype(dtype)
        self.E = np.array(c['E0'] if E0 is None else E0, dtype=self.dt, copy=True)
        self.opt = O.Adam([self.E], lr=c['lr'])

    def _oracle(self, lam):
        c = self.c
        ext = np.concatenate([np.asarray(c['Re'], dtype=self.dt), self.E], axis=0)
        return O.VectorSpaceOracle(c['B'], c['n'], c['z'], c['Rw'], ext, c['W'], c['b'], lam, dtype=self.dt)

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], c['Ve'] + c['y'][sl].astype(np.int64), c['w'][sl]

    def train_step(self, batch, neg):
        """-> the returned loss (before the update): data term + lambda / (2B) sum(E E); then oracle.Adam on E alone."""
        c = self.c
        X, y, w = self._batch(batch)
        _, grads, _ = self._oracle(c['lam']).loss_and_grads(X, y, w, neg)
        g = grads[0][c['Ve']:]                       # data term of the new rows + lambda / B * E
        data, _, _ = self._oracle(0.0).loss_and_grads(X, y, w, neg)
        # VectorSpaceOracle.regularizer() of a model whose only non-zero regularised tensor is E
        zero = lambda *shape: np.zeros(shape, dtype=self.dt)
        reg = O.VectorSpaceOracle(c['B'], c['n'], c['z'], zero(1, c['dw']), self.E, zero(c['dw'], c['de']), zero(c['de']),
                                  c['lam'], dtype=self.dt).regularizer()
        self.opt.update([self.E], [np.asarray(g, dtype=self.dt)])
        return self.dt.type(data + reg)

    def eval_loss(self, batch, neg):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).eval_loss(X, y, neg)

    @property
    def m(self):
        return self.opt.m[0]

    @property
    def v(self):
        return self.opt.v[0]
