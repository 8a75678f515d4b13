"""Inputs of the word fold-in tests (tests/test_wfold_inputs_cpu.py proves their structure, tests/test_gpu_wfold.py runs
them) and the oracle twin of a word fold-in step.

A word fold-in learns Nw new word rows Nv on top of a frozen vectorspace model (include/sert_hip_wfold.h); new word v is
token id Vw + v.  Every case is the smallest shape at which one mechanism of the device path is live; `structure` names it,
the property is forced by construction, and the CPU test proves it from X with NumPy.  The twin restates no maths: loss,
gradient and update come from oracle.sert_oracle.VectorSpaceOracle / Adam on the extended table concat(R_w, Nv).
"""
import numpy as np

from oracle import sert_oracle as O

STEPS = 3
CHUNK = 64            # kWfoldChunk (csrc/wfold_index.h): the entries of one item of the inverted index
BASE = dict(Vw=50, Nw=5, Ve=7, dw=12, de=8, n=3, z=4, B=32, batches=3, lam=0.01, lr=0.01)

# name -> (overrides of BASE, the structure the case exists for)
CASES = {
    'base': (dict(), 'tokens over [0, Vw + Nw); a new word at least twice in one batch; a window with two different new '
                     'words; windows with none; one new word absent from batch 0'),
    'ragged': (dict(B=24), 'B is not a multiple of 16: a ragged last workgroup of the loss kernel'),
    'wide': (dict(de=128), 'two float4 column chunks per lane of the loss kernel; 32 float4 columns per row of the reduction'),
    'odd_de': (dict(de=6), 'd_e is not a multiple of 4: the scalar instances of the project and loss kernels and of the '
                           'reduction'),
    'odd_dw': (dict(dw=10), 'd_w is not a multiple of 4 in the upload\'s gather and in both GEMMs'),
    'many_cands': (dict(z=20), 'z + 1 > 16 candidates per instance'),
    'twice_in_window': (dict(), 'one new word at every position of some windows: multiplicity n'),
    'empty_batch': (dict(), 'batch 1 holds no new word: the data gradient is exactly zero, the rows still move by L2 and '
                            'their moments'),
    'all_new': (dict(), 'every token is a new word: A0 = b'),
    'heavy': (dict(Nw=1, B=200), 'one new word in every window: more occurrences than one chunk, a second level'),
    'heavy3': (dict(Nw=1, B=1366), 'one new word at every position of B = 1366 windows: 4098 > 64 * 64 occurrences, the '
                                   'smallest batch at n = 3 whose index has a third level'),
    'many_words': (dict(Nw=300, B=64), 'most new rows have no occurrence in a batch; P and G are GEMMs over 300 rows'),
}
# sampler seed of the device-drawn runs
SEED = 20250


def make_case(name):
    over, structure = CASES[name]
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
    rng = np.random.RandomState(2000 + sorted(CASES).index(name))
    Vw, Nw, Ve, dw, de, n, z, B = (c[k] for k in ('Vw', 'Nw', 'Ve', 'dw', 'de', 'n', 'z', 'B'))
    M = B * c['batches'] + 5          # (a trailing M mod B = 5 instances are never visited)
    c['M'] = M
    c['Rw'] = O.glorot_uniform(rng, (Vw, dw))
    c['Re'] = O.glorot_uniform(rng, (Ve, de))
    c['W'] = O.glorot_uniform(rng, (dw, de))
    c['b'] = (0.1 * rng.randn(de)).astype(np.float32)
    c['Nv0'] = O.glorot_uniform(rng, (Nw, dw))
    X = rng.randint(0, Vw + Nw, size=(M, n)).astype(np.int32)
    if name == 'base':
        first = X[:B]
        first[first == Vw + Nw - 1] = 0                 # the last new word is absent from batch 0
        X[0] = (Vw, 3, Vw)                              # a new word twice in one batch (here: in one window) ...
        X[1] = (Vw + 1, Vw + 2, 4)                      # ... a window with two different new words ...
        X[2] = (1, 2, 3)                                # ... a window with none
    elif name == 'twice_in_window':
        X[np.arange(0, M, 4)] = Vw + 2                  # every position of every fourth window
    elif name == 'empty_batch':
        mid = X[B:2 * B]
        mid[mid >= Vw] -= Vw                            # batch 1: trained words only
    elif name == 'all_new':
        X = rng.randint(Vw, Vw + Nw, size=(M, n)).astype(np.int32)
    elif name == 'heavy':
        X = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
        X[np.arange(M), rng.randint(0, n, size=M)] = Vw  # the word once in every window ...
        X[np.arange(0, M, 2), 0] = Vw                   # ... and a second time in about every other one
    elif name == 'heavy3':
        X[...] = Vw
    elif name == 'many_words':
        X = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
        X[:, 1] = Vw + rng.randint(0, Nw, size=M)       # one new word per window: at most B of the 300 occur in a batch
    c['X'] = X
    c['y'] = rng.randint(0, Ve, size=M).astype(np.int32)
    c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
    # explicit negatives of step s (the step trains batch s)
    c['neg'] = rng.randint(0, Ve, size=(STEPS, B, z)).astype(np.int64)
    c['eval_neg'] = rng.randint(0, Ve, size=(B, z)).astype(np.int64)
    return c


def new_tokens(c):
    """(M, n) int32: the new word of every position, -1 for a trained word."""
    return np.where(c['X'] >= c['Vw'], c['X'] - c['Vw'], -1).astype(np.int32)


def index_of_batch(c, batch):
    """The inverted index the contract states for one batch, from its constants alone: per new word of the batch, ascending,
    the batch rows of its occurrences ascending by (row, position); lists of more than CHUNK entries cut into chunks.
    -> (rows, levels): rows the level-0 entries; levels a list of item lists [(begin, end, dst)], dst = word or -(p + 1)."""
    B = c['B']
    tok = new_tokens(c)[batch * B:(batch + 1) * B]
    rows, segs = [], []
    for v in sorted(set(tok[tok >= 0].tolist())):
        r, _ = np.nonzero(tok == v)                     # (row-major: ascending by (row, position))
        segs.append((len(rows), len(rows) + len(r), v))
        rows += r.tolist()
    levels = []
    while segs:
        items, nxt, parts = [], [], 0
        for b, e, v in segs:
            if e - b <= CHUNK:
                items.append((b, e, v))
            else:
                first = parts
                for s in range(b, e, CHUNK):
                    items.append((s, min(e, s + CHUNK), -(parts + 1)))
                    parts += 1
                nxt.append((first, parts, v))
        levels.append(items)
        segs = nxt
    return np.asarray(rows, np.int32), levels


class WordFoldInTwin(object):
    """The word fold-in on the CPU, on oracle objects alone.  dtype: float32 (the reference's) or float64."""

    def __init__(self, c, dtype=np.float32, Nv0=None):
        self.c, self.dt = c, np.dtype(dtype)
        self.Nv = np.array(c['Nv0'] if Nv0 is None else Nv0, dtype=self.dt, copy=True)
        self.opt = O.Adam([self.Nv], lr=c['lr'])

    def _oracle(self, lam):
        c = self.c
        ext = np.concatenate([np.asarray(c['Rw'], dtype=self.dt), self.Nv], axis=0)
        return O.VectorSpaceOracle(c['B'], c['n'], c['z'], ext, c['Re'], c['W'], c['b'], lam, dtype=self.dt)

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], c['y'][sl], c['w'][sl]

    def train_step(self, batch, neg):
        """-> the returned loss (before the update): data term + lambda / (2B) sum(Nv Nv); then oracle.Adam on Nv alone."""
        c = self.c
        X, y, w = self._batch(batch)
        _, grads, _ = self._oracle(c['lam']).loss_and_grads(X, y, w, neg)
        g = grads[1][c['Vw']:]                       # data term of the new rows + lambda / B * Nv
        data, _, _ = self._oracle(0.0).loss_and_grads(X, y, w, neg)
        # VectorSpaceOracle.regularizer() of a model whose only non-zero regularised tensor is Nv
        zero = lambda *shape: np.zeros(shape, dtype=self.dt)
        reg = O.VectorSpaceOracle(c['B'], c['n'], c['z'], self.Nv, zero(1, c['de']), zero(c['dw'], c['de']), zero(c['de']),
                                  c['lam'], dtype=self.dt).regularizer()
        self.opt.update([self.Nv], [np.asarray(g, dtype=self.dt)])
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
