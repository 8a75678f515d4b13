"""Inputs of the loglinear word fold-in tests (tests/test_ll_wfold_inputs_cpu.py proves their structure,
tests/test_gpu_ll_wfold.py runs them) and the oracle twin of a loglinear word fold-in step.

A loglinear word fold-in learns Nw new word rows Nv (Nw, d) on top of a frozen loglinear model
(include/sert_hip_ll_wfold.h); new word v is token id Vw + v.  Every case is the smallest shape at which one mechanism of the
device path is live; `structure` names it, the property is forced by construction, and the CPU test proves it from X with
NumPy.  The twin restates no maths: loss and gradient come from oracle.sert_oracle.LogLinearOracle on the extended table
concat(R_w, Nv), the L2 term from a LogLinearOracle whose only non-zero tensor is Nv, the update from oracle.Adadelta.
"""
import numpy as np

from oracle import sert_oracle as O
from tests import ll_foldin_cases as LC
from tests import wfold_cases as WC

STEPS = 3
CHUNK = WC.CHUNK            # kWfoldChunk (csrc/wfold_index.h): the entries of one item of the inverted index
REG_MAX_VE = 1024           # the last V_e of the row kernel's register form (csrc/host/api_ll_wfold.inc: llw_forward)
BASE = dict(Vw=50, Nw=5, Ve=7, d=12, n=3, B=32, lam=0.01)
TRAILING = 5                # M = 3 B + 5: the trailing M mod B instances are never visited
CLIP_SCALE = LC.CLIP_SCALE  # clip_live: W times this
CLIP_MARGIN = LC.CLIP_MARGIN

# name -> (overrides of BASE, the structure the case exists for)
CASES = {
    'base': (dict(), 'a new word absent from batch 0; an instance with no new word; a new word twice in one window'),
    've8': (dict(Ve=8), 'V_e % 4 == 0: 16-byte rows in the row kernel and the float4 reduction'),
    've700': (dict(Ve=700), 'several entities per lane; V_e is a multiple of 4 and no multiple of 256'),
    've1024': (dict(Ve=1024), 'the last V_e of the register form'),
    've1025': (dict(Ve=1025), 'the first V_e of the streaming form, scalar rows'),
    've4100': (dict(Ve=4100), 'G = dZ W^T under the K >= 4096 rule of gemm_long_k: V_e // 1024 = 4 k ranges, the last one ragged; '
                              '16-byte rows'),
    'n1': (dict(n=1), 'window of one token'),
    'n32': (dict(n=32), 'the window limit'),
    'all_new': (dict(), 'every token is a new word: no frozen word, an empty frozen table'),
    'one_word': (dict(Nw=1), 'a single new word'),
    'many_words': (dict(Nw=300), 'most new rows have no occurrence in a batch; Zn and G are GEMMs over 300 rows'),
    'chunk65': (dict(), 'new word 0 in exactly 64 positions of batch 0 (one item) and 65 of batch 1 (two chunks, a second level)'),
    'three_levels': (dict(B=144, n=32), 'new word 0 in 4097 > 64 * 64 positions of batch 0: a third level'),
    'odd_d': (dict(d=7), 'word dimension not a multiple of 4: scalar gathers, GEMMs off their vector paths'),
    'd300': (dict(d=300), 'the W3C dimension'),
    'batch_of_one': (dict(B=1), 'a single instance per batch'),
    'lam0': (dict(lam=0.0), 'no L2 term'),
    'clip_live': (dict(), 'W scaled by %g: frozen and new token probabilities below 1e-7, labels with Q_y below 1e-7 and labels '
                          'above it, nothing within %g of a clip bound' % (CLIP_SCALE, CLIP_MARGIN)),
}


def _place(rng, Xb, word, count):
    """Exactly `count` positions of the batch slice Xb (a view) hold `word`."""
    flat = Xb.reshape(-1)
    flat[flat == word] = 0
    flat[rng.choice(flat.size, count, replace=False)] = word
    assert int((Xb == word).sum()) == count


def _build(name, seed):
    over, structure = CASES[name]
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
    rng = np.random.RandomState(seed)
    Vw, Nw, Ve, d, n, B = (c[k] for k in ('Vw', 'Nw', 'Ve', 'd', 'n', 'B'))
    M = 3 * B + TRAILING
    c['M'], c['batches'] = M, M // B
    c['Rw'] = O.glorot_uniform(rng, (Vw, d))
    c['W'] = O.glorot_uniform(rng, (d, Ve))
    c['b'] = (0.1 * rng.randn(Ve)).astype(np.float32)
    # the new rows at the scale of the TRAINED table (Glorot's bound of its fan), as sert_amd.foldin.new_word_rows draws them
    bound = np.sqrt(6.0 / (Vw + d))
    c['Nv0'] = rng.uniform(-bound, bound, size=(Nw, d)).astype(np.float32)
    X = rng.randint(0, Vw + Nw, size=(M, n)).astype(np.int32)
    if name == 'base':
        first = X[:B]
        first[first == Vw + Nw - 1] = 0                 # the last new word is absent from batch 0
        X[0] = (Vw, 3, Vw)                              # a new word twice in one window ...
        X[1] = (Vw + 1, Vw + 2, 4)                      # ... a window with two different new words ...
        X[2] = (1, 2, 3)                                # ... an instance with none
    elif name == 'all_new':
        X = rng.randint(Vw, Vw + Nw, size=(M, n)).astype(np.int32)
    elif name == 'one_word':
        X[::7, 0] = Vw                                  # the word in every batch
    elif name == 'many_words':
        X = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
        X[:, 1] = Vw + rng.randint(0, Nw, size=M)       # one new word per window: at most B of the 300 occur in a batch
    elif name == 'chunk65':
        X[X == Vw] = 1
        _place(rng, X[:B], Vw, CHUNK)
        _place(rng, X[B:2 * B], Vw, CHUNK + 1)
    elif name == 'three_levels':
        X[X == Vw] = 1
        _place(rng, X[:B], Vw, CHUNK * CHUNK + 1)
    c['X'] = X
    c['y'] = rng.randint(0, Ve, size=M).astype(np.int32)
    c['w'] = rng.uniform(0.5, 2.0, M).astype(np.float32)
    if name == 'clip_live':
        c['W'] = (c['W'] * np.float32(CLIP_SCALE)).astype(np.float32)
    return c


# (M, n) int32: the new word of every position, -1 for a trained word; and the inverted index the contract states for one
# batch, from its constants alone -- the word fold-in's rule is this one's (csrc/wfold_index.h is shared)
new_tokens = WC.new_tokens
index_of_batch = WC.index_of_batch


def expected_plan(c, batch):
    """What sert_debug_ll_wfold_plan must report after a training step on `batch`, from the case's constants."""
    _, levels = index_of_batch(c, batch)
    vec = c['Ve'] % 4 == 0
    return dict(form='reg' if c['Ve'] <= REG_MAX_VE else 'stream', vec=vec, train=True, levels=len(levels),
                items=[len(items) for items in levels], segsum=('rows64' if vec else 'scalar') if levels else 'none')


def clip_report(c):
    """clip_live's conditions over the three steps (step s trains batch s) and the evaluation of batch 1 after step 0, on
    the float64 twin -> dict of counts and the smallest relative distance of a P or a Q_y from a clip bound."""
    tw = LlWordFoldInTwin(c, np.float64)
    lo, hi = O.clip_bounds(np.float64)
    B, Vw = c['B'], c['Vw']
    rep = dict(frozen_clipped=0, new_clipped=0, frozen_total=0, new_total=0, labels_clipped=[], margin=np.inf, finite=True,
               grad_nonzero=True)

    def look(batch, count):
        f = tw.forward(batch)
        P, Q = f['P3'], f['Q']
        new = c['X'][batch * B:(batch + 1) * B] >= Vw
        Qy = Q[np.arange(B), c['y'][batch * B:(batch + 1) * B]]
        for v in (P, Qy):
            for bound in (lo, hi):
                rep['margin'] = min(rep['margin'], float(np.abs(v - bound).min() / bound))
        if count:
            rep['frozen_clipped'] += int((P[~new] < lo).sum())
            rep['new_clipped'] += int((P[new] < lo).sum())
            rep['frozen_total'] += P[~new].size
            rep['new_total'] += P[new].size
            rep['labels_clipped'].append(int((Qy < lo).sum()))

    for s in range(STEPS):
        look(s, True)
        _, g = tw.train_step(s, return_grads=True)
        rep['finite'] = rep['finite'] and bool(np.isfinite(g).all())
        rep['grad_nonzero'] = rep['grad_nonzero'] and bool(np.abs(g).max() > 0)
        if s == 0:
            look(1, False)
    return rep


def clip_ok(rep, B):
    return (rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0 and all(0 < k < B for k in rep['labels_clipped']) and
            rep['margin'] > CLIP_MARGIN and rep['finite'] and rep['grad_nonzero'])


_made = {}
# the seeds were dealt in sorted order; a later case takes the next one, so that no earlier case's input moves
_SEED_ORDER = sorted(set(CASES) - {'ve4100'}) + ['ve4100']


def make_case(name):
    """The case, generated once per process.  clip_live: the first seed of a fixed sequence whose float64 trajectory meets
    every condition of clip_report (case generation ENFORCES them; the CPU test asserts them again)."""
    if name in _made:
        return _made[name]
    seed = 3000 + _SEED_ORDER.index(name)
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


class LlWordFoldInTwin(object):
    """The loglinear word fold-in on the CPU, on oracle objects alone.  dtype: float32 (the reference's) or float64."""

    def __init__(self, c, dtype=np.float32, Nv0=None):
        self.c, self.dt = c, np.dtype(dtype)
        self.Nv = np.array(c['Nv0'] if Nv0 is None else Nv0, dtype=self.dt, copy=True)
        self.opt = O.Adadelta([self.Nv], lr=1.0, rho=0.95, eps=1e-6)

    def _oracle(self, lam):
        c = self.c
        ext = np.concatenate([np.asarray(c['Rw'], dtype=self.dt), self.Nv], axis=0)
        return O.LogLinearOracle(c['B'], c['n'], ext, c['W'], c['b'], lam, dtype=self.dt)

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], c['y'][sl].astype(np.int64), c['w'][sl]

    def forward(self, batch):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).forward(X, y)

    def loss_and_grads(self, batch):
        """-> (data loss, gradient of Nv with lambda / B * Nv, the oracle's forward and backward record)."""
        c = self.c
        X, y, w = self._batch(batch)
        _, grads, f = self._oracle(c['lam']).loss_and_grads(X, y, w)
        data, _, _ = self._oracle(0.0).loss_and_grads(X, y, w)
        return data, np.array(grads[0][c['Vw']:], dtype=self.dt), f

    def train_step(self, batch, return_grads=False):
        """-> the returned loss (before the update): data term + lambda / (2B) sum(Nv Nv); then oracle.Adadelta on Nv alone."""
        c = self.c
        data, g, _ = self.loss_and_grads(batch)
        # LogLinearOracle.regularizer() of a model whose only non-zero tensor is Nv
        zero = lambda *shape: np.zeros(shape, dtype=self.dt)
        reg = O.LogLinearOracle(c['B'], c['n'], self.Nv, zero(c['d'], 1), zero(1), c['lam'], dtype=self.dt).regularizer()
        self.opt.update([self.Nv], [g])
        loss = self.dt.type(data + reg)
        return (loss, g) if return_grads else loss

    def eval_loss(self, batch):
        X, y, _ = self._batch(batch)
        return self._oracle(0.0).eval_loss(X, y)

    def state(self):
        """name -> (rows, cols) array, named as tests.util names the loglinear model's word table and its moments."""
        return {'R_w': self.Nv, 'accu.R_w': self.opt.accu[0], 'delta.R_w': self.opt.delta[0]}
