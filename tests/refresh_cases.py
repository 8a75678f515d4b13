"""Inputs of the refresh tests (tests/test_refresh_inputs_cpu.py proves their structure, tests/test_gpu_refresh.py runs them)
and the oracle twin of a refresh step.

A refresh handle (sert_foldin_create_refresh, include/sert_hip_foldin.h) trains Nt = num_refresh + num_new SLOTS: slot
s < num_refresh is trained row refresh[s], slot num_refresh + e is new entity e = row V_e + e of the extended table.  y is a
slot, negatives are ids of the extended table.  The loss kernels foldin_nce_map<NCH> / foldin_nce_map_scalar<NPL>
(csrc/kernels_foldin.h) look every negative up in slot_of; everything behind them is the fold-in's, with N := Nt.

Every case has TWO steps with different negatives (step s trains batch s), V_e <= 320, B <= 48, z <= 3 and explicit
negatives.  The twin restates no maths: it builds Ext, calls VectorSpaceOracle.loss_and_grads and applies oracle.Adam to the
slot rows only.
"""
import numpy as np

from oracle import sert_oracle as O

STEPS = 2
SEED = 20241          # sampler seed of the device-drawn runs
CHUNK, SORT_TILE, SORT_MAX_BITS = 16, 2048, 11       # as tests/foldin_key_cases.py
BASE = dict(Vw=50, Ve=8, dw=12, de=8, n=3, z=3, B=16, lam=0.01, lr=0.01, num_new=0, w_none=False)

# name -> overrides of BASE and the structure the case exists for
CASES = {
    'order_and_edges': (dict(refresh=[7, 0, 3]),
                        'refresh is unsorted and names both ends of the table; negatives cover a refreshed row, a frozen row and '
                        'the instance\'s own positive; a refreshed row is the negative of several instances'),
    'mixed': (dict(refresh=[5, 1], num_new=3),
              'positives on refreshed and on new slots; negatives on V_e + e and on refreshed ids'),
    'all_rows': (dict(refresh='permutation'), 'every trained row is refreshed: no frozen pair, no sentinel run'),
    'ragged': (dict(refresh=[2, 6], num_new=1, B=20, w_none=True),
               'B = 20: the last workgroup of the vector kernel has 4 live rows; w = None at upload (the twin\'s ones)'),
    'wave_fixup': (dict(Ve=320, refresh='first256_shuffled', de=4, B=48),
                   'Nt = 256: the fix-up takes the wave form; most slots get no pair'),
    'sparse': (dict(Ve=40, refresh=[31, 4, 17, 22, 9, 38, 0, 12, 26, 35], num_new=2, z=2),
               'most slots are hit by no pair of either step (the lambda = 0 test: they keep their bits)'),
}
# one case per instance of the loss kernels: NCH = k at d_e = 64 k - 60, NPL = k at d_e = 64 (k - 1) + 2
for _k in range(1, 9):
    CASES['vector_k%d' % _k] = (dict(refresh=[6, 2], num_new=1, de=64 * _k - 60), 'foldin_nce_map<%d>' % _k)
    CASES['scalar_k%d' % _k] = (dict(refresh=[6, 2], num_new=1, de=64 * (_k - 1) + 2), 'foldin_nce_map_scalar<%d>' % _k)
INSTANCE_CASES = tuple('%s_k%d' % (f, k) for f in ('vector', 'scalar') for k in range(1, 9))
DEVICE_NEGATIVES_CASE, LAMBDA0_CASE = 'mixed', 'sparse'


def expected_plan(c):
    """FoldIn.plan() after a training step of the case: the fold-in's dispatch (csrc/host/api_foldin.inc, lazy_segsum.inc) with N := Nt."""
    de, Nt, total = c['de'], c['Nt'], c['B'] * (c['z'] + 1)
    bits = 1
    while (1 << bits) <= Nt:
        bits += 1
    if de % 4 == 0:
        k = -(-(de // 4) // 16)
        loss, vec, nch = 'vector', 4, next(n for n in (1, 2, 5, 8) if k <= n)
    else:
        k, loss, vec, nch = -(-de // 64), 'scalar', 1, 4
    return dict(loss=loss, k=k, train=True, sort_bits=bits, passes=-(-bits // SORT_MAX_BITS), vec=vec, nch=nch,
                col_passes=-(-(de // vec) // (16 * nch)), fixup='workgroup' if Nt < 256 else 'wave', tiles=-(-total // SORT_TILE))


_cache = {}


def make_case(name):
    """The case, built once per process; read-only.  'refresh' (num_refresh) int32, 'ext_of_slot' (Nt) int64, 'E0' (Nt, d_e) the
    slots' initial rows (trained rows of refresh, then 'New0'), 'y' (M) slots, 'neg' [step 0, step 1] (B, z) int64 ids of the
    extended table, 'w_upload' (None: the ones vector), 'w' what the twin weighs with, 'plan'."""
    if name in _cache:
        return _cache[name]
    over, structure = CASES[name]
    c = dict(BASE)
    c.update(over)
    c['name'], c['structure'] = name, structure
    rng = np.random.RandomState(3000 + list(CASES).index(name))
    Vw, Ve, dw, de, n, z, B, num_new = (c[k] for k in ('Vw', 'Ve', 'dw', 'de', 'n', 'z', 'B', 'num_new'))
    if isinstance(c['refresh'], str):
        c['refresh'] = rng.permutation(Ve if c['refresh'] == 'permutation' else 256)
    refresh = c['refresh'] = np.asarray(c['refresh'], dtype=np.int32)
    R = c['num_refresh'] = len(refresh)
    Nt = c['Nt'] = R + num_new
    ext = Ve + num_new
    c['ext_of_slot'] = np.concatenate([refresh.astype(np.int64), Ve + np.arange(num_new, dtype=np.int64)])
    M = c['M'] = STEPS * B + 5              # (a trailing M mod B = 5 instances are never visited)
    c['batches'] = (0, 1)
    c['Rw'] = O.glorot_uniform(rng, (Vw, dw))
    c['Re'] = O.glorot_uniform(rng, (Ve, de))
    c['W'] = O.glorot_uniform(rng, (dw, de))
    c['b'] = (0.1 * rng.randn(de)).astype(np.float32)
    c['New0'] = O.glorot_uniform(rng, (max(num_new, 1), de))[:num_new]
    c['E0'] = np.concatenate([c['Re'][refresh], c['New0']], axis=0)
    c['X'] = rng.randint(0, Vw, size=(M, n)).astype(np.int32)
    frozen = np.setdiff1d(np.arange(Ve), refresh)
    if name == 'sparse':
        y = rng.choice([0, 1, 2, 10], size=M)
        pool = np.concatenate([frozen[:6], [refresh[0], refresh[4]]])
        neg = [pool[rng.randint(0, len(pool), size=(B, z))].astype(np.int64) for _ in range(STEPS)]
    else:
        y = rng.randint(0, Nt, size=M)
        y[:Nt] = rng.permutation(Nt)[:M]    # (where B allows: every slot a positive in step 1)
        neg = [rng.randint(0, ext, size=(B, z)).astype(np.int64) for _ in range(STEPS)]
    y = c['y'] = y.astype(np.int32)
    if name == 'order_and_edges':
        for s in range(STEPS):
            own = c['ext_of_slot'][y[s * B:(s + 1) * B]]
            rows = np.arange(s, B, 3)
            neg[s][rows, 0] = own[rows]                      # the instance's own positive as its negative
            neg[s][1:6, 1] = refresh[0]                      # row 7 (the table's last, slot 0): hit by five instances
            neg[s][6:9, 2] = frozen[s]                       # a frozen row
            neg[s][9:11, 2] = refresh[1]                     # row 0 (the table's first)
    elif name == 'mixed':
        for s in range(STEPS):
            neg[s][0:4, 0] = Ve + np.arange(4) % num_new     # new rows
            neg[s][4:8, 1] = refresh[np.arange(4) % R]       # refreshed ids
            neg[s][8:10, 2] = frozen[s]
    c['neg'] = neg
    c['eval_neg'] = rng.randint(0, ext, size=(B, z)).astype(np.int64)
    c['w_upload'] = None if c['w_none'] else rng.uniform(0.5, 2.0, M).astype(np.float32)
    c['w'] = np.ones(M, np.float32) if c['w_upload'] is None else c['w_upload']
    c['plan'] = expected_plan(c)
    c['table'] = dict(map=True, num_refresh=R, num_new=num_new, rows=Nt)
    for a in list(c.values()) + neg:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _cache[name] = c
    return c


def slot_keys(c, s):
    """The (B (z + 1)) keys the loss kernel writes for step s, pair-major: the slot, or the sentinel Nt for a frozen row."""
    B = c['B']
    slot_of = np.full(c['Ve'] + c['num_new'], c['Nt'], dtype=np.int64)
    slot_of[c['ext_of_slot']] = np.arange(c['Nt'])
    keys = np.concatenate([c['y'][s * B:(s + 1) * B].astype(np.int64)[:, None], slot_of[c['neg'][s]]], axis=1)
    return keys.ravel()


class RefreshTwin(object):
    """The refresh on the CPU, on oracle objects alone.  dtype: float32 (the reference's) or float64.  ext_of_slot: another
    slot order than the case's (the CPU test's mutant)."""

    def __init__(self, c, dtype=np.float32, E0=None, lam=None, ext_of_slot=None):
        self.c, self.dt = c, np.dtype(dtype)
        self.lam = c['lam'] if lam is None else lam
        self.ext_of_slot = np.asarray(c['ext_of_slot'] if ext_of_slot is None else ext_of_slot, dtype=np.int64)
        if E0 is None:
            E0 = np.concatenate([c['Re'], c['New0']], axis=0)[self.ext_of_slot]
        self.E = np.array(E0, dtype=self.dt, copy=True)
        self.opt = O.Adam([self.E], lr=c['lr'])

    def ext(self):
        """Ext = concat(R_e, new rows) with every slot's current value written to its row."""
        c = self.c
        ext = np.concatenate([np.asarray(c['Re'], dtype=self.dt), np.zeros((c['num_new'], c['de']), dtype=self.dt)], axis=0)
        ext[self.ext_of_slot] = self.E
        return ext

    def _oracle(self, lam):
        c = self.c
        return O.VectorSpaceOracle(c['B'], c['n'], c['z'], c['Rw'], self.ext(), c['W'], c['b'], lam, dtype=self.dt)

    def _batch(self, i):
        c = self.c
        sl = slice(i * c['B'], (i + 1) * c['B'])
        return c['X'][sl], self.ext_of_slot[c['y'][sl]], c['w'][sl]

    def train_step(self, batch, neg):
        """-> the returned loss (before the update): data term + lambda / (2B) sum(E E) over the slots; then oracle.Adam on E."""
        c = self.c
        X, y, w = self._batch(batch)
        _, grads, _ = self._oracle(self.lam).loss_and_grads(X, y, w, neg)
        g = grads[0][self.ext_of_slot]                # data term of the slot rows + lambda / B * E, in slot order
        data, _, _ = self._oracle(0.0).loss_and_grads(X, y, w, neg)
        # VectorSpaceOracle.regularizer() of a model whose only non-zero regularised tensor is E (as tests/foldin_cases.py)
        zero = lambda *shape: np.zeros(shape, dtype=self.dt)
        reg = O.VectorSpaceOracle(c['B'], c['n'], c['z'], zero(1, c['dw']), self.E, zero(c['dw'], c['de']), zero(c['de']),
                                  self.lam, dtype=self.dt).regularizer()
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


_refs = {}


def case_reference(name, dtype, lam=None):
    """The twin's two steps of a case in `dtype` on the case's explicit negatives, computed once and shared: a list, per step,
    of dict(loss, E, m, v) -- copies of the twin's state after the step, read-only."""
    key = (name, np.dtype(dtype).name, lam)
    if key not in _refs:
        c = make_case(name)
        tw = RefreshTwin(c, dtype, lam=lam)
        out = []
        for s in range(STEPS):
            loss = tw.train_step(s, c['neg'][s])
            st = dict(loss=loss, E=tw.E.copy(), m=tw.m.copy(), v=tw.v.copy())
            for a in st.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out.append(st)
        _refs[key] = out
    return _refs[key]
