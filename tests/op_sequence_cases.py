"""Sequences of API calls in which every step-schedule mechanism is live -- shared by the CPU proof of the inputs
(test_op_sequences_cpu.py) and the GPU test (test_gpu_op_sequences.py).

A training step leaves state for the next call: word-table rows that are behind (the lazy update), a forward + backward that ran
ahead for the announced batch, the next step's negatives, entity keys sorted or partitioned early, an entity-table update deferred
past the tail with its sums of squares handed over, a tail waiting for the next gather.  Every public entry point between two
steps has to leave that state right.  The suite tests each mechanism at its kernels' shape edges in straight runs of train_batch;
here the calls are INTERLEAVED, at the smallest shapes at which each mechanism runs (CASES), and every call is replayed on the
NumPy oracle in float32 and in float64 (replay / case_reference).

One sequence is a list of ops (dicts, 'op' one of TRAIN_OPS or of other_kinds(case)), built BY CONSTRUCTION from the case's seed
(build_ops): every other kind stands once behind a training step that announced the following one, once in front of a training
step that was announced before the op, and once between two steps nobody announced (op_positions; the CPU test asserts the
coverage from the list alone).  apply_op applies an op to an engine, Replay.apply to the oracle.

How far the float32 replay is from the float64 one, measured by the CPU test over the whole sequences -- worst loss and worst
prediction (relative; half of 1e-5 is asserted), worst tensor read or final entry globally as a fraction of TENSOR_TOL and row-wise
as a fraction of the smaller of its two row bounds (float32 oracle / float64 oracle; under 0.5 is asserted), the smallest factor
between a clipped probability and a clip bound (loglinear; above 2 is asserted), and the seconds both replays take together:
    case            ops  steps  losses   predict  tensors  rows   clip margin  seconds
    fs_lazy         115    80   1.2e-07  4.8e-07   0.14    0.30       -          15
    ll_lazy         112    80   2.1e-07  2.1e-07   0.01    0.01    1.1e+04       20
    ll_stream       103    71   2.5e-07  3.0e-07   0.01    0.01      177          1
    vs_b32768       101    66   8.1e-08  3.1e-07   0.14    0.14       -          12
    vs_lazy         122    85   1.3e-07  3.5e-07   0.13    0.30       -          15
    vs_lazy_big_re  111    76   1.1e-07  6.6e-07   0.13    0.21       -          28
    vs_scalar       112    75   1.2e-07  2.9e-07   0.13    0.13       -         0.1
    vs_sorted       112    75   1.4e-07  3.3e-07   0.15    0.16       -           3
(The 0.13 of TENSOR_TOL every Adam case shows is the second moments': float32's 1 - 0.999 is 1.3e-5 off.)
"""
import time

import numpy as np

from oracle import philox
from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import util as U

LAM, SEED = 0.01, 77          # regularisation; the engines' sampler seed
NB, NV = 6, 2                 # training / validation batches of every case
LOSS_TOL = 1e-5               # the project's bound for a loss and for predict (tests/test_gpu_parity.py)
KEEP_LOSS_TOL = 2e-6          # keep_grads = 1 against the product engine (tests/test_gpu_lazy_dense.py)
LAZY_MAX_TOUCHED = 0.35       # csrc/host/optimizer_and_loss.inc: a batch above it takes the dense launch without a hint
LAZY_MIN_ELEMENTS = 1 << 22   # ... and so does a table below this size
SORT_FREE_MAX_ENTITIES = 2048

# kind: 'vs' (NCE), 'fs' (full softmax), 'll' (loglinear); lazy: the word table takes the lazy update; short: fewer ops (big replays).
# What must be live in each case is asserted by the GPU test (check_liveness).
CASES = {
    'vs_lazy': dict(kind='vs', B=64, n=4, z=4, Vw=33000, dw=128, Ve=40, de=16, lazy=True),
    'vs_sorted': dict(kind='vs', B=1024, n=3, z=10, Vw=2000, dw=32, Ve=2049, de=64, lazy=False),
    # (lr: nearly every row of both tables sees the regulariser's gradient alone, and what float32 makes of Adam's constants moves
    #  such a row by 1.4e-6 of its norm per step at lr = 1e-3 -- the float32 REPLAY was 4.8e-5 from the float64 one row-wise after
    #  35 steps, the whole float64 bound.  A quarter of the step size, a quarter of that.)
    'vs_lazy_big_re': dict(kind='vs', B=256, n=4, z=4, Vw=33000, dw=128, Ve=33000, de=128, lazy=True, short=True, lr=2.5e-4),
    'vs_scalar': dict(kind='vs', B=33, n=3, z=2, Vw=300, dw=30, Ve=50, de=18, lazy=False),
    'vs_b32768': dict(kind='vs', B=32768, n=2, z=2, Vw=4000, dw=16, Ve=64, de=16, lazy=False, short=True),
    'll_lazy': dict(kind='ll', B=32, n=4, Vw=70000, dw=64, Ve=53, lazy=True),
    'll_stream': dict(kind='ll', B=4, n=4, Vw=200, dw=12, Ve=9001, lazy=False, labels='csr'),
    'fs_lazy': dict(kind='fs', B=64, n=4, Vw=33000, dw=128, Ve=37, de=16, lazy=True),
}
SEEDS = {name: 300 + k for k, name in enumerate(CASES)}

TRAIN_OPS = ('train', 'train_explicit', 'train_many')
HINTS = ('right', 'wrong', 'none', 'cleared')
# ops that go through invalidate_speculation (csrc/sert_hip.hip): a run-ahead, the negatives drawn ahead, the early keys, the
# predictions of the lazy table and the handed-over sums of squares do not survive them
INVALIDATING = ('eval', 'eval_many', 'set', 'set_step', 'reupload')


def other_kinds(case):
    """The non-training op kinds of a case.  negatives_of_step exists for the NCE model only."""
    kinds = ['eval', 'eval_many', 'get', 'set', 'set_step', 'set_eval_draws', 'reupload', 'predict', 'synchronize']
    if CASES[case]['kind'] == 'vs':
        kinds.append('negatives_of_step')
    return tuple(kinds)


def tensor_names(case):
    """The twelve (loglinear: nine) readable tensors of a case as U.oracle_state names them."""
    ll = CASES[case]['kind'] == 'll'
    moments = ('accu', 'delta') if ll else ('m', 'v')
    out = []
    for par in (U.LL_PARAMS if ll else U.VS_PARAMS):
        out += [par, moments[0] + '.' + par, moments[1] + '.' + par]
    return out


def tensor_id(name):
    moment, _, par = name.rpartition('.')
    return U.STATE_IDS[par][0 if not moment else 1 if moment in ('m', 'accu') else 2]


def set_forms(case):
    """In the order the builder takes them: rows of R_w behind an announced run (rows behind, predictions alive), b between two
    steps nobody announced, R_e behind an announced run again (sums of squares handed over)."""
    return ('rw_rows', 'b') if CASES[case]['kind'] == 'll' else ('rw_rows', 'b', 're')


# --------------------------------------------------------------------------- #
# problems
# --------------------------------------------------------------------------- #

_problems = {}


def case_problem(name):
    """The problem of a case, built once per process and read-only: the dict of util.make_vs_problem / make_ll_problem over
    NB + NV batches (the last NV are the validation split), plus `perm` (the row permutation of the reupload op), `avg` / `ids` /
    `queries` (the inputs of the predict op), `new_re` / `new_rows` / `row_ids` (what the set op writes)."""
    if name in _problems:
        return _problems[name]
    c = CASES[name]
    B, n, N = c['B'], c['n'], c['B'] * (NB + NV)
    if c['kind'] == 'll':
        p = U.make_ll_problem(SEEDS[name], N, n, c['Vw'], c['Ve'], c['dw'], c.get('labels', 'int'))
    else:
        p = U.make_vs_problem(SEEDS[name], N, n, c.get('z', 0), c['Vw'], c['Ve'], c['dw'], c['de'])
    rng = np.random.RandomState(SEEDS[name] + 1000)
    p['perm'] = rng.permutation(B * NB)
    p['row_ids'] = np.sort(rng.choice(c['Vw'], 5, replace=False))
    # (far larger than the rows they replace: in the lazy cases five rows then carry about as much of sum(p^2) as the whole table
    #  did, so a predicted share kept across the write shows in the fp32 loss -- at Glorot scale five rows of 33000 are below its
    #  resolution)
    p['new_rows'] = rng.uniform(-0.5, 0.5, (5, c['dw'])).astype(np.float32)
    if c['kind'] == 'll':
        p['ids'] = rng.randint(0, c['Vw'], size=(3, n)).astype(p['X'].dtype)
        p['queries'] = [rng.randint(0, c['Vw'], size=k) for k in (1, 2, 3)]
    else:
        # (half as large again as the table it replaces: sums of squares kept across the write are off by a factor of 2.25)
        p['new_re'] = (np.float32(1.5) * O.glorot_uniform(rng, (c['Ve'], c['de']))).astype(np.float32)
        p['avg'] = (0.1 * rng.randn(7, c['dw'])).astype(np.float32)
    del p['rng']
    for a in p.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _problems[name] = p
    return p


def touched_fractions(name):
    """Per training batch, before and after the reupload's permutation: distinct words / vocabulary."""
    c, p = CASES[name], case_problem(name)
    B = c['B']
    out = []
    for X in (p['X'][:B * NB], p['X'][:B * NB][p['perm']]):
        out += [len(np.unique(X[j * B:(j + 1) * B])) / float(c['Vw']) for j in range(NB)]
    return out


# --------------------------------------------------------------------------- #
# sequences
# --------------------------------------------------------------------------- #

def build_ops(name):
    """The op list of a case: a function of the case's seed and nothing else."""
    c = CASES[name]
    rng = np.random.RandomState(SEEDS[name] + 2000)
    kinds = other_kinds(name)
    ops = []
    batch = lambda: int(rng.randint(NB))
    train = lambda hint: ops.append(dict(op='train', b=batch(), hint=hint))
    rounds = {k: 0 for k in kinds}
    gets, sets = tensor_names(name), set_forms(name)

    def other(kind):
        r = rounds[kind]
        rounds[kind] += 1
        op = dict(op=kind)
        if kind == 'eval':
            op.update(split=('train', 'valid')[r % 2], b=int(rng.randint(NB if r % 2 == 0 else NV)))
        elif kind == 'eval_many':
            split = ('valid', 'train')[r % 2]
            op.update(split=split, bs=[int(v) for v in rng.randint(NV if split == 'valid' else NB, size=2 + r % 2)])
        elif kind == 'get':
            op.update(which=gets[r % len(gets)])
        elif kind == 'set':
            op.update(form=sets[r % len(sets)])
        elif kind == 'set_step':
            # to current + delta, never the current value; -1 first, behind an announced run: the update number of the next step is
            # one that predictions were made for
            op.update(delta=(-1, 5, -3)[r % 3])
        elif kind == 'set_eval_draws':
            op.update(delta=(7, -2, 3)[r % 3])
        elif kind == 'negatives_of_step':
            op.update(evaluation=bool(r % 2), offset=int(rng.randint(3)))
        ops.append(op)

    # 1. a straight announced run: a full pass of the lazy update, kLazyK - 1 sparse ones, a full one again; every tail but the
    #    last inside the next gather
    for _ in range(6):
        train('right')
    train('none')
    # 2. announcements that are wrong, withdrawn, or met by a step that cannot use them
    train('wrong'); train('cleared'); train('right')
    ops.append(dict(op='train_explicit', b=batch()))                    # discards the run-ahead made for it
    train('right')
    ops.append(dict(op='train_many', bs=[batch(), batch()]))            # its first step takes the run-ahead
    train('right')
    # 3. reads inside an announced run, every tensor once: the first read of a group flushes the rows that are behind under the
    #    run-ahead, which survives it
    for k in range(0, len(gets), 4):
        train('right')
        for g in gets[k:k + 4]:
            rounds['get'] += 1
            ops.append(dict(op='get', which=g))
    train('right'); train('none')
    # 4. every other kind behind an announced run of two steps -- the second leaves rows of a lazy table behind and keeps their
    #    predictions -- and in front of an announced step that announces again (a sparse pass, if the predictions were kept);
    #    then between two steps nobody announced.  (A table that is never lazy: one announcing step in front.)
    for kind in kinds:
        if c['lazy']:
            train('right')
        train('right'); other(kind); train('right'); train('none'); other(kind); train('cleared' if rounds[kind] % 2 else 'none')
    # 5. two calls between an announcing step and the announced one: the first meets the run-ahead, the second what the first left
    for first, second in (('get', 'set_step'), ('eval', 'get'), ('set', 'predict')) if not c.get('short') else ():
        train('right'); train('right'); other(first); other(second); train('right'); train('none')
    if c.get('short'):
        train('right'); other('get'); other('set_step'); train('right'); other('set'); other('predict'); train('none')
    # 6. the end of the sequence inside an announced run
    train('right'); train('right'); train('none')
    return ops


def is_training(op):
    return op['op'] in TRAIN_OPS


def first_batch(op):
    return op['bs'][0] if op['op'] == 'train_many' else op['b']


def next_training(ops, i):
    """Index of the first training op behind op i, or None."""
    for j in range(i + 1, len(ops)):
        if is_training(ops[j]):
            return j
    return None


def hinted_batch(ops, i):
    """The batch a hinted engine announces in front of train op i: an int, -1 (cleared) or None (no call)."""
    op = ops[i]
    assert op['op'] == 'train'
    j = next_training(ops, i)
    nxt = first_batch(ops[j]) if j is not None else None
    if op['hint'] == 'right':
        return nxt
    if op['hint'] == 'wrong':
        return ((nxt if nxt is not None else op['b']) + 1 + i % (NB - 1)) % NB
    return -1 if op['hint'] == 'cleared' else None


def op_positions(ops):
    """{kind: set of positions} of every non-training op: 'behind_live' -- directly behind a training step that announced the
    following training step; 'before_announced' -- directly in front of a training step that the last training step in front
    of the op announced; 'between_unhinted' -- directly between two train ops that announce nothing."""
    out = {}
    for i, op in enumerate(ops):
        if is_training(op):
            continue
        pos = out.setdefault(op['op'], set())
        prev = ops[i - 1] if i > 0 else None
        nxt = ops[i + 1] if i + 1 < len(ops) else None
        if prev is not None and prev['op'] == 'train' and prev['hint'] == 'right' and next_training(ops, i - 1) is not None:
            pos.add('behind_live')
        if nxt is not None and is_training(nxt):
            k = i - 1
            while k >= 0 and not is_training(ops[k]):
                k -= 1
            if k >= 0 and ops[k]['op'] == 'train' and ops[k]['hint'] == 'right':
                pos.add('before_announced')
        if (prev is not None and nxt is not None and prev['op'] == 'train' and nxt['op'] == 'train' and
                prev['hint'] in ('none', 'cleared') and nxt['hint'] in ('none', 'cleared')):
            pos.add('between_unhinted')
    return out


def negatives_drawn_ahead(ops, i):
    """For train op i on an engine that is never hinted: were its negatives drawn during the step before -- a training step
    behind which no invalidating call came?  (The first step of an engine has none; explicit negatives do not use them.)"""
    assert ops[i]['op'] == 'train'
    for k in range(i - 1, -1, -1):
        if is_training(ops[k]):
            return True
        if ops[k]['op'] in INVALIDATING:
            return False
    return False


# --------------------------------------------------------------------------- #
# the oracle replay
# --------------------------------------------------------------------------- #

class Replay(object):
    """The sequence on the oracle, in float32 and in float64 side by side.  The step counter (= Adam's t, = the training
    sampler's position) and the evaluation draw counter are modelled here, on the host."""

    def __init__(self, name):
        c, p = CASES[name], case_problem(name)
        self.name, self.c, self.p = name, c, p
        B, n = c['B'], c['n']
        adam = dict(lr=c.get('lr', 1e-3))
        mk = {'vs': lambda dt: O.VectorSpaceOracle(B, n, c['z'], p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dt, adam_kwargs=adam),
              'fs': lambda dt: O.VectorSpaceSoftmaxOracle(B, n, p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dt, adam_kwargs=adam),
              'll': lambda dt: O.LogLinearOracle(B, n, p['Rw'], p['W'], p['b'], LAM, dtype=dt)}[c['kind']]
        self.oras = (mk(np.float32), mk(np.float64))
        self.step, self.draws = 0, 0
        self.train_rows = np.arange(B * NB)                 # row order of the training split as uploaded
        self.valid_rows = np.arange(B * NB, B * (NB + NV))
        self.clip_margin = np.inf                           # loglinear: min over every clipped probability of its distance
                                                            # from a clip bound as a factor (float64 replay)

    def _batch(self, split, b):
        rows = (self.train_rows if split == 'train' else self.valid_rows)[b * self.c['B']:(b + 1) * self.c['B']]
        p = self.p
        y = p['ydense'][rows] if self.c['kind'] == 'll' else p['y'][rows]
        return p['X'][rows], y, p['w'][rows]

    def _margin(self, f):
        lo, hi = O.clip_bounds(np.float64)
        for a in (f['P3'], f['Q']):
            self.clip_margin = min(self.clip_margin, float(a.min() / lo), float((1.0 - a.max()) / (1.0 - hi)))

    def _train(self, b, neg=None):
        X, y, w = self._batch('train', b)
        kind = self.c['kind']
        if kind == 'vs' and neg is None:
            neg = philox.training_negatives(SEED, self.step, self.c['B'], self.c['z'], self.c['Ve'])
        out = []
        for ora in self.oras:
            if kind == 'vs':
                out.append(ora.train_step(X, y, w, neg))
            elif kind == 'fs':
                out.append(ora.train_step(X, y, w))
            else:
                loss, grads, f = ora.loss_and_grads(X, y, w)
                ora.opt.update(ora.params(), grads)
                if ora.dtype == np.float64:
                    self._margin(f)
                out.append(loss)
        self.step += 1
        return out

    def _eval(self, split, b):
        X, y, _ = self._batch(split, b)
        kind = self.c['kind']
        out = []
        if kind == 'vs':
            neg = philox.evaluation_negatives(SEED, self.draws, self.c['B'], self.c['z'], self.c['Ve'])
            self.draws += 1
        for ora in self.oras:
            if kind == 'vs':
                out.append(ora.eval_loss(X, y, neg))
            elif kind == 'fs':
                out.append(ora.eval_loss(X, y))
            else:
                f = ora.forward(X, y)
                if ora.dtype == np.float64:
                    self._margin(f)
                out.append(O._sum(f['loss'], dtype=ora.dtype) / ora.dtype.type(len(f['loss'])))
        return out

    def apply(self, op):
        """Apply one op; returns its record: dict(op=kind, step, draws after the op, and what the op returns as pairs
        (float32 replay, float64 replay))."""
        k, p, c = op['op'], self.p, self.c
        rec = dict(op=k)
        if k == 'train':
            rec['loss'] = self._train(op['b'])
        elif k == 'train_explicit':
            rec['loss'] = self._train(op['b'], explicit_negatives(self.name, self.step))
        elif k == 'train_many':
            rec['losses'] = [self._train(b) for b in op['bs']]
        elif k == 'eval':
            rec['loss'] = self._eval(op['split'], op['b'])
        elif k == 'eval_many':
            rec['losses'] = [self._eval(op['split'], b) for b in op['bs']]
        elif k == 'get':
            rec['value'] = [np.array(U.oracle_state(ora)[op['which']], copy=True) for ora in self.oras]
        elif k == 'set':
            for ora in self.oras:
                if op['form'] == 'b':
                    ora.b *= ora.dtype.type(0.5)
                elif op['form'] == 'rw_rows':
                    ora.R_w[p['row_ids']] = p['new_rows']
                else:
                    ora.R_e[...] = p['new_re']
        elif k == 'set_step':
            self.step = max(0, self.step + op['delta'])
            for ora in self.oras:
                if hasattr(ora.opt, 't'):
                    ora.opt.t = self.step
        elif k == 'set_eval_draws':
            self.draws = max(0, self.draws + op['delta'])
        elif k == 'reupload':
            self.train_rows = self.train_rows[p['perm']]
        elif k == 'predict':
            if c['kind'] == 'll':
                rec['tokens'] = [ora.token_distributions(p['ids'])[1] for ora in self.oras]
                # (the product over a query's tokens in float64 for both replays: a float32 sum of logarithms of magnitude 9 each
                #  is the aggregate's own rounding, 2e-6 of the score per term at V_e = 9001, not the model's)
                rec['ranks'] = [[O.loglinear_rank(ora.token_distributions(np.asarray(q)[None, :])[1][0].astype(np.float64))
                                 for q in p['queries']] for ora in self.oras]
                rec['ranks'] = [[_by_entity(order, sc) for order, sc in per] for per in rec['ranks']]
            else:
                rec['value'] = [ora.predict(p['avg']) for ora in self.oras]
        elif k == 'negatives_of_step':
            pos = (self.draws if op['evaluation'] else self.step) + op['offset']
            draw = philox.evaluation_negatives if op['evaluation'] else philox.training_negatives
            rec['value'] = draw(SEED, pos, c['B'], c['z'], c['Ve'])
        else:
            assert k == 'synchronize', k
        rec['step'], rec['draws'] = self.step, self.draws
        return rec


def _by_entity(order, scores):
    out = np.empty(len(order), dtype=np.float64)
    out[order] = scores
    return out


def explicit_negatives(name, step):
    """What train_explicit passes: the negatives the device sampler draws at training position `step` (Engine.negatives_of_step
    returns the same array; the GPU test asserts it)."""
    c = CASES[name]
    return philox.training_negatives(SEED, step, c['B'], c['z'], c['Ve']) if c['kind'] == 'vs' else None


_reference = {}


def case_reference(name):
    """dict(ops, records = Replay.apply's record per op, final = (oracle_state of the float32 replay, of the float64 one),
    clip_margin, seconds) of a case -- computed once per process and shared by the engines of its test; read-only.  Only the
    case asked for last is kept (the snapshots of a lazy case's reads are tens of megabytes each)."""
    if name not in _reference:
        _reference.clear()
        t0 = time.time()
        ops = build_ops(name)
        rp = Replay(name)
        records = [rp.apply(op) for op in ops]
        _reference[name] = dict(ops=ops, records=records, final=tuple(U.oracle_state(ora) for ora in rp.oras),
                                clip_margin=rp.clip_margin, seconds=time.time() - t0)
    return _reference[name]


# --------------------------------------------------------------------------- #
# engines
# --------------------------------------------------------------------------- #

def make_engine(name, keep_grads=0):
    c, p = CASES[name], case_problem(name)
    ll = c['kind'] == 'll'
    kind = {'vs': C.KIND_VECTORSPACE, 'fs': C.KIND_VECTORSPACE_SOFTMAX, 'll': C.KIND_LOGLINEAR}[c['kind']]
    opt = dict(lr=1.0, beta1=0.95, beta2=0.0, eps=1e-6) if ll else dict(lr=c.get('lr', 1e-3), beta1=0.9, beta2=0.999, eps=1e-8)
    eng = C.Engine(kind=kind, batch_size=c['B'], global_batch_size=c['B'], window_size=c['n'], vocab_size=c['Vw'],
                   num_entities=c['Ve'], word_dim=c['dw'], entity_dim=0 if ll else c['de'], num_negatives=c.get('z', 0),
                   id_bytes=p['X'].dtype.itemsize, device=0, keep_grads=keep_grads, deterministic=1, lambda_=LAM, seed=SEED, **opt)
    eng.set_tensor(C.T_RW, p['Rw'])
    if not ll:
        eng.set_tensor(C.T_RE, p['Re'])
    eng.set_tensor(C.T_W, p['W'])
    eng.set_tensor(C.T_B, p['b'])
    upload(eng, name, 'train', np.arange(c['B'] * NB))
    upload(eng, name, 'valid', np.arange(c['B'] * NB, c['B'] * (NB + NV)))
    return eng


def upload(eng, name, split, rows):
    c, p = CASES[name], case_problem(name)
    sp = C.SPLIT_TRAIN if split == 'train' else C.SPLIT_VALIDATE
    w = p['w'][rows] if split == 'train' else None
    if c.get('labels') == 'csr':
        eng.upload_dataset(sp, p['X'][rows], csr=p['y'][rows], w=w)
    else:
        eng.upload_dataset(sp, p['X'][rows], y_int=p['y'][rows], w=w)


def apply_op(eng, name, ops, i, hinted, state):
    """Apply op i to an engine; `state` is the caller's dict for this engine (the row order of its training split).  Returns what
    the call returned, as the replay's record names it: 'loss' / 'losses' (float32), 'value', 'tokens', 'ranks'."""
    c, p, op = CASES[name], case_problem(name), ops[i]
    k = op['op']
    sp = lambda s: C.SPLIT_TRAIN if s == 'train' else C.SPLIT_VALIDATE
    out = {}
    if k == 'train':
        h = hinted_batch(ops, i) if hinted else None
        if h is not None:
            eng.hint_next_batch(None if h < 0 else h)
        out['loss'] = eng.train_batch(op['b'])
    elif k == 'train_explicit':
        neg = eng.negatives_of_step(eng.get_step()) if c['kind'] == 'vs' else None
        out['negatives'] = neg
        out['loss'] = eng.train_batch(op['b'], neg)
    elif k == 'train_many':
        out['losses'] = eng.train_batches(op['bs'])
    elif k == 'eval':
        out['loss'] = eng.eval_batch(sp(op['split']), op['b'])
    elif k == 'eval_many':
        out['losses'] = eng.eval_batches(sp(op['split']), op['bs'])
    elif k == 'get':
        par = op['which'].rpartition('.')[2]
        out['value'] = eng.get_tensor(tensor_id(op['which']), U.state_shapes(eng.cfg)[par])
    elif k == 'set':
        if op['form'] == 'b':
            eng.set_tensor(C.T_B, eng.get_tensor(C.T_B) * np.float32(0.5))
        elif op['form'] == 'rw_rows':
            rw = eng.get_tensor(C.T_RW, (c['Vw'], c['dw']))
            rw[p['row_ids']] = p['new_rows']
            eng.set_tensor(C.T_RW, rw)
        else:
            eng.set_tensor(C.T_RE, p['new_re'])
    elif k == 'set_step':
        eng.set_step(max(0, eng.get_step() + op['delta']))
    elif k == 'set_eval_draws':
        eng.set_eval_draws(max(0, eng.get_eval_draws() + op['delta']))
    elif k == 'reupload':
        state['train_rows'] = state['train_rows'][p['perm']]
        upload(eng, name, 'train', state['train_rows'])
    elif k == 'predict':
        if c['kind'] == 'll':
            out['tokens'] = eng.predict_tokens(p['ids'])
            idx, score, _, _, status, _ = eng.ll_rank_queries(p['queries'])
            out['ranks'] = (idx, score, status)
        else:
            out['value'] = eng.predict_project(p['avg'])
    elif k == 'negatives_of_step':
        pos = (eng.get_eval_draws() if op['evaluation'] else eng.get_step()) + op['offset']
        out['value'] = eng.negatives_of_step(pos, evaluation=op['evaluation'])
    else:
        assert k == 'synchronize', k
        eng.synchronize()
    out['step'], out['draws'] = eng.get_step(), eng.get_eval_draws()
    return out
