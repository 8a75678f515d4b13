"""Loglinear problems that are tame apart from ONE non-finite value planted into the initial parameters -- shared by the CPU
proof of the inputs (test_ll_nonfinite_inputs_cpu.py) and the GPU test (test_gpu_ll_nonfinite.py).

The contract under test: a non-finite parameter that a batch reads makes that batch's loss non-finite (the epoch loop stops
on nothing else, sert_amd/models.py _EpochPass.accept).  np.clip and Theano's Clip keep a NaN; a clip written as
fminf(fmaxf(x, lo), hi) returns lo for one, and a loss kernel that clips that way reports a finite loss while its backward
fills W and b with NaN -- after which every step returns log(V_e) for ever.  One case per loss form the default build can
reach (csrc/host/step_softmax_loglinear.inc, ll_forward), the expected form recorded for each of the four launches of the
GPU test as Engine.ll_loss_form() reports it.

Every problem is tame apart from its plant: Glorot-scale parameters, no probability within a factor two of a clip bound (the
CPU test proves it), lambda = 0 -- with a positive lambda the L2 term's sum of squares would carry most plants into the loss
whatever the kernels do."""
import numpy as np

from oracle import sert_oracle as O
from tests import util as U

B, VW, D, NB, NV, LAM = 8, 120, 16, 2, 1, 0.0         # rows per batch, words, word dim, training / validation batches
N = B * (NB + NV)                                     # rows 0 .. B*NB - 1: the training split, the rest: the validation split
LONG_ROW_LABELS = 1025                                # csrc/kernels_ll.h: kLlFusedLabels + 1

# Three reserved words, one per window position a word plant sits at.  Each occurs exactly once in batch 0 of the training
# split (so the distinct-word table of that batch poisons ONE row) and once in the validation batch, never in batch 1.
# position: 0, the last one, and 3 -- with n = 7 these fall into every trip of the row loops of ll_row_wave (three window
# rows in flight) and ll_row_from_table (five).
PLANT_WORDS = {'first': VW - 3, 'last': VW - 2, 'mid': VW - 1}
TRAIN_ROW = {'first': 0, 'last': 5, 'mid': 6}         # row of batch 0 that holds the word (two wave-per-row workgroups)
VALID_ROW = {'first': 3, 'last': 0, 'mid': 5}         # row of the validation batch that holds it
WORD_COLUMN = 5                                       # the element of the word's row that is planted


def position(which, n):
    return {'first': 0, 'last': n - 1, 'mid': 3}[which]


def _form(form, param, train, slots, segments=0):
    return dict(form=form, param=param, train=train, slots=slots, segments=segments)


def _forms(train, evaluate, segments=0):
    """The four launches of the GPU test.  A training step and an evaluation of the TRAINING split read the distinct-word
    table through per-token slots; the validation split has no word index.  keep_grads does not enter ll_forward's choice."""
    step = _form(train[0], train[1], True, True, segments)
    return dict(train_keep0=step, train_keep1=dict(step),
                ev_train=_form(evaluate[0], evaluate[1], False, True, segments),
                ev_valid=_form(evaluate[0], evaluate[1], False, False, segments))


# id -> window, V_e, label kind and the forms.  ll_forward: (n + 1) V_e floats within 150 KiB of LDS and no row above
# kLlFusedLabels labels -> a fused form; training with n <= 64: ll_row_wave<cdiv(V_e / 4, 64) rounded up to 1, 2, 4, 8> where
# V_e % 4 == 0 and V_e <= 2048, else ll_row_from_table<128> up to V_e = 2048 and <512> above; n > 64 and every fused
# evaluation: ll_fused_row<512>.  Otherwise the streaming kernels, param = 1 with 16-byte rows (V_e % 4 == 0), over
# cdiv(V_e, 4096) segments.  b_std / b_mean of `fusedrow`: see tests/ll_csr_cases.py.
CASES = {
    'wave1': dict(n=7, Ve=256, forms=_forms(('wave', 1), ('fused_row', 512))),
    'wave2': dict(n=7, Ve=400, forms=_forms(('wave', 2), ('fused_row', 512))),
    'wave4': dict(n=7, Ve=800, forms=_forms(('wave', 4), ('fused_row', 512))),
    'wave8': dict(n=7, Ve=1028, forms=_forms(('wave', 8), ('fused_row', 512))),
    'table128': dict(n=7, Ve=601, forms=_forms(('table', 128), ('fused_row', 512))),
    'table512': dict(n=7, Ve=2050, forms=_forms(('table', 512), ('fused_row', 512))),
    'fusedrow': dict(n=65, Ve=300, b_std=0.1 * 3 / 65, b_mean=0.3, forms=_forms(('fused_row', 512), ('fused_row', 512))),
    'stream_scalar': dict(n=4, Ve=9001, forms=_forms(('stream', 0), ('stream', 0), segments=3)),
    'stream_v4': dict(n=4, Ve=9004, forms=_forms(('stream', 1), ('stream', 1), segments=3)),
    'fallback': dict(n=7, Ve=1028, labels='csr', forms=_forms(('stream', 1), ('stream', 1), segments=1)),
}
SEEDS = {name: 300 + k for k, name in enumerate(CASES)}

# plant -> what is written (see planted()).  neg_inf_bias is the control: exp(-inf) = 0, the probability clips to 1e-7, its
# mask is zero, and loss and gradients are finite -- a repair that poisons too much fails there.
WORD_PLANTS = {'nan_word': ('first', np.nan), 'nan_word_last': ('last', np.nan), 'nan_word_mid': ('mid', np.nan),
               'inf_word': ('first', np.inf)}
DENSE_PLANTS = ('nan_bias_first', 'nan_bias_last', 'nan_W')
CONTROL = 'neg_inf_bias'
PLANTS = tuple(WORD_PLANTS) + DENSE_PLANTS + (CONTROL,)


def make_problem(name):
    """dict(Rw, W, b, X, w, y = int labels or a CSR matrix, ydense = what the oracle takes, free = an entity that is no row's
    label).  CSR (`fallback`): row 0 of the training split and row 0 of the validation split hold LONG_ROW_LABELS labels --
    every entity but three -- so that both splits take the streaming kernels; every other row has one to four."""
    c = CASES[name]
    n, Ve = c['n'], c['Ve']
    rng = np.random.RandomState(SEEDS[name])
    Rw = O.glorot_uniform(rng, (VW, D))
    W = O.glorot_uniform(rng, (D, Ve))
    b = (c.get('b_mean', 0.0) + c.get('b_std', 0.1) * rng.randn(Ve)).astype(np.float32)
    X = rng.randint(0, VW - len(PLANT_WORDS), size=(N, n))
    for which, word in PLANT_WORDS.items():
        X[TRAIN_ROW[which], position(which, n)] = word
        X[B * NB + VALID_ROW[which], position(which, n)] = word
    X = X.astype(U.id_dtype(VW))
    w = rng.uniform(0.5, 2.0, N).astype(np.float32)
    if c.get('labels', 'int') == 'int':
        y = rng.randint(0, Ve, size=N).astype(np.int32)
        ydense, used = y, set(y.tolist())
    else:
        import scipy.sparse as sp
        spare = np.sort(rng.choice(Ve, Ve - LONG_ROW_LABELS, replace=False))      # the entities the long rows leave out
        others = np.setdiff1d(np.arange(Ve), spare)
        assert len(others) == LONG_ROW_LABELS
        indptr, indices, data = [0], [], []
        for r in range(N):
            cols = others if r in (0, B * NB) else np.sort(rng.choice(others, 1 + r % 4, replace=False))
            vals = rng.uniform(0.5, 1.5, len(cols))
            indices += cols.tolist()
            data += (vals / vals.sum()).tolist()
            indptr.append(len(indices))
        y = sp.csr_matrix((np.array(data, dtype=np.float32), np.array(indices, dtype=np.int32),
                           np.array(indptr, dtype=np.int64)), shape=(N, Ve))
        ydense, used = np.asarray(y.todense(), dtype=np.float32), set(indices)
    free = min((e for e in range(Ve) if e not in used), key=lambda e: abs(e - Ve // 2))
    return dict(Rw=Rw, W=W, b=b, X=X, w=w, y=y, ydense=ydense, free=int(free))


_problems = {}


def case_problem(name):
    """(case dict, problem) of a case, built once per process; treat both as read-only."""
    if name not in _problems:
        p = make_problem(name)
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _problems[name] = (CASES[name], p)
    return _problems[name]


def planted(name, plant):
    """(R_w, W, b, info) of a case with one plant written in (plant None: the clean problem).  info: rows of batch 0 and of
    the validation batch whose loss the plant must make non-finite, and for the control the entity whose bias is -inf."""
    c, p = case_problem(name)
    Rw, W, b = p['Rw'].copy(), p['W'].copy(), p['b'].copy()
    info = dict(train_rows=[], valid_rows=[], entity=None)
    if plant in WORD_PLANTS:
        which, value = WORD_PLANTS[plant]
        Rw[PLANT_WORDS[which], WORD_COLUMN] = value
        info.update(train_rows=[TRAIN_ROW[which]], valid_rows=[VALID_ROW[which]])
    elif plant in DENSE_PLANTS:
        if plant == 'nan_bias_first':
            b[0] = np.nan
        elif plant == 'nan_bias_last':
            b[c['Ve'] - 1] = np.nan                       # the ragged last lane / float4 / segment
        else:
            W[D // 2, c['Ve'] - 1] = np.nan
        info.update(train_rows=list(range(B)), valid_rows=list(range(B)))
    elif plant == CONTROL:
        b[p['free']] = -np.inf
        info['entity'] = p['free']
    else:
        assert plant is None, plant
    return Rw, W, b, info


def split(p, which, batch=0):
    """(X, y for the oracle, w) of one batch of the training split or of the validation batch."""
    r0 = batch * B if which == 'train' else B * NB
    sl = slice(r0, r0 + B)
    return p['X'][sl], p['ydense'][sl], p['w'][sl]


_refs = {}


def reference(name, plant, dtype):
    """The oracle's run of a case with a plant in `dtype`, computed once per process and shared; read-only.  dict:
    ev_train / ev_valid = eval_loss of batch 0 and of the validation batch at the INITIAL parameters (with the per-row losses
    ev_train_rows / ev_valid_rows), steps = per training step dict(loss, rowloss = the unweighted per-row losses, params =
    copies of [R_w, W, b] after the update, f = the forward's intermediates -- clean problem only), ora = the oracle after
    the last step."""
    key = (name, plant, np.dtype(dtype).name)
    if key not in _refs:
        c, p = case_problem(name)
        Rw, W, b, _ = planted(name, plant)
        with np.errstate(all='ignore'):
            ora = O.LogLinearOracle(B, c['n'], Rw, W, b, LAM, dtype=dtype)
            out = {}
            for which in ('train', 'valid'):
                X, y, _ = split(p, which)
                out['ev_' + which] = ora.eval_loss(X, y)
                out['ev_%s_rows' % which] = ora.forward(X, y)['loss']
            steps = []
            for s in range(NB):
                X, y, w = split(p, 'train', s)
                loss, grads, f = ora.loss_and_grads(X, y, w)
                ora.opt.update(ora.params(), grads)
                steps.append(dict(loss=loss, rowloss=f['loss'], params=[np.array(a, copy=True) for a in ora.params()],
                                  f=f if plant is None else None))
            out.update(steps=steps, ora=ora)
        _refs[key] = out
    return _refs[key]
