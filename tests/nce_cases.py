"""Vectorspace problems whose only difficulty is WHICH template instance of the NCE score / loss / gradient kernel they reach --
shared by the CPU proof of the inputs (test_nce_inputs_cpu.py) and the GPU test (test_gpu_nce_forms.py).

vs_loss<TRAIN> (csrc/host/step_vectorspace.inc) picks the kernel (csrc/kernels_vs.h) from d_e and z alone:

  regs           vs_nce_regs<NCH, TRAIN, MAXC>: d_e % 4 == 0, NCH = ceil(d_e / 64) <= 4 and z + 1 <= 12; MAXC = 6 for z + 1 <= 6,
                 else 12.  Lane l of a row's sixteen holds candidate min(l, z); the lanes past z contribute nothing.
  per_candidate  vs_nce<NCH, TRAIN>: d_e % 4 == 0 otherwise -- NCH 5..8 at any z, NCH 1..4 only when z + 1 >= 13.
  scalar         vs_nce_scalar<NPL, TRAIN>: d_e % 4 != 0, NPL = ceil(d_e / 64); one wave per row, four rows per workgroup.

That is 8 + 8 + 8 instances, each compiled for training and for evaluation, each with masks of its own: `c < chunks` for the
last float4 chunk of a row (scalar: `c < de` in the last 64-column slice), `l <= z` for the lanes that hold a candidate, the
clamped rows of a ragged last workgroup, the workgroup's loss partial over valid rows only.  Every instance gets the smallest
d_e that reaches it (one lane alone in the last chunk / slice) and the largest (every lane full); z sits on both sides of every
threshold of the dispatch (z + 1 = 6 | 7 and 12 | 13) and at 0; B is 5 (less than a workgroup of 16 rows, ragged for the
scalar form's 4), 16 (exactly one), 37 or 67 (ragged in both).

Everything else is fixed and tiny (util.make_vs_problem: Glorot parameters, weights in [0.5, 2]; lambda = 0.01) with explicit
negatives.  Planted in every batch: entity 0 is the target of the first row and entity V_e - 1 of the last; one row's target is
among its own negatives (z >= 1); one row of each training batch has weight exactly 0.  The data set is 3 B rows: two training
batches (the second step reads the tables the first one updated) and a third batch that is evaluated.

Each case states the form Engine.nce_form() (sert_debug_nce_form) must report."""
import numpy as np

from oracle import sert_oracle as O
from tests import util as U

N, VW, DW, VE, LAM = 2, 50, 8, 7, 0.01
TRAIN_STEPS, BATCHES = 2, 3
BATCH_SIZES = (5, 16, 37, 67)
SCALAR_Z = (0, 1, 5, 6, 11, 12)
LOSS_TOL, ACT_TOL = 1e-5, 2e-5                # tests/test_gpu_parity.py, unchanged; the gradients take U.ROW_TOL64
LO, HI = O.clip_bounds(np.float32)
LOGIT_LO = float(np.log(np.float64(LO)) - np.log1p(-np.float64(LO)))
SIGMOID_CUT = 15.0                            # Theano's float32 sigmoid is 1 above it: the upper decision point of the mask

# d_e and z of every case, family by family
_REGS = [  # (NCH, de, z for MAXC 6, z for MAXC 12)
    (1, 4, 0, 6), (1, 64, 5, 11), (2, 68, 5, 11), (2, 128, 1, 6), (3, 132, 0, 6), (3, 192, 5, 11), (4, 196, 5, 11), (4, 256, 2, 6)]
_PER_CANDIDATE = [(4, 12), (64, 12), (68, 12), (128, 15), (132, 12), (192, 13), (196, 12), (256, 12),
                  (260, 0), (320, 5), (324, 6), (384, 12), (388, 1), (448, 11), (452, 5), (512, 12)]
_SCALAR = [5, 63, 65, 127, 129, 191, 193, 255, 257, 319, 321, 383, 385, 447, 449, 511]


def _cases():
    rows = []
    for nch, de, z6, z12 in _REGS:
        rows.append(('regs%dx6_de%d_z%d' % (nch, de, z6), z6, de, dict(form='regs', param=nch, maxc=6)))
        rows.append(('regs%dx12_de%d_z%d' % (nch, de, z12), z12, de, dict(form='regs', param=nch, maxc=12)))
    for de, z in _PER_CANDIDATE:
        nch = -(-de // 64)
        rows.append(('cand%d_de%d_z%d' % (nch, de, z), z, de, dict(form='per_candidate', param=nch, maxc=0)))
    for k, de in enumerate(_SCALAR):
        z = SCALAR_Z[k % len(SCALAR_Z)]
        rows.append(('scalar%d_de%d_z%d' % (-(-de // 64), de, z), z, de, dict(form='scalar', param=-(-de // 64), maxc=0)))
    # B: the four sizes in turn, the turn shifted by one after every four cases -- every form walks through all four and the two
    # widths of one instance get two different ones
    return {name: dict(B=BATCH_SIZES[(k + k // 4) % 4], z=z, de=de, form=form) for k, (name, z, de, form) in enumerate(rows)}


CASES = _cases()
SEEDS = {name: 700 + k for k, name in enumerate(CASES)}
# Picked on the CPU, from the oracle alone (test_nce_inputs_cpu.py: the float32 oracle within a quarter of every bound of the
# float64 one).  With z = 1 a row whose target is also its negative has da = g (2 sigmoid(u) - 1) R_e[y], which cancels as
# u -> 0: the first seeds of these cases hold such a row with |u| ~ 1e-3, where the float32 ORACLE misses U.ROW_TOL64 by itself.
SEEDS.update(regs2x6_de128_z1=1006, cand7_de388_z1=828, scalar4_de255_z1=839)

# the 24 instances, as (form, NCH or NPL, MAXC)
INSTANCES = ([('regs', n, c) for n in (1, 2, 3, 4) for c in (6, 12)] + [('per_candidate', n, 0) for n in range(1, 9)] +
             [('scalar', n, 0) for n in range(1, 9)])


def instance_of(c):
    f = c['form']
    return f['form'], f['param'], f['maxc']


def dispatch(de, z):
    """The form vs_loss picks for (d_e, z), restated from the table above."""
    if de % 4:
        return dict(form='scalar', param=-(-de // 64), maxc=0)
    nch = -(-(de // 4) // 16)
    if nch <= 4 and z + 1 <= 12:
        return dict(form='regs', param=nch, maxc=6 if z + 1 <= 6 else 12)
    return dict(form='per_candidate', param=nch, maxc=0)


def launch_shape(c, train):
    """(workgroups, loss partials) the hook must report: sixteen rows per workgroup and one loss partial per workgroup in a
    training step; the scalar form has four rows per workgroup and leaves no partials, and no evaluating instance does."""
    if c['form']['form'] == 'scalar':
        return -(-c['B'] // 4), 0
    wg = -(-c['B'] // 16)
    return wg, wg if train else 0


def zero_weight_row(B):
    return B // 2


def self_negative_row(B):
    return B // 2 - 1


def last_slice_columns(c):
    """Columns of the last float4 chunk of a row (scalar form: of its last 64-column slice)."""
    width = 64 if c['form']['form'] == 'scalar' else 4
    return c['de'] - width * (-(-c['de'] // width) - 1)


_cache = {}


def case_problem(name):
    """(case dict, problem) of a case, built once per process; treat both as read-only.  problem: the dict of
    util.make_vs_problem over BATCHES batches of B rows with the plants of the module docstring, neg = [neg (B, z) int64 of
    each batch]."""
    if name not in _cache:
        c = CASES[name]
        B, z = c['B'], c['z']
        p = U.make_vs_problem(SEEDS[name], B * BATCHES, N, z, VW, VE, DW, c['de'])
        rng = np.random.RandomState(SEEDS[name] + 1000)
        p['neg'] = [rng.randint(0, VE, size=(B, z)).astype(np.int64) for _ in range(BATCHES)]
        for b in range(BATCHES):
            p['y'][b * B] = 0
            p['y'][b * B + B - 1] = VE - 1
            if z >= 1:
                r = self_negative_row(B)
                p['neg'][b][r, z // 2] = p['y'][b * B + r]
            if b < TRAIN_STEPS:
                p['w'][b * B + zero_weight_row(B)] = 0
        for a in list(p.values()) + p['neg']:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, p)
    return _cache[name]


def batch_slice(c, b):
    return slice(b * c['B'], (b + 1) * c['B'])


_refs = {}


def case_reference(name, dtype):
    """The oracle's run of a case in `dtype`, computed once per process and shared (read-only): a list of three dicts.  The
    two training steps: loss (with the regulariser), rowloss = w * row loss, da, dRe (with the L2 term), and t, u, sig, cand and
    Re (the table the step read) for the input proofs.  The evaluation of the third batch by the parameters after both
    updates: loss (unweighted mean, no regulariser) and rowloss (unweighted)."""
    key = (name, np.dtype(dtype).name)
    if key not in _refs:
        c, p = case_problem(name)
        ora = O.VectorSpaceOracle(c['B'], N, c['z'], p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dtype)
        steps = []
        for s in range(BATCHES):
            sl = batch_slice(c, s)
            if s < TRAIN_STEPS:
                Re = ora.R_e.copy()
                loss, g, f = ora.loss_and_grads(p['X'][sl], p['y'][sl], p['w'][sl], p['neg'][s])
                st = dict(loss=loss, rowloss=np.asarray(p['w'][sl], dtype) * f['loss'], da=f['da'], dRe=g[0], Re=Re)
                ora.opt.update(ora.params(), g)
            else:
                f = ora.forward(p['X'][sl], p['y'][sl], p['neg'][s])
                st = dict(loss=ora.eval_loss(p['X'][sl], p['y'][sl], p['neg'][s]), rowloss=f['loss'], Re=ora.R_e.copy())
            st.update({k: f[k] for k in ('t', 'p', 'u', 'sig', 'cand')})
            for a in st.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            steps.append(st)
        _refs[key] = steps
    return _refs[key]


# --------------------------------------------------------------------------------------------------------------------- #
# the two measures of the GPU test, and the kernel's contract restated so that a reference can be made wrong on purpose
# --------------------------------------------------------------------------------------------------------------------- #

def rowloss_err(got, ref):
    """(worst error, its row) of row losses as _check_rowloss of tests/test_gpu_parity.py prices them: each row against its own
    magnitude, floored at 1e-3 of the mean magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).mean())
    return float(err.max()), int(err.argmax())


def nce_rows(t, Re, cand, w, drop_columns=0, drop_last_candidate=False):
    """float64: (w * row loss (B), da (B, d_e)) of the kernel's contract (csrc/kernels_vs.h, K6) from the projection t, the
    entity table and the candidates, for scores inside every clip.  drop_columns: that many trailing columns are left out of
    the dot products and of da; drop_last_candidate: candidate z is left out -- the two masks an instance could get wrong."""
    t, Re, w = np.asarray(t, np.float64), np.asarray(Re, np.float64), np.asarray(w, np.float64)
    B, de = t.shape
    keep = de - drop_columns
    if drop_last_candidate:
        cand = cand[:, :-1]
    p = np.clip(t, -np.float64(HI), np.float64(HI))
    E = Re[cand]                                              # (B, candidates, d_e)
    u = (E[:, :, :keep] * p[:, None, :keep]).sum(axis=2)
    sig = 1.0 / (1.0 + np.exp(-u))
    logs = np.log1p(-sig)
    du = (w / B)[:, None] * sig
    if cand.shape[1]:
        logs[:, 0] = np.log(sig[:, 0])
        du[:, 0] = -(w / B) * (1.0 - sig[:, 0])
    dp = (du[:, :, None] * E).sum(axis=1)
    dp[:, keep:] = 0
    return -w * logs.sum(axis=1), dp * (1.0 - t * t)


def mask_margins(st32, st64):
    """(err, margin of the scores, margin of t) of one step of the float32 reference: err = max |u32 - u64| with u64 the float64
    dot product of the float32 oracle's own R_e rows and p (the measure of tests/test_gpu_vs_saturated.py), joined with the
    float32 oracle's distance from the float64 one in t; the scores' distance from the two decision points of the sigmoid
    mask, u = 15 and u = logit(1e-7); the distance of max |t| from the clip bound 1 - 2^-23."""
    E = st32['Re'][st32['cand']]
    u64 = np.einsum('bcd,bd->bc', E.astype(np.float64), st32['p'].astype(np.float64))
    err = float(np.abs(st32['u'].astype(np.float64) - u64).max())
    err = max(err, float(np.abs(st32['t'].astype(np.float64) - st64['t']).max()))
    mu = float(min(SIGMOID_CUT - u64.max(), u64.min() - LOGIT_LO))
    mt = float(np.float64(HI) - np.abs(st32['t'].astype(np.float64)).max())
    return err, mu, mt
