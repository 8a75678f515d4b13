"""Vectorspace problems that reach the EXACT-COUNT instances of the NCE score / loss / gradient kernel, vs_nce_regs<NCH, TRAIN, 11>
-- shared by the CPU proof of the inputs (test_nce_exact_inputs_cpu.py) and the GPU test (test_gpu_nce_exact.py).  The companion
of tests/nce_cases.py, whose constants, plants and measures are used as they are.

vs_loss<TRAIN> (csrc/host/step_vectorspace.inc) picks MAXC of the regs form from z alone: 6 for z + 1 <= 6, 11 for z + 1 == 11
exactly (z = 10 is the reference's default; a twelfth slot would fetch, dot and scale by 0 one more entity row per pair), 12 for
every other z + 1 <= 12.  With MAXC = 11 every slot of the body holds a real candidate: the mask `l <= z` still decides which
LANES carry a score (lanes 11..15 repeat candidate 10 and contribute nothing), but no slot is idle.  A training step whose d_e
is 64 NCH exactly -- every lane full -- runs the instance without the `c < chunks` masks (<NCH, true, MAXC, true>); every other
width and every evaluation runs the masked one.  The largest width of each NCH below reaches the former in its two training
steps, the smallest the latter.

  CASES       z = 10 at the smallest and the largest d_e of every NCH (one lane alone in the last chunk / every lane full);
              B walks through 5 (less than a workgroup of 16 rows), 16 (exactly one), 37 and 67 (ragged).
  NEIGHBOURS  z = 9 and z = 11 at d_e = 128: on either side of the exact count, still MAXC = 12.
  SATURATED   z = 10, d_e = 128, B = 37 with two of every three columns of the projection weights scaled until their
              pre-activations have a standard deviation of 6 (tests/test_gpu_vs_saturated.py: _scale_projection): every batch
              has units with |t| above the clip bound 1 - 2^-23, whose da is exactly 0 -- the clip mask in the epilogue of
              <2, true, 11, true>, the instance the default settings train with.  The scores stay O(1): no sigmoid mask is near.

Everything else is as in tests/nce_cases.py: V_w = 50, V_e = 7, d_w = 8, window 2, lambda = 0.01, explicit negatives; entity 0 is
the target of the first row and V_e - 1 of the last; one row's target is among its own negatives; one row of each training batch
has weight exactly 0; two training batches and a third that is evaluated."""
import numpy as np

from oracle import sert_oracle as O
from tests import nce_cases as K
from tests import util as U

Z = 10
WIDTHS = [(1, 4), (1, 64), (2, 68), (2, 128), (3, 132), (3, 192), (4, 196), (4, 256)]     # (NCH, d_e)
SURE_A = 10.0      # |a| at or above it: 1 - tanh < 4.2e-9 < 2^-25, t is +-1 in float32 by any tanh good to a few ulp -- clipped for sure


def _form(nch, maxc):
    return dict(form='regs', param=nch, maxc=maxc)


CASES = {'regs%dx11_de%d_z10' % (nch, de): dict(B=K.BATCH_SIZES[k % 4], z=Z, de=de, form=_form(nch, 11))
         for k, (nch, de) in enumerate(WIDTHS)}
NEIGHBOURS = {'regs2x12_de128_z9': dict(B=37, z=9, de=128, form=_form(2, 12)),
              'regs2x12_de128_z11': dict(B=67, z=11, de=128, form=_form(2, 12))}
SATURATED = {'regs2x11_de128_z10_saturated': dict(B=37, z=Z, de=128, form=_form(2, 11), saturated=True)}
ALL = dict(CASES, **dict(NEIGHBOURS, **SATURATED))
# Picked on the CPU, from the oracle alone (test_nce_exact_inputs_cpu.py): the float32 oracle within a quarter of every bound of
# the float64 one, every score ten of its own errors away from the sigmoid's masks.
SEEDS = {name: 900 + k for k, name in enumerate(ALL)}

# the eight new instances, as (form, NCH, MAXC); each compiled for training and for evaluation
INSTANCES = [('regs', n, 11) for n in (1, 2, 3, 4)]


def dispatch(de, z):
    """The form vs_loss picks for (d_e, z): the table of tests/nce_cases.py with the exact-count branch."""
    d = K.dispatch(de, z)
    if d['form'] == 'regs' and z + 1 == 11:
        d = dict(d, maxc=11)
    return d


def _scale_projection(p, B):
    """tests/test_gpu_vs_saturated.py: two of every three columns of W times sW, chosen from the first batch so that those
    columns of a get a standard deviation of 6; every third column stays at its Glorot scale."""
    scaled = np.arange(p['W'].shape[1]) % 3 != 2
    h = p['Rw'][p['X'][:B].astype(np.int64)].sum(axis=1, dtype=np.float64) / p['X'].shape[1]
    sW = float(np.round(6.0 / (h @ p['W'])[:, scaled].std()))
    p['W'][:, scaled] *= np.float32(sW)
    p['sW'] = sW


_cache = {}


def case_problem(name):
    """(case dict, problem) of a case, built once per process and read-only: tests/nce_cases.py: case_problem, same plants."""
    if name not in _cache:
        c = ALL[name]
        B, z = c['B'], c['z']
        p = U.make_vs_problem(SEEDS[name], B * K.BATCHES, K.N, z, K.VW, K.VE, K.DW, c['de'])
        rng = np.random.RandomState(SEEDS[name] + 1000)
        p['neg'] = [rng.randint(0, K.VE, size=(B, z)).astype(np.int64) for _ in range(K.BATCHES)]
        if c.get('saturated'):
            _scale_projection(p, B)
        for b in range(K.BATCHES):
            p['y'][b * B] = 0
            p['y'][b * B + B - 1] = K.VE - 1
            r = K.self_negative_row(B)
            p['neg'][b][r, z // 2] = p['y'][b * B + r]
            if b < K.TRAIN_STEPS:
                p['w'][b * B + K.zero_weight_row(B)] = 0
        for a in list(p.values()) + p['neg']:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, p)
    return _cache[name]


_refs = {}


def case_reference(name, dtype):
    """The oracle's run of a case in `dtype`, once per process and read-only: tests/nce_cases.py: case_reference, with the
    pre-activation a beside t (the saturated case decides by it which units are clipped for sure)."""
    key = (name, np.dtype(dtype).name)
    if key not in _refs:
        c, p = case_problem(name)
        ora = O.VectorSpaceOracle(c['B'], K.N, c['z'], p['Rw'], p['Re'], p['W'], p['b'], K.LAM, dtype=dtype)
        steps = []
        for s in range(K.BATCHES):
            sl = K.batch_slice(c, s)
            if s < K.TRAIN_STEPS:
                Re = ora.R_e.copy()
                loss, g, f = ora.loss_and_grads(p['X'][sl], p['y'][sl], p['w'][sl], p['neg'][s])
                st = dict(loss=loss, rowloss=np.asarray(p['w'][sl], dtype) * f['loss'], da=f['da'], dRe=g[0], Re=Re)
                ora.opt.update(ora.params(), g)
            else:
                f = ora.forward(p['X'][sl], p['y'][sl], p['neg'][s])
                st = dict(loss=ora.eval_loss(p['X'][sl], p['y'][sl], p['neg'][s]), rowloss=f['loss'], Re=ora.R_e.copy())
            st.update({k: f[k] for k in ('a', 't', 'p', 'u', 'sig', 'cand')})
            for a in st.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            steps.append(st)
        _refs[key] = steps
    return _refs[key]


def surely_clipped(st64):
    """Units of one step whose t is above the clip bound whoever computes it: |a| >= SURE_A on the float64 oracle."""
    return np.abs(st64['a']) >= SURE_A


def last_candidate_twice(cand):
    """The candidates a twelve-slot body WITHOUT the mask of its idle slot would count: candidate z once more."""
    return np.concatenate([cand, cand[:, -1:]], axis=1)
