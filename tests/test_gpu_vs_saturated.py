"""-m gpu: vectorspace steps where tanh and the sigmoid saturate, against the FLOAT32 oracle.

Every other vectorspace test starts from Glorot-uniform parameters: the projection a = h.W + b and the scores
u = <R_e[c], clip(t)> stay O(1), so neither the clip of t, nor the clip of sigmoid(u) / Theano's sigmoid cut-offs, nor
any of their gradient masks is ever active.  Here the problems of make_vs_problem are rescaled (saturate_vs /
saturate_fs below: scores over about +-100, two of every three columns of a with a standard deviation of 6) and a few
EXACT values are planted, so that the inclusive bounds are met exactly and not only statistically.

The clip decisions are float32 decisions (the float64 oracle has other bounds, clip_bounds(float64)): the float32
oracle is the only comparator, as in test_loglinear_with_saturated_probabilities.  Each problem proves ON THE ORACLE,
before every step, that its inputs are decidable (check_vs_inputs / check_fs_inputs; the same functions run without a
GPU in tests/test_vs_saturated_inputs_cpu.py):
  * err = max |u32 - u64|, u64 the float64 dot product of the oracle's float32 R_e rows and float32 p -- measured on
    the reference, never on the engine; every score is at least 10 err away from both decision points of the sigmoid
    mask, u = 15 (Theano's cut-off; sigmoid(15) < 1 - 2^-23, so the cut-off IS the upper bound) and u = logit(1e-7).
    The factor 10 is there because the engine sums in another order.  Only candidates whose entity row has a single
    non-zero element are exempt: their score is ONE rounded product in any summation order (the planted rows).
  * shares over the three steps: >= 5 % of the candidates above the upper bound, >= 5 % below the lower one, >= 5 %
    inside; >= 1 % of the elements of t outside the clip, >= 30 % inside.
These are conditions on the inputs: a failing one fails the test.

The band 7.9 < |a| < 9.1 is NOT excluded: there float32 tanh lands on 1 - 2^-23, 1 - 2^-24 or 1, the engine's
fast_tanh may differ from np.tanh by one unit in the last place and the mask [|t| <= 1 - 2^-23] may then differ for
that element.  Its da changes by at most (1 - t^2) |dp| <= 2.4e-7 |dp|, below every tolerance, since max |da| comes
from the columns left at their Glorot scale.

Plants (vectorspace; row 0 of the first batch, exact at step 0 only -- Adam moves the parameters afterwards):
  * word W0 has the embedding e_0 and fills the window of row 0, so h = e_0 and a[0, c] = W[0, c] + b[c] in one
    rounding: a = -20 (t = -1 exactly), a = 0 (t = 0) and a = 12 ln 2, where tanh is 1 - 2^-23 = the bound itself in
    np.tanh and in fast_tanh (1 - t = 2^-23 (1 +- 1e-6) sits half a spacing away from either neighbour) -- the one
    element that tells `<=` from `<` in the t mask.  Column C0 is +20 for EVERY row (W[:, C0] = 0, b[C0] = 20, and
    stays so: its da is masked, so dW and db are exactly 0 there).
  * the scores are planted through R_e against the already clipped p[C0] = hi = 1 - 2^-23 (an exact u is not
    reachable through tanh itself): the entity rows E16 / E15 / ELO are zero but for column C0, where they hold
    16 + 2^-19, 15 + 2^-19 and -(17 + 2^-19), whose products with hi round to exactly 16, 15 and -17.
    u = 15.0 is INSIDE (x > 15 is false and sigmoid(15) < hi); u = 16 is outside, du = 0; u = -17 is below the
    lower bound (sigmoid = 4.1e-8), du = 0 -- as the TARGET of row 0, where a mask applied to the clipped s would
    leave du = -g sigmoid / 1e-7 = -0.41 g.  E16 and ELO meet nothing but clipped candidates wherever they are
    drawn, at every step: their gradient rows must be exactly the L2 term.  E15 is a candidate of the planted row
    only (random draws of it are redirected), its gradient row is du p_0 + the L2 term.
"""
import functools

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import util as U

pytestmark = pytest.mark.gpu

LOSS_TOL, ACT_TOL, GRAD_TOL, PARAM_TOL = 1e-5, 2e-5, 1e-4, 1e-4      # tests/test_gpu_parity.py, unchanged
LAM, STEPS = 0.01, 3
LO, HI = O.clip_bounds(np.float32)
A_HI = np.float32(12.0 * np.log(2.0))        # tanh(A_HI) = 1 - 2^-23 in float32
X16, X15, X17 = np.float32(16 + 2.0 ** -19), np.float32(15 + 2.0 ** -19), np.float32(17 + 2.0 ** -19)
E16, E15, ELO = 0, 1, 2                       # planted entity ids (ELO only where V_e >= 5)
LOGIT_LO = float(np.log(np.float64(LO)) - np.log1p(-np.float64(LO)))

# the smallest shapes that reach each form of the NCE kernel (csrc/host/step_vectorspace.inc) and both entity-gradient
# paths; `seed` picked on the CPU so that every input condition holds at all three steps
VS_SAT = {
    'regs_1x6': dict(B=64, n=5, z=4, Vw=500, Ve=37, dw=32, de=48, seed=1),
    'regs_2x12_ragged': dict(B=70, n=3, z=10, Vw=300, Ve=300, dw=16, de=128, seed=3),
    'regs_4x6': dict(B=48, n=2, z=5, Vw=100, Ve=9, dw=8, de=256, seed=1),
    'per_candidate_1': dict(B=80, n=2, z=20, Vw=50, Ve=3, dw=8, de=32, seed=2),
    'per_candidate_5': dict(B=48, n=4, z=10, Vw=300, Ve=300, dw=16, de=300, seed=1),
    'scalar_2': dict(B=96, n=3, z=7, Vw=200, Ve=11, dw=30, de=70, seed=2),
    'sorted_chain': dict(B=300, n=2, z=5, Vw=300, Ve=5000, dw=16, de=32, seed=3),
}
# V_e = 37: fs_softmax_ce<., 16>; 1500: <., 32>; 3000: the streaming form; tile: SERT_FS_TILE_ROWS (ragged last tile)
FS_SAT = {
    'epl16': dict(B=64, n=5, Vw=500, Ve=37, dw=32, de=48, tile=None, seed=1),
    'epl32': dict(B=96, n=3, Vw=200, Ve=1500, dw=30, de=68, tile=None, seed=1),
    'epl32_tile40': dict(B=96, n=3, Vw=200, Ve=1500, dw=30, de=68, tile=40, seed=1),
    'streaming': dict(B=48, n=4, Vw=300, Ve=3000, dw=16, de=64, tile=None, seed=1),
}


def plant_columns(de):
    """(C0, C1, C2, C3): the always-saturated column and the columns of a = -20, 0, 12 ln 2 in the planted row --
    the first and the last lanes / chunks of a row."""
    return 0, de - 1, 1, de - 2


def _project(p, rows):
    h = (p['Rw'][p['X'][rows].astype(np.int64)].sum(axis=1, dtype=np.float64) / p['X'].shape[1]).astype(np.float32)
    return np.clip(np.tanh(h @ p['W'] + p['b']), -HI, HI), h


def _scale_projection(p, B):
    """Two of every three columns of W times sW, chosen from the oracle's own first batch so that those columns of a
    get a standard deviation of 6; every third column stays at its Glorot scale (live units set max |da|)."""
    scaled = np.arange(p['W'].shape[1]) % 3 != 2
    _, h = _project(p, slice(0, B))
    sW = float(np.round(6.0 / (h @ p['W'])[:, scaled].std()))           # (b is not scaled)
    p['W'][:, scaled] *= np.float32(sW)
    p['sW'] = sW


def _plant_projection(p, sat_value):
    """Row 0 of the data set: h = e_0, a[0, C1] = -|sat_value|, a[0, C2] = 0, a[0, C3] = 12 ln 2."""
    Vw, de = p['Rw'].shape[0], p['W'].shape[1]
    c0, c1, c2, c3 = plant_columns(de)
    w0 = Vw - 1
    p['Rw'][w0] = 0
    p['Rw'][w0, 0] = 1
    p['X'][0, :] = w0
    for c, v in ((c1, -sat_value), (c2, 0.0), (c3, A_HI)):
        p['W'][0, c] = v
        p['b'][c] = 0


def saturate_vs(dims):
    B, n, z, Ve, de = dims['B'], dims['n'], dims['z'], dims['Ve'], dims['de']
    p = U.make_vs_problem(dims['seed'], B * STEPS, n, z, dims['Vw'], Ve, dims['dw'], de, zipf=True)
    _scale_projection(p, B)
    p0, _ = _project(p, slice(0, B))
    p['sE'] = float(np.round(30.0 / (p0.astype(np.float64) @ p['Re'].astype(np.float64).T).std()))
    p['Re'] *= np.float32(p['sE'])
    # plants
    c0 = plant_columns(de)[0]
    _plant_projection(p, 20.0)
    p['W'][:, c0] = 0
    p['b'][c0] = 20
    planted = [(E16, X16), (E15, X15)] + ([(ELO, -X17)] if Ve >= 5 else [])
    for e, x in planted:
        p['Re'][e] = 0
        p['Re'][e, c0] = x
    assert X16 * HI == 16 and X15 * HI == 15 and X17 * HI == 17          # (float32 products: one rounding)
    p['negs'] = [p['rng'].randint(0, Ve, size=(B, z)).astype(np.int64) for _ in range(STEPS)]
    p['y'][p['y'] == E15] = Ve - 1                 # E15 is a candidate of the planted row only
    for neg in p['negs']:
        neg[neg == E15] = Ve - 1
    p['negs'][0][0, 0], p['negs'][0][0, 1] = E15, E16
    if Ve >= 5:
        p['y'][0] = ELO
    p['planted_entities'] = [e for e, _ in planted]
    return p


def check_vs_inputs(ora, f, row_losses=True):
    """The decidability figures of one step, from the oracle's forward pass `f`: (err, margin at 15, margin at
    logit(1e-7)).  Candidates whose entity row has exactly one non-zero element are exempt (one rounded product)."""
    E = ora.R_e[f['cand']]
    u64 = np.einsum('bcd,bd->bc', E.astype(np.float64), f['p'].astype(np.float64))
    err = float(np.abs(f['u'].astype(np.float64) - u64).max())
    free = (np.count_nonzero(ora.R_e, axis=1) != 1)[f['cand']]
    m15 = float(np.abs(u64[free] - 15.0).min())
    mlo = float(np.abs(u64[free] - LOGIT_LO).min())
    assert m15 >= 10 * err and mlo >= 10 * err, ('a score within 10 err of a decision point', err, m15, mlo)
    # ... and the reference's own error bar on the row losses.  For 10 < u < 15 float32 holds 1 - sigmoid(u) in a handful
    # of steps of 2^-24 (1 + exp(-u) rounds to a multiple of 2^-23 first), so log(1 - s) jumps by up to 2^-24 / (1 - s)
    # -- 1.5e-3 at u = 10 -- when u crosses the preimage of a rounding boundary.  A row whose oracle value moves by more
    # than half the row-loss tolerance when every score moves by its own float32 error cannot be checked at that
    # tolerance against ANY other summation order: such a problem (seed) is not used.
    # (row_losses=False: where only the batch mean is compared -- the device's own negatives cannot be picked)
    if not row_losses:
        return err, m15, mlo
    lo, hi = LO, HI
    wobble = 0.0
    for sign in (-1.0, 1.0):
        sig = O.theano_sigmoid((f['u'].astype(np.float64) + sign * err * free).astype(np.float32))     # (exact plants stay)
        s = np.clip(sig, lo, hi)
        alt = -(np.log(s[:, 0]).astype(np.float64) + np.log(np.float32(1) - s[:, 1:]).astype(np.float64).sum(axis=1))
        base = f['loss'].astype(np.float64)
        wobble = max(wobble, float((np.abs(alt - base) / np.maximum(np.abs(base), 1e-3 * np.abs(base).mean())).max()))
    assert wobble < 0.5 * ACT_TOL, ('the float32 oracle\'s own row losses move by', wobble, 'under its own error of the scores', err)
    return err, m15, mlo


class Run(object):
    pass


@functools.lru_cache(maxsize=None)
def vs_reference(name):
    """The saturated problem `name`, its three float32 oracle steps (per step: loss, gradients, forward values) and
    the oracle after them -- computed once, shared by every test of the problem and never modified."""
    dims = VS_SAT[name]
    B, n, z, de = dims['B'], dims['n'], dims['z'], dims['de']
    p = saturate_vs(dims)
    ora = O.VectorSpaceOracle(B, n, z, p['Rw'], p['Re'], p['W'], p['b'], LAM)
    r = Run()
    r.dims, r.p, r.ora, r.steps, r.figures = dims, p, ora, [], []
    above = below = inside = cands = t_out = t_in = t_all = 0
    c0, c1, c2, c3 = plant_columns(de)
    for s in range(STEPS):
        sl = slice(s * B, (s + 1) * B)
        l2_rows = {e: (np.float32(LAM) / np.float32(B)) * ora.R_e[e] for e in p['planted_entities']}
        loss, grads, f = ora.loss_and_grads(p['X'][sl], p['y'][sl], p['w'][sl], p['negs'][s])
        r.figures.append(check_vs_inputs(ora, f))
        above += int((f['sig'] > HI).sum())
        below += int((f['sig'] < LO).sum())
        inside += int(((f['sig'] >= LO) & (f['sig'] <= HI)).sum())
        cands += f['sig'].size
        t_out += int((np.abs(f['t']) > HI).sum())
        t_in += int((np.abs(f['t']) <= HI).sum())
        t_all += f['t'].size
        assert np.all(np.isfinite(loss)) and all(np.all(np.isfinite(g)) for g in grads)
        # E16 / ELO: clipped wherever they are candidates, at every step -> the L2 term, bit for bit
        for e in p['planted_entities']:
            if e != E15:
                assert np.all(f['du'][f['cand'] == e] == 0) and np.array_equal(grads[0][e], l2_rows[e]), (s, e)
        if s == 0:
            t0, u0, du0 = f['t'][0], f['u'][0], f['du'][0]
            assert t0[c0] == 1 and t0[c1] == -1 and t0[c2] == 0 and t0[c3] == HI, t0[[c0, c1, c2, c3]]
            assert np.all(f['t'][:, c0] == 1)
            assert u0[1] == 15 and u0[2] == 16 and du0[1] > 0 and du0[2] == 0, (u0[:3], du0[:3])
            if ELO in p['planted_entities']:
                assert u0[0] == -17 and du0[0] == 0 and 0 < f['sig'][0, 0] < LO
            assert (f['cand'] == E15).sum() == 1
            assert grads[0][E15, c1] == -grads[0][E15, c3] != 0
            # the planted row's live elements really carry a gradient (else the exact-bound plant shows nothing)
            assert f['da'][0, c0] == 0 and f['da'][0, c1] == 0 and f['da'][0, c2] != 0 and f['da'][0, c3] != 0
        else:
            assert not (f['cand'] == E15).any()
        r.steps.append(dict(loss=loss, grads=[g.copy() for g in grads], l2_rows=l2_rows, Re0=ora.R_e.copy() if s == 0 else None,
                            f={k: f[k].copy() for k in ('h', 't', 'da', 'dh', 'loss', 'cand', 'du', 'p')}))
        ora.opt.update(ora.params(), grads)
    r.shares = dict(above=above / cands, below=below / cands, inside=inside / cands, t_out=t_out / t_all, t_in=t_in / t_all)
    assert min(r.shares['above'], r.shares['below'], r.shares['inside']) >= 0.05, r.shares
    assert r.shares['t_out'] >= 0.01 and r.shares['t_in'] >= 0.30, r.shares
    return r


def _engine_on(p, dims, keep, lam=LAM):
    eng = U.vs_engine(p, dims['B'], dims['n'], dims['z'], lam, keep_grads=keep)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    return eng


def _check_rowloss(eng, f, w):                   # (tests/test_gpu_parity.py)
    ref = np.asarray(w, np.float64) * np.asarray(f['loss'], np.float64)
    got = eng.get_tensor(C.T_ACT_ROWLOSS, ref.shape)
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).mean())
    assert err.max() < ACT_TOL, ('row loss', int(err.argmax()), float(err.max()), got[err.argmax()], ref[err.argmax()])


@pytest.mark.parametrize('egrad', ['default', 'sorted'])
@pytest.mark.parametrize('name', list(VS_SAT))
def test_saturated_vectorspace_steps(hip_lib, name, egrad, monkeypatch):
    """keep_grads = 1: after each of three steps the loss, the row losses, t, da, dh and all four gradients; at step 0
    the planted elements (module docstring) bit for bit."""
    if egrad == 'sorted':
        monkeypatch.setenv('SERT_EGRAD_SORT', '1')
    r = vs_reference(name)
    d, p = r.dims, r.p
    B, de, dw = d['B'], d['de'], d['dw']
    c0, c1, c2, c3 = plant_columns(de)
    eng = _engine_on(p, d, keep=1)
    for s, st in enumerate(r.steps):
        f = st['f']
        loss = eng.train_batch(s, p['negs'][s])
        print('%s step %d: loss %.6f (oracle %.6f)  err %.1e  margins %.1e %.1e' % ((name, s, loss, st['loss']) + r.figures[s]))
        assert abs(loss - st['loss']) <= LOSS_TOL * abs(st['loss']), (s, loss, st['loss'])
        _check_rowloss(eng, f, p['w'][s * B:(s + 1) * B])
        T = eng.get_tensor(C.T_ACT_T, (B, de))
        DA = eng.get_tensor(C.T_ACT_DA, (B, de))
        assert U.rel_err(T, f['t']) < ACT_TOL
        assert U.rel_err(DA, f['da']) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_ACT_DH, (B, dw)), f['dh']) < GRAD_TOL
        dRe, dRw, dW, db = st['grads']
        gRe = eng.get_tensor(C.T_GRAD_RE, dRe.shape)
        assert U.rel_err(gRe, dRe) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_GRAD_RW), dRw.ravel()) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_GRAD_W), dW.ravel()) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_GRAD_B), db.ravel()) < GRAD_TOL
        # entities that meet clipped candidates only: the L2 term and nothing else, bit for bit
        for e in p['planted_entities']:
            if e != E15:
                assert np.array_equal(gRe[e], st['l2_rows'][e]), (s, e, gRe[e][c0], st['l2_rows'][e][c0], np.abs(gRe[e]).max())
        # the always-saturated column: masked for every row
        assert np.all(T[:, c0] == 1) and np.all(DA[:, c0] == 0)
        if s == 0:
            cols = [c0, c1, c2, c3]
            assert np.array_equal(T[0, cols], f['t'][0, cols]), (T[0, cols], f['t'][0, cols])     # 1, -1, 0, 1 - 2^-23
            assert DA[0, c1] == 0                                                          # |t| = 1: outside
            # t = 1 - 2^-23 is INSIDE (and t = 0): da = dp (1 - t^2), priced against the sum of its terms' magnitudes
            terms = np.abs(f['du'][0][:, None] * r.steps[0]['Re0'][f['cand'][0]][:, [c2, c3]]).sum(axis=0)
            for k, c in enumerate((c2, c3)):
                bound = GRAD_TOL * terms[k] * (1.0 - float(f['t'][0, c]) ** 2)
                assert DA[0, c] != 0 and abs(DA[0, c] - f['da'][0, c]) <= bound, (c, DA[0, c], f['da'][0, c], bound)
            # the clip of t INSIDE the entity-gradient kernels (kernels_egrad.h re-clips t): row 0 is E15's only pair,
            # p_0[C1] = -hi (t = -1, clipped) and p_0[C3] = hi (t on the bound), R_e[E15] is 0 in both columns: the two
            # gradient elements are du (-hi) and du hi, the same bits but for the sign -- du (-1) without the clip
            assert gRe[E15, c1] == -gRe[E15, c3] and gRe[E15, c3] != 0, (gRe[E15, c1], gRe[E15, c3])
            # E15 (u = 15.0, inside): its gradient row is du p_0 + the L2 term
            err15, _ = U.row_err(gRe, dRe, rows=[E15])
            assert err15 < GRAD_TOL, ('gradient row of the u = 15 entity', err15, gRe[E15][:4], dRe[E15][:4])
    assert U.rel_err(eng.get_tensor(C.T_RW), r.ora.R_w.ravel()) < PARAM_TOL
    assert U.rel_err(eng.get_tensor(C.T_RE), r.ora.R_e.ravel()) < PARAM_TOL
    assert U.rel_err(eng.get_tensor(C.T_W), r.ora.W.ravel()) < PARAM_TOL
    assert U.rel_err(eng.get_tensor(C.T_B), r.ora.b.ravel()) < PARAM_TOL
    eng.close()


@pytest.mark.parametrize('egrad', ['default', 'sorted'])
@pytest.mark.parametrize('name', list(VS_SAT))
def test_saturated_vectorspace_steps_product_path(hip_lib, name, egrad, monkeypatch):
    """keep_grads = 0: nothing is read until the last step; then every step's loss and the whole state (parameters,
    m, v) against the float32 oracle."""
    if egrad == 'sorted':
        monkeypatch.setenv('SERT_EGRAD_SORT', '1')
    r = vs_reference(name)
    eng = _engine_on(r.p, r.dims, keep=0)
    losses = [eng.train_batch(s, r.p['negs'][s]) for s in range(STEPS)]
    for s, st in enumerate(r.steps):
        assert abs(losses[s] - st['loss']) <= LOSS_TOL * abs(st['loss']), (s, losses[s], st['loss'])
    print('\n'.join(U.check_state(U.engine_state(eng), U.oracle_state(r.ora))))
    eng.close()


@pytest.mark.parametrize('name', ['regs_1x6', 'scalar_2'])
def test_saturated_vectorspace_evaluation(hip_lib, name):
    """The TRAIN = false instantiations on saturated inputs: eval_batch with explicit negatives against ora.eval_loss,
    eval_batches against a loop of eval_batch, and the training path with the device's own negatives (read back with
    sert_negatives_of_step and fed to the oracle)."""
    r = vs_reference(name)
    d, p = r.dims, r.p
    B, n, z = d['B'], d['n'], d['z']
    ora = O.VectorSpaceOracle(B, n, z, p['Rw'], p['Re'], p['W'], p['b'], LAM)      # (the initial parameters)
    eng = _engine_on(p, d, keep=0)
    for s in range(STEPS):
        sl = slice(s * B, (s + 1) * B)
        ref = ora.eval_loss(p['X'][sl], p['y'][sl], p['negs'][s])
        got = eng.eval_batch(C.SPLIT_TRAIN, s, p['negs'][s])
        assert abs(got - ref) <= LOSS_TOL * abs(ref), (s, got, ref)
    # device-drawn evaluation negatives: the loop and the batched call see the same draws from the same counter
    first = eng.get_eval_draws()
    loop = np.array([eng.eval_batch(C.SPLIT_TRAIN, s) for s in (2, 0, 1)], np.float32)
    for k, s in enumerate((2, 0, 1)):
        neg = eng.negatives_of_step(first + k, evaluation=True)
        check_vs_inputs(ora, ora.forward(p['X'][s * B:(s + 1) * B], p['y'][s * B:(s + 1) * B], neg), row_losses=False)
        ref = ora.eval_loss(p['X'][s * B:(s + 1) * B], p['y'][s * B:(s + 1) * B], neg)
        assert abs(loop[k] - ref) <= LOSS_TOL * abs(ref), (s, loop[k], ref)
    eng.set_eval_draws(first)
    assert np.array_equal(eng.eval_batches(C.SPLIT_TRAIN, [2, 0, 1]), loop)
    # a training step with the device's own negatives
    neg = eng.negatives_of_step(eng.get_step())
    check_vs_inputs(ora, ora.forward(p['X'][:B], p['y'][:B], neg), row_losses=False)
    ref, _, _ = ora.loss_and_grads(p['X'][:B], p['y'][:B], p['w'][:B], neg)
    got = eng.train_batch(0)
    assert abs(got - ref) <= LOSS_TOL * abs(ref), (got, ref)
    eng.close()


# --------------------------------------------------------------------------- #
# the additive full-softmax variant
# --------------------------------------------------------------------------- #
EBIG, ZBIG = 0, np.float32(400.0)


def saturate_fs(dims):
    """The same rescaling for SERT_KIND_VECTORSPACE_SOFTMAX; sE such that about 40 % of the first batch's rows have
    P[y] < 1e-7 (the rest carries the gradient).  Plants: the projection plants of the vectorspace problems in row 0
    (a = -10 in column C1 for that row alone, +10 - 20 h_0 > 0 elsewhere), and P[y] > 1 - 2^-23 for row 0: its label
    EBIG has the entity row -400 e_C1, a logit of +400 for row 0 (P[y] = 1.0 in float32) and about -400 for the rows
    whose C1 unit saturates at +1."""
    B, n, Ve, de = dims['B'], dims['n'], dims['Ve'], dims['de']
    p = U.make_vs_problem(dims['seed'], B * STEPS, n, 0, dims['Vw'], Ve, dims['dw'], de, zipf=True)
    _scale_projection(p, B)
    p0, _ = _project(p, slice(0, B))
    Z0 = p0.astype(np.float64) @ p['Re'].astype(np.float64).T
    y0 = p['y'][:B].astype(np.int64)

    def share(sE):
        Z = sE * Z0
        m = Z.max(axis=1)
        lp = Z[np.arange(B), y0] - m - np.log(np.exp(Z - m[:, None]).sum(axis=1))
        return (lp < np.log(1e-7)).mean()
    p['sE'] = float(min(range(1, 400), key=lambda sE: (abs(share(sE) - 0.4), sE)))
    p['Re'] *= np.float32(p['sE'])
    c0, c1, c2, c3 = plant_columns(de)
    _plant_projection(p, 20.0)
    p['W'][:, c1] = 0
    p['W'][0, c1] = -20
    p['b'][c1] = 10
    p['Re'][EBIG] = 0
    p['Re'][EBIG, c1] = -ZBIG
    p['y'][0] = EBIG
    return p


def check_fs_inputs(ora, f, y):
    """(err, margin at the lower bound, margin at the upper bound), log domain.  err = max |Z32 - Z64| on the oracle.
    P[y] < 1e-7 is decided by log P[y] = z_y - logsumexp(z) against log(1e-7); P[y] > 1 - 2^-23 means the float32
    quotient is 1 - 2^-24 or 1, i.e. the sum delta of the OTHER entities' exp(z_j - z_y) stays below 2^-24 (at
    2^-24 < delta < 3 * 2^-24 the float32 row sum is 1 + 2^-23 and P[y] = 1 - 2^-23, inside): log(delta) against
    log(2^-24).  Both at least 10 err away."""
    B = len(y)
    Z64 = f['p'].astype(np.float64) @ ora.R_e.astype(np.float64).T
    err = float(np.abs(f['Z'].astype(np.float64) - Z64).max())
    zy = Z64[np.arange(B), y]
    m = Z64.max(axis=1)
    lse = m + np.log(np.exp(Z64 - m[:, None]).sum(axis=1))
    others = Z64.copy()
    others[np.arange(B), y] = -np.inf
    mo = others.max(axis=1)
    ldelta = mo + np.log(np.exp(others - mo[:, None]).sum(axis=1)) - zy
    mlo = float(np.abs(zy - lse - np.log(np.float64(LO))).min())
    mhi = float(np.abs(ldelta - np.log(2.0 ** -24)).min())
    assert mlo >= 10 * err and mhi >= 10 * err, ('P[y] within 10 err of a bound', err, mlo, mhi)
    return err, mlo, mhi


@functools.lru_cache(maxsize=None)
def fs_reference(problem):
    """(B, n, Vw, Ve, dw, de, seed) -> the saturated softmax problem and its three float32 oracle steps."""
    dims = dict(zip(('B', 'n', 'Vw', 'Ve', 'dw', 'de', 'seed'), problem))
    B, n = dims['B'], dims['n']
    p = saturate_fs(dims)
    ora = O.VectorSpaceSoftmaxOracle(B, n, p['Rw'], p['Re'], p['W'], p['b'], LAM)
    r = Run()
    r.dims, r.p, r.ora, r.steps, r.figures = dims, p, ora, [], []
    below = inside = 0
    c0, c1, c2, c3 = plant_columns(dims['de'])
    for s in range(STEPS):
        sl = slice(s * B, (s + 1) * B)
        y = p['y'][sl].astype(np.int64)
        loss, grads, f = ora.loss_and_grads(p['X'][sl], p['y'][sl], p['w'][sl])
        r.figures.append(check_fs_inputs(ora, f, y))
        below += int((f['py'] < LO).sum())
        inside += int(((f['py'] >= LO) & (f['py'] <= HI)).sum())
        assert np.all(np.isfinite(loss)) and all(np.all(np.isfinite(g)) for g in grads)
        dead = (f['py'] < LO) | (f['py'] > HI)
        assert not f['dZ'][dead].any() and not f['da'][dead].any() and not f['dh'][dead].any()
        if s == 0:
            t0 = f['t'][0]
            assert t0[c1] == -1 and t0[c2] == 0 and t0[c3] == HI, t0[[c1, c2, c3]]
            assert f['py'][0] == 1.0 and dead[0]
            # ... and an inside row whose C3-like bound element exists is not needed here: vs_tanh_backward's
            # inclusive bound is met by every element of t that equals 1 - 2^-23 in a live row
            live_hi = (np.abs(f['t']) == HI) & ~dead[:, None] & (f['da'] != 0)
            assert live_hi.any(), 'no element with |t| = 1 - 2^-23 and a gradient'
        r.steps.append(dict(loss=loss, grads=[g.copy() for g in grads], dead=dead,
                            f={k: f[k].copy() for k in ('t', 'da', 'dh', 'loss', 'py')}))
        ora.opt.update(ora.params(), grads)
    r.shares = dict(below=below / (B * STEPS), inside=inside / (B * STEPS))
    assert r.shares['below'] >= 0.05 and r.shares['inside'] >= 0.05, r.shares
    return r


def fs_key(name):
    d = FS_SAT[name]
    return tuple(d[k] for k in ('B', 'n', 'Vw', 'Ve', 'dw', 'de', 'seed'))


@pytest.mark.parametrize('keep', [1, 0])
@pytest.mark.parametrize('name', list(FS_SAT))
def test_saturated_softmax_variant_steps(hip_lib, name, keep, monkeypatch):
    """Three steps of the additive full-softmax variant against VectorSpaceSoftmaxOracle (float32): vs_clip,
    fs_softmax_ce in its three forms and with row tiles, vs_tanh_backward.  Rows whose P[y] is clipped (below 1e-7, or
    above 1 - 2^-23: the planted row 0) have a zero row of dZ: their rows of da and dh are exactly zero.  Elements of
    t that sit exactly ON the bound 1 - 2^-23 in a live row keep their gradient (inclusive mask)."""
    tile = FS_SAT[name]['tile']
    if tile:
        monkeypatch.setenv('SERT_FS_TILE_ROWS', str(tile))
    r = fs_reference(fs_key(name))
    d, p = r.dims, r.p
    B, de, dw = d['B'], d['de'], d['dw']
    eng = C.Engine(kind=C.KIND_VECTORSPACE_SOFTMAX, batch_size=B, global_batch_size=B, window_size=d['n'],
                   vocab_size=d['Vw'], num_entities=d['Ve'], word_dim=dw, entity_dim=de, num_negatives=0,
                   id_bytes=p['X'].dtype.itemsize, device=0, keep_grads=keep, deterministic=1, lambda_=LAM, lr=1e-3,
                   beta1=0.9, beta2=0.999, eps=1e-8, seed=1)
    for which, a in ((C.T_RW, p['Rw']), (C.T_RE, p['Re']), (C.T_W, p['W']), (C.T_B, p['b'])):
        eng.set_tensor(which, a)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    for s, st in enumerate(r.steps):
        f = st['f']
        loss = eng.train_batch(s)
        print('%s step %d: loss %.6f (oracle %.6f)  err %.1e  margins %.1e %.1e' % ((name, s, loss, st['loss']) + r.figures[s]))
        assert abs(loss - st['loss']) <= LOSS_TOL * abs(st['loss']), (s, loss, st['loss'])
        if not keep:
            continue
        _check_rowloss(eng, f, p['w'][s * B:(s + 1) * B])
        T = eng.get_tensor(C.T_ACT_T, (B, de))
        DA = eng.get_tensor(C.T_ACT_DA, (B, de))
        DH = eng.get_tensor(C.T_ACT_DH, (B, dw))
        assert U.rel_err(T, f['t']) < ACT_TOL
        assert U.rel_err(DA, f['da']) < GRAD_TOL
        assert U.rel_err(DH, f['dh']) < GRAD_TOL
        assert not DA[st['dead']].any() and not DH[st['dead']].any(), 'a clipped row of P[y] has a gradient'
        # |t| exactly on the bound, same bits on both sides, live row: the gradient is there (dp (1 - t^2), ~2.4e-7 dp)
        on = (np.abs(f['t']) == HI) & (np.abs(T) == HI) & ~st['dead'][:, None] & (f['da'] != 0)
        if s == 0:
            assert on.any()
        assert np.all(DA[on] != 0)
        assert np.all(np.abs(DA[on] - f['da'][on]) <= 1e-2 * np.abs(f['da'][on])), (DA[on], f['da'][on])
        dRe, dRw, dW, db = st['grads']
        assert U.rel_err(eng.get_tensor(C.T_GRAD_RE), dRe.ravel()) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_GRAD_RW), dRw.ravel()) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_GRAD_W), dW.ravel()) < GRAD_TOL
        assert U.rel_err(eng.get_tensor(C.T_GRAD_B), db.ravel()) < GRAD_TOL
    assert U.rel_err(eng.get_tensor(C.T_RW), r.ora.R_w.ravel()) < PARAM_TOL
    assert U.rel_err(eng.get_tensor(C.T_RE), r.ora.R_e.ravel()) < PARAM_TOL
    if not keep:
        print('\n'.join(U.check_state(U.engine_state(eng), U.oracle_state(r.ora))))
    eng.close()
