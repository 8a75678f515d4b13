"""-m gpu: the fold-in step at every key structure, kernel instance and upload route of tests/foldin_key_cases.py, against the
oracle twin of tests/foldin_cases.py.  What every step launched is asked of the handle (FoldIn.plan, sert_debug_foldin_plan):
a case that a moved dispatch threshold takes off its kernels fails here by name instead of passing for the wrong reason.
The gradient itself is checked, not only what Adam makes of it: from zero moments the first moment after step 1 is
(1 - beta1) g, row by row against the float32 and the float64 twin; then E, m and v after step 2, whose plan differs from
step 1's.  tests/test_foldin_keys_inputs_cpu.py proves the inputs and that these bounds tell a dropped carry, a stale bound
or a shifted slab from a right step."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import foldin_cases as FC
from tests import foldin_key_cases as K
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own
_NO_PLAN = dict(loss='none', k=0, train=False, sort_bits=0, passes=0, vec=0, nch=0, col_passes=0, fixup='none', tiles=0)


def _engine(c):
    e = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=_MODEL_B, global_batch_size=_MODEL_B, window_size=c['n'],
                 vocab_size=c['Vw'], num_entities=c['Ve'], word_dim=c['dw'], entity_dim=c['de'], num_negatives=2, id_bytes=4,
                 device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=99)
    for which, key in ((C.T_RW, 'Rw'), (C.T_RE, 'Re'), (C.T_W, 'W'), (C.T_B, 'b')):
        e.set_tensor(which, c[key])
    return e


def _foldin(c, eng, lam=None):
    f = C.FoldIn(eng, c['E0'], c['B'], c['z'], c['lam'] if lam is None else lam, lr=c['lr'], seed=FC.SEED)
    assert f.plan() == _NO_PLAN, (c['name'], 'before the first step')
    f.upload(c['X'], c['y'], c['w_upload'])
    return f


def _state(f):
    return dict(E=f.get_rows(C.FOLDIN_ROWS), m=f.get_rows(C.FOLDIN_M), v=f.get_rows(C.FOLDIN_V))


def _check(label, got, r32, r64, keys):
    for key in keys:
        mult = 2 if key == 'v' else 1       # (a second moment: twice the row-wise bound, as tests/test_gpu_foldin.py)
        print(U.check_tensor('%s %s' % (label, key), got[key], r32[key], r64[key], row_tol32=mult * U.ROW_TOL32,
                             row_tol64=mult * U.ROW_TOL64))


# what is checked after each step: after step 1 the moments alone (from zero moments m = (1 - beta1) g: the gradient itself)
_CHECKED = {0: ('m', 'v'), 1: ('E', 'm', 'v')}


def _two_steps(c, f, refs=None):
    """Both steps of a case on a handle; the plan after each; where refs = (float32 run, float64 run) of the twin is given, the
    loss of each step against the float32 twin and the state behind it, every row, against both.
    -> [loss of step 0, of step 1], [state after step 0, after step 1]"""
    losses, states = [], []
    for s, b in enumerate(c['batches']):
        got = f.train_batch(b, c['neg'][s])
        plan = f.plan()
        assert plan == c['plan'], (c['name'], 'step', s, 'launched', plan, 'the case is there for', c['plan'])
        losses.append(got)
        states.append(_state(f))
        if refs is not None:
            ref = refs[0][s]['loss']
            print('%s step %d: loss %.7f twin %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
            _check('%s step %d' % (c['name'], s), states[s], refs[0][s], refs[1][s], _CHECKED[s])
    return np.asarray(losses, np.float32), states


@pytest.mark.parametrize('name', list(K.CASES))
def test_foldin_step_at_every_structure(hip_lib, name):
    """Per case, explicit negatives: the plan after every step is the stated one, and with it the case produces the events it
    claims; each loss within 1e-5 of the float32 twin; m and v after step 1 (from zero moments: the gradient itself), E, m and v
    after step 2, every row, against both twins; then an evaluation -- its loss against the twin on the device's rows, the
    loss entries of the plan rewritten, the gradient entries and the state left alone.

    Measured on the MI355X, worst row error against float64 over the 27 cases (the bound is 5e-5, twice that for v): m after
    step 1 6.0e-7 (loss_vector_d260), m after step 2 6.6e-7 (n255_d128), E after step 2 4.9e-6 (runs_wave_v1), v 1.3e-5 in
    every case -- the float32 twin's own distance from float64 (1 - beta2 in float32).  As a check of this test (not kept):
    with the final flush of foldin_chunk_reduce never writing a tail carry, every one of the 27 cases fails."""
    c = K.case_problem(name)
    r32, _ = K.case_reference(name, np.float32)
    r64, _ = K.case_reference(name, np.float64)
    if c['M'] >= K.SLAB:
        assert C.debug_gemm_route(C.GEMM_FORM_PLAIN, K.SLAB, c['de'], c['dw']).startswith('x3_'), 'the slab left the bf16 pipe'
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        assert f.num_batches() == c['M'] // c['B']
        _, states = _two_steps(c, f, (r32, r64))
        assert K.events_of(name, f.plan()) == K.events_of(name)
        tw = FC.FoldInTwin(c, E0=states[1]['E'])            # (evaluate the twin ON the device's rows)
        b = c['batches'][1]
        got, ref = f.eval_batch(b, c['eval_neg']), tw.eval_loss(b, c['eval_neg'])
        print('%s evaluation: loss %.7f twin %.7f' % (name, got, ref))
        assert abs(got - ref) <= 1e-5 * abs(ref), (name, got, ref)
        assert f.plan() == dict(c['plan'], train=False), (name, 'after an evaluation', f.plan())
        after = _state(f)
        assert all(U.same_bits(after[k], states[1][k]) for k in after) and f.get_step() == K.STEPS
    finally:
        f.close()
        eng.close()


def test_absent_rows_are_untouched_at_lambda_zero(hip_lib):
    """lambda = 0: a row that no pair of either step hit has a zero gradient in both steps, and a zero gradient gives a zero Adam
    update -- it keeps the bits of E0 and its moments are bit-zero.  A stale or stray row of G shows here in the last bit."""
    name = K.EXACT_CASE
    c = K.case_problem(name)
    refs = K.case_reference(name, np.float32, lam=0.0)[0], K.case_reference(name, np.float64, lam=0.0)[0]
    eng = _engine(c)
    f = _foldin(c, eng, lam=0.0)
    try:
        _, states = _two_steps(c, f, refs)
        hit = np.zeros(c['N'], bool)
        for s in range(K.STEPS):
            hit[np.unique(K.step_keys(name, s)[K.step_keys(name, s) < c['N']])] = True
        absent = np.nonzero(~hit)[0]
        assert len(absent) >= 10 and hit.sum() >= 10
        E, m, v = (states[1][k] for k in ('E', 'm', 'v'))
        zero = np.zeros((len(absent), c['de']), np.float32)
        assert U.same_bits(E[absent], c['E0'][absent]) and U.same_bits(m[absent], zero) and U.same_bits(v[absent], zero)
        assert np.all(np.abs(m[hit]).max(axis=1) > 0)
    finally:
        f.close()
        eng.close()


def test_multi_tile_two_pass_case_is_reproducible(hip_lib):
    """The case with several sort tiles and two sort passes, run on two handles: the same bits."""
    c = K.case_problem(K.REPRO_CASE)
    eng = _engine(c)
    try:
        runs = []
        for _ in range(2):
            f = _foldin(c, eng)
            losses, states = _two_steps(c, f)
            f.close()
            runs.append([losses] + [st[k] for st in states for k in ('E', 'm', 'v')])
        for a, b in zip(*runs):
            assert U.same_bits(a, b)
    finally:
        eng.close()
