"""-m gpu: the tail of a hinted vectorspace step inside the next batch's gather launch.

A single-GPU vectorspace step ends with one launch (vs_tail: the split-K combine of dW / db, Adam on W and b, the loss).  A
step whose next batch was announced (sert_hint_next_batch) leaves that launch out: its workgroups lead the gather launch of
the run-ahead step (vs_gather_mean_tail).  Nothing but the schedule may change -- every comparison below is BIT for bit --
and the host counters of sert_debug_tail_counts say which form ran."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import util as U

pytestmark = pytest.mark.gpu

STATE = [C.T_RW, C.T_RE, C.T_W, C.T_B,
         C.T_STATE0_RW, C.T_STATE0_RE, C.T_STATE0_W, C.T_STATE0_B,
         C.T_STATE1_RW, C.T_STATE1_RE, C.T_STATE1_W, C.T_STATE1_B]


def run(p, dims, order, hints, keep_grads=0, timing=0):
    """Train the batches of `order`; hints[i] is announced in front of step i (None: nothing).  Returns the per-step losses
    (bit patterns), parameters + both moment tensors, and the tail counters."""
    eng = U.vs_engine(p, dims['B'], dims['n'], dims['z'], 0.01, keep_grads=keep_grads)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    if timing:
        eng.timing_enable(timing)
    losses = []
    for b, h in zip(order, hints):
        if h is not None:
            eng.hint_next_batch(h)
        losses.append(np.float32(eng.train_batch(b)))
    eng.synchronize()
    if timing:
        eng.timing_enable(0)
    state = [eng.get_tensor(t).copy() for t in STATE]
    counts = eng.tail_counts()
    eng.close()
    return np.array(losses, dtype=np.float32).view(np.uint32), state, counts


def assert_same(a, b):
    assert np.array_equal(a[0], b[0]), (a[0], b[0])
    assert np.all(np.isfinite(a[0].view(np.float32)))
    for t, x, y in zip(STATE, a[1], b[1]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), t


def right_hints(order):
    return [order[i + 1] if i + 1 < len(order) else None for i in range(len(order))]


FOLD_DIMS = [
    # C2's dimensions at 8192 rows (the bench's small_batch record)
    (dict(B=8192, n=10, z=10, Vw=100000, Ve=1000, dw=128, de=128), 3, [0, 1, 2, 0, 1, 2]),
    # several batches in cyclic order, W + b no multiple of the tail's 64 elements per workgroup
    (dict(B=1024, n=5, z=6, Vw=5000, Ve=300, dw=64, de=100), 5, [2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3]),
    # more tail workgroups (1093) than one pass of the collector's 1024 virtual threads
    (dict(B=512, n=4, z=5, Vw=3000, Ve=200, dw=256, de=272), 4, [0, 1, 2, 3, 0, 1, 2]),
]


@pytest.mark.parametrize('dims,nb,order', FOLD_DIMS, ids=['c2_8192', 'cyclic', 'wide'])
def test_hinted_steps_carry_the_tail_in_the_next_gather(hip_lib, dims, nb, order):
    """Hinted and un-hinted runs of the same batches: equal per-step losses, parameters and both moment tensors; every
    hinted step but the last has its tail inside a gather launch, every un-hinted step launches it alone."""
    d = dims
    p = U.make_vs_problem(91, d['B'] * nb, d['n'], d['z'], d['Vw'], d['Ve'], d['dw'], d['de'], zipf=True)
    plain = run(p, d, order, [None] * len(order))
    hinted = run(p, d, order, right_hints(order))
    assert plain[2] == {'alone': len(order), 'in_gather': 0}, plain[2]
    assert hinted[2] == {'alone': 1, 'in_gather': len(order) - 1}, hinted[2]
    assert_same(plain, hinted)


@pytest.mark.parametrize('case', ['dw_not_x4', 'keep_grads', 'timing'])
def test_steps_the_fold_does_not_apply_to(hip_lib, case):
    """A word dimension that is no multiple of four (the scalar gather), keep_grads (no run-ahead: the caller may read the
    step's activations), a model with timing enabled (every group alone on one queue): hinted steps launch the tail alone
    and still equal the un-hinted ones."""
    d = dict(B=512, n=4, z=5, Vw=2000, Ve=150, dw=30 if case == 'dw_not_x4' else 32, de=48)
    nb, order = 4, [1, 2, 3, 0, 1, 2]
    kw = dict(keep_grads=1 if case == 'keep_grads' else 0, timing=1 if case == 'timing' else 0)
    p = U.make_vs_problem(92, d['B'] * nb, d['n'], d['z'], d['Vw'], d['Ve'], d['dw'], d['de'])
    plain = run(p, d, order, [None] * len(order), **kw)
    hinted = run(p, d, order, right_hints(order), **kw)
    assert plain[2] == {'alone': len(order), 'in_gather': 0}, plain[2]
    assert hinted[2] == {'alone': len(order), 'in_gather': 0}, hinted[2]
    assert_same(plain, hinted)


def test_a_discarded_run_ahead_still_publishes_both_losses(hip_lib):
    """The hint names one batch, the next call trains another: the first step's tail went out with the gather of the
    run-ahead that is then discarded, the second step starts over -- both losses are published and equal the un-hinted
    run's, as does everything after.  A hint past the data set announces nothing: that step's tail is launched alone."""
    d = dict(B=1024, n=5, z=6, Vw=5000, Ve=300, dw=64, de=96)
    nb, order = 5, [0, 2, 4, 1, 3, 0]
    wrong = [1, 3, nb, 2, 4, None]      # never the batch that follows; nb: out of range
    p = U.make_vs_problem(93, d['B'] * nb, d['n'], d['z'], d['Vw'], d['Ve'], d['dw'], d['de'], zipf=True)
    plain = run(p, d, order, [None] * len(order))
    hinted = run(p, d, order, wrong)
    assert hinted[2] == {'alone': 2, 'in_gather': 4}, hinted[2]
    assert_same(plain, hinted)
