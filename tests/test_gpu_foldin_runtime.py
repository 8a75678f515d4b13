"""GPU: the contract of the runtime the three fold-in handles share (csrc/host/foldin_common.inc: the loss ring of
*_train_batches, the upload that replaces or empties the one before, the sampler's counters), on the `base` case of
tests/foldin_cases.py, tests/ll_foldin_cases.py and tests/wfold_cases.py: B = 32, three batches.  Everything here is bit for
bit between two handles of one library: there is no tolerance."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import foldin_cases as FC
from tests import ll_foldin_cases as LC
from tests import util as U
from tests import wfold_cases as WC
from tests import test_gpu_foldin as TF
from tests import test_gpu_ll_foldin as TL
from tests import test_gpu_wfold as TW

pytestmark = pytest.mark.gpu

# name -> (the case, its model, its handle without an upload, every trainable tensor and accumulator, NCE?)
KINDS = {
    'foldin': (lambda: FC.make_case('base'), TF._engine, lambda c, e: TF._foldin(c, e, upload=False), TF._state, True),
    'll_foldin': (lambda: LC.make_case('base'), TL._engine, lambda c, e: TL._foldin(c, e, upload=False), TL._state, False),
    'wfold': (lambda: WC.make_case('base'), TW._engine, lambda c, e: TW._wfold(c, e, upload=False), TW._state, True),
}


class Kind(object):
    def __init__(self, name):
        make, self._engine, self._handle, self.state, self.nce = KINDS[name]
        self.name, self.c = name, make()

    def handles(self, count, upload=True):
        """`count` handles on one snapshot of the case's model, with the case's upload"""
        eng = self._engine(self.c)
        out = [self._handle(self.c, eng) for _ in range(count)]
        eng.close()
        if upload:
            for f in out:
                f.upload(self.c['X'], self.c['y'], self.c['w'])
        return out


@pytest.fixture(scope='module', params=sorted(KINDS))
def kind(request):
    return Kind(request.param)


@pytest.fixture(scope='module', params=sorted(k for k in KINDS if KINDS[k][4]))
def nce_kind(request):
    return Kind(request.param)


def _same(kind, f, g):
    return all(U.same_bits(a, b) for a, b in zip(kind.state(f), kind.state(g)))


def test_ring_regrowth(hip_lib, kind):
    """train_batches over two batches, then over five: the second call outgrows the ring (synchronise, free, regrow).  The
    same seven batches through train_batch on a second handle: the same losses and the same state, bit for bit."""
    f, g = kind.handles(2)
    assert f.num_batches() == 3
    first, second = [0, 1], [2, 0, 1, 1, 0]
    got = np.concatenate([f.train_batches(first), f.train_batches(second)])
    ref = np.array([g.train_batch(b) for b in first + second], dtype=np.float32)
    assert got.shape == (7,) and U.same_bits(got, ref), (got, ref)
    assert _same(kind, f, g)
    f.close()
    g.close()


def test_second_upload_replaces_the_first(hip_lib, kind):
    """Upload A, then upload B with no step in between: three steps give the bits of a handle that only ever saw B."""
    c = kind.c
    f, g = kind.handles(2, upload=False)
    m = 2 * c['B'] + 3                    # B: the first 2 B + 3 instances of A in reverse order -- two batches, another M
    Xb, yb, wb = (np.ascontiguousarray(c[k][:m][::-1]) for k in ('X', 'y', 'w'))
    f.upload(c['X'], c['y'], c['w'])
    f.upload(Xb, yb, wb)
    g.upload(Xb, yb, wb)
    assert f.num_batches() == g.num_batches() == 2
    for b in (0, 1, 0):
        assert U.same_bits(np.float32(f.train_batch(b)), np.float32(g.train_batch(b)))
    assert _same(kind, f, g)
    f.close()
    g.close()


def test_empty_upload(hip_lib, kind):
    """An upload of M = 0 after a real one leaves no batch and no instance; a later real upload trains as a fresh handle."""
    c = kind.c
    f, g = kind.handles(2)
    f.upload(np.zeros((0, c['n']), dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert f.num_batches() == 0
    with pytest.raises(C.SertError, match='no fold-in instances uploaded'):
        f.train_batch(0)
    f.upload(c['X'], c['y'], c['w'])
    assert f.num_batches() == 3
    for b in (0, 1, 2):
        assert U.same_bits(np.float32(f.train_batch(b)), np.float32(g.train_batch(b)))
    assert _same(kind, f, g)
    f.close()
    g.close()


def test_sampler_state(hip_lib, nce_kind):
    """After k device-drawn steps and j device-drawn evaluations the counters read k and j, and negatives_of_step(k) is what
    a second handle at set_step(k) draws: its device-drawn step and this handle's step on those negatives, passed
    explicitly, leave the same bits."""
    kind, k, j = nce_kind, 2, 1
    f, g = kind.handles(2)
    for b in range(k):
        f.train_batch(b)
    for b in range(j):
        f.eval_batch(b)
    assert (f.get_step(), f.get_eval_draws()) == (k, j)
    for which, value in enumerate(kind.state(f)):       # (ROWS, M, V = 0, 1, 2 in both headers)
        g.set_rows(which, value)
    g.set_step(k)
    assert g.get_step() == k and g.get_eval_draws() == 0
    neg = f.negatives_of_step(k)
    assert neg.dtype == np.int64 and np.array_equal(neg, g.negatives_of_step(k))
    assert not np.array_equal(neg, f.negatives_of_step(k, True))       # (the evaluation draws are another stream)
    assert U.same_bits(np.float32(f.train_batch(2, neg)), np.float32(g.train_batch(2)))
    assert _same(kind, f, g)
    assert f.get_step() == g.get_step() == k + 1
    f.close()
    g.close()
