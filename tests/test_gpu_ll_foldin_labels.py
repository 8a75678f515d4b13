"""GPU: the loglinear fold-in on label ROWS that may name trained entities (sert_ll_foldin_upload_csr, llf_row_csr in
csrc/kernels_ll_foldin.h) against its oracle twin (tests/ll_foldin_label_cases.py: LogLinearOracle on the dense rows).  The
bounds are those of tests/test_gpu_ll_foldin.py: loss 1e-5 relative; Wn, bn and the four accumulators through
tests.util.check_tensor, against the float32 twin and the float64 one."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import ll_foldin_cases as LC
from tests import ll_foldin_label_cases as LL
from tests import util as U
from tests.test_gpu_ll_foldin import _STATE, _check_against_twins, _engine, _state

pytestmark = pytest.mark.gpu


def _upload(f, c, **over):
    a = dict((k, c[k]) for k in ('X', 'indptr', 'indices', 'data', 'w'))
    a.update(over)
    f.upload_csr(a['X'], a['indptr'], a['indices'], a['data'], a['w'])


def _foldin(c, eng, upload=True):
    f = C.LlFoldIn(eng, c['Wn0'], c['bn0'], c['B'], c['lam'])
    if upload:
        _upload(f, c)
    return f


@pytest.fixture(scope='module', params=sorted(LL.CASES))
def case(request):
    return LL.make_case(request.param)


def test_parity(hip_lib, case):
    """Every case for three steps (step s trains batch s): the loss of each step, then Wn, bn and the four accumulators; the
    engine's frozen tensors keep their bits."""
    c = case
    eng = _engine(c)
    try:
        frozen = [eng.get_tensor(t).copy() for t in (C.T_RW, C.T_W, C.T_B)]
        f = _foldin(c, eng)
        assert f.num_batches() == c['batches']
        t32, t64 = LL.LlLabelTwin(c), LL.LlLabelTwin(c, np.float64)
        for s in range(LL.STEPS):
            got = f.train_batch(s)
            ref = t32.train_step(s)
            t64.train_step(s)
            print('%s step %d: loss %.7f oracle %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
            if c['name'] == 'no_labels' and s == 0:
                assert got == 0.0
                assert U.same_bits(f.get_tensor(C.LL_FOLDIN_W), c['Wn0']) and U.same_bits(f.get_tensor(C.LL_FOLDIN_B), c['bn0'])
        _check_against_twins(f, t32, t64, c['name'])
        for a, t in zip(frozen, (C.T_RW, C.T_W, C.T_B)):
            assert U.same_bits(a, eng.get_tensor(t))
        f.close()
    finally:
        eng.close()


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch = the twin's eval_loss on the device's tensors (unweighted, unregularised), after one training step; no
    state bit changes."""
    c = case
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        tw = LL.LlLabelTwin(c)
        f.train_batch(0)
        before = _state(f)
        tw.Wn[...] = before[0]
        tw.bn[...] = before[1]
        for batch in (1, 2):
            got, ref = f.eval_batch(batch), tw.eval_loss(batch)
            print('%s eval batch %d: %.7f oracle %.7f' % (c['name'], batch, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], batch, got, ref)
        for a, b in zip(before, _state(f)):
            assert U.same_bits(a, b)
    finally:
        f.close()
        eng.close()


@pytest.mark.parametrize('name', ['mixed', 'wide'])
def test_reproducible_and_train_batches(hip_lib, name):
    """Two handles hold the same bits after five steps over [0, 2, 1, 1, 0]; train_batches (one synchronisation) gives the
    bits of the train_batch loop."""
    c = LL.make_case(name)
    eng = _engine(c)
    order = [0, 2, 1, 1, 0]
    try:
        a, b = _foldin(c, eng), _foldin(c, eng)
        la = np.asarray([a.train_batch(i) for i in order], np.float32)
        lb = b.train_batches(order)
        assert U.same_bits(la, lb)
        for x, y in zip(_state(a), _state(b)):
            assert U.same_bits(x, y)
        assert not U.same_bits(_state(a)[0], c['Wn0'])
        a.close()
        b.close()
    finally:
        eng.close()


def test_one_hot_rows_against_the_integer_upload(hip_lib):
    """one_hot -- one entry of value 1 at V_e + y -- meets the integer upload's oracle bounds on the same data (test_parity runs
    it); here the two forms on two handles: both within 1e-5 of the same oracle loss.  Whether they leave the same bits is
    printed, not asserted.  Then either form replaces the other on ONE handle, the optimiser state kept: the handle goes on
    as a twin does that is fed the same batches."""
    c, b = LL.make_case('one_hot'), LC.make_case('base')
    eng = _engine(c)
    try:
        rows, ints = _foldin(c, eng), C.LlFoldIn(eng, b['Wn0'], b['bn0'], b['B'], b['lam'])
        ints.upload(b['X'], b['y'], b['w'])
        t32, t64 = LL.LlLabelTwin(c), LL.LlLabelTwin(c, np.float64)      # (one_hot's rows ARE base's labels: one twin for both)
        for s in range(LL.STEPS):
            lr, li, ref = rows.train_batch(s), ints.train_batch(s), t32.train_step(s)
            t64.train_step(s)
            print('one_hot step %d: loss of the rows %.7f, of the integers %.7f, oracle %.7f' % (s, lr, li, ref))
            assert abs(lr - ref) <= 1e-5 * abs(ref) and abs(li - ref) <= 1e-5 * abs(ref)
        same = all(U.same_bits(x, y) for x, y in zip(_state(rows), _state(ints)))
        print('one_hot: label rows and integer labels leave %s bits after %d steps' % ('THE SAME' if same else 'DIFFERENT', LL.STEPS))
        ints.close()
        # rows -> integers -> rows on the handle `rows`, the optimiser state kept: integer labels of base, then the rows of
        # mixed (its instances, rows and weights; the frozen tensors are the engine's, one_hot's)
        rows.upload(b['X'], b['y'], b['w'])
        got, ref = rows.train_batch(1), t32.train_step(1)
        t64.train_step(1)
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        m = LL.make_case('mixed')
        assert all(m[k] == c[k] for k in ('Vw', 'Ve', 'N', 'd', 'n', 'B', 'lam'))
        _upload(rows, m)
        for t in (t32, t64):
            t.c = dict(m, Rw=c['Rw'], W=c['W'], b=c['b'])
        got, ref = rows.train_batch(2), t32.train_step(2)
        t64.train_step(2)
        print('rows -> integers -> rows: loss %.7f oracle %.7f' % (got, ref))
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        _check_against_twins(rows, t32, t64, 'rows -> integers -> rows')
        rows.close()
    finally:
        eng.close()


def test_refusals_keep_the_earlier_upload(hip_lib):
    """Every fault of the rows is found on the host and comes back with its message; after each the earlier upload still
    trains: the handle ends where a handle ends that never saw a refusal."""
    c = LL.make_case('mixed')
    V = c['Ve'] + c['N']
    eng = _engine(c)
    try:
        f, clean = _foldin(c, eng), _foldin(c, eng)
        row = 3                                       # three entries
        a = int(c['indptr'][row])
        assert c['indptr'][row + 1] - a == 3

        def changed(key, at, value):
            v = c[key].copy()
            v[at] = value
            return {key: v}

        swapped = c['indices'].copy()
        swapped[a], swapped[a + 1] = swapped[a + 1], swapped[a]
        bad = [
            ('csr_indptr\\[0\\] != 0', changed('indptr', 0, 1)),
            ('csr_indptr is not non-decreasing', changed('indptr', 5, c['indptr'][4] - 1)),
            ('label column out of range', changed('indices', a, -1)),
            ('label column out of range', changed('indices', a + 2, V)),
            ('csr_indices of row %d are not strictly increasing' % row, dict(indices=swapped)),
            ('csr_indices of row %d are not strictly increasing' % row, changed('indices', a + 1, c['indices'][a])),
            ('token id out of range', changed('X', (3, 1), -1)),
            ('token id out of range', changed('X', (3, 1), c['Vw'])),
        ]
        assert c['indptr'][4] >= 1
        for message, over in bad:
            with pytest.raises(C.SertError, match=message):
                _upload(f, c, **over)
            assert f.num_batches() == c['batches']
        with pytest.raises(C.SertError, match='indptr'):
            f.upload_csr(c['X'], c['indptr'][:-1], c['indices'], c['data'], c['w'])          # (the binding: indptr is M + 1)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batch(c['batches'])
        for s in range(LL.STEPS):
            assert U.same_bits(np.float32(f.train_batch(s)), np.float32(clean.train_batch(s)))
        for x, y in zip(_state(f), _state(clean)):
            assert U.same_bits(x, y)
        # a handle without an upload: refused uploads leave it without one
        g = _foldin(c, eng, upload=False)
        with pytest.raises(C.SertError, match='not strictly increasing'):
            _upload(g, c, indices=swapped)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            g.train_batch(0)
        for h in (f, clean, g):
            h.close()
    finally:
        eng.close()
