"""GPU: folding unseen WORDS into a trained loglinear model on label ROWS (sert_ll_wfold_upload_csr, include/sert_hip_ll_wfold.h;
llw_row_csr, csrc/kernels_ll_wfold.h) against its oracle twin (tests/ll_wfold_rows_cases.py: ll_wfold_cases' twin with the dense
slice of the rows as a batch's labels).  Loss 1e-5 relative; Nv and both accumulators through tests.util.check_tensor with the
bounds tests/util.py assigns to the loglinear model's word table and its second moments, against the float32 twin and the
float64 one."""
import numpy as np
import pytest
import scipy.sparse

from sert_amd import _capi as C
from tests import ll_wfold_cases as LW
from tests import ll_wfold_rows_cases as LR
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own
_STATE = (('R_w', C.LL_WFOLD_ROWS), ('accu.R_w', C.LL_WFOLD_ACCU), ('delta.R_w', C.LL_WFOLD_DELTA))


def _engine(c):
    return U.ll_engine(dict(Rw=c['Rw'], W=c['W'], b=c['b'], X=c['X']), _MODEL_B, c['n'], 0.01, keep_grads=0)


def _upload(f, c, **over):
    v = dict((k, over.get(k, c[k])) for k in ('X', 'indptr', 'indices', 'data', 'w'))
    f.upload_csr(v['X'], v['indptr'], v['indices'], v['data'], v['w'])


def _foldin(c, eng, upload=True, **kw):
    f = C.LlWordFoldIn(eng, c['Nv0'], c['B'], c['lam'], **kw)
    if upload:
        _upload(f, c)
    return f


def _state(f):
    return [f.get_rows(which) for _, which in _STATE]


def _set_state(f, state):
    for (_, which), val in zip(_STATE, state):
        f.set_rows(which, val)


def _check_against_twins(f, t32, t64, label):
    s32, s64 = t32.state(), t64.state()
    log = []
    for name, which in _STATE:
        square = name.rpartition('.')[0] in U.SECOND_MOMENTS
        log.append(U.check_tensor('%s %s' % (label, name), f.get_rows(which), s32[name], s64[name],
                                  row_tol32=U.state_row_tol32(name), row_tol64=(2 if square else 1) * U.ROW_TOL64))
    print('\n'.join(log))


def _twins(c):
    return LR.LlWordFoldInRowsTwin(c), LR.LlWordFoldInRowsTwin(c, np.float64)


@pytest.fixture(scope='module', params=sorted(LR.CASES))
def case(request):
    return LR.make_case(request.param)


def test_parity_and_plan(hip_lib, case):
    """Every case for three steps (step s trains batch s): the loss of each step and what the step launched -- the label kind,
    the row kernel's form, the levels and items of the reduction against the case's constants --, then Nv and both
    accumulators."""
    c = case
    eng = _engine(c)
    try:
        f = _foldin(c, eng)
        assert f.num_batches() == c['batches']
        assert f.plan()['form'] == 'none'
        t32, t64 = _twins(c)
        for s in range(LR.STEPS):
            got = f.train_batch(s)
            ref = t32.train_step(s)
            t64.train_step(s)
            print('%s step %d: loss %.7f oracle %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
            plan = f.plan()
            print('%s step %d: %r' % (c['name'], s, plan))
            for key, want in LR.expected_plan(c, s).items():
                assert plan[key] == want, (c['name'], s, key, plan[key], want)
            assert plan['gemm_z'] != 'none' and plan['gemm_g'] != 'none' and plan['splits'] >= 1
        _check_against_twins(f, t32, t64, c['name'])
        f.close()
    finally:
        eng.close()


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch on rows = the twin's eval_loss evaluated on the device's tensors (unweighted, unregularised), after one
    training step; no state bit changes."""
    c = case
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        f.train_batch(0)
        before = _state(f)
        tw = LR.LlWordFoldInRowsTwin(c, Nv0=before[0])
        for batch in (1, 2):
            got, ref = f.eval_batch(batch), tw.eval_loss(batch)
            print('%s eval batch %d: %.7f oracle %.7f' % (c['name'], batch, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], batch, got, ref)
            plan = f.plan()
            assert (plan['labels'], plan['train'], plan['levels'], plan['gemm_g']) == ('rows', False, 0, 'none'), plan
        for a, b in zip(before, _state(f)):
            assert U.same_bits(a, b)
    finally:
        f.close()
        eng.close()


def test_one_hot_rows_against_the_integer_upload(hip_lib):
    """one_hot: rows of one entry of value 1 at y and an integer upload of the same instances.  The three losses and Nv of the
    rows handle against the integer handle's as the float32 reference (and the float64 twin), through check_tensor: bit equality
    is not demanded, the compiler may contract the label's add differently in the two kernels."""
    c = LR.make_case('one_hot')
    eng = _engine(c)
    try:
        rows = _foldin(c, eng)
        ints = C.LlWordFoldIn(eng, c['Nv0'], c['B'], c['lam'])
        ints.upload(c['X'], c['y'], c['w'])
        t64 = LR.LlWordFoldInRowsTwin(c, np.float64)
        lr, li, l64 = [], [], []
        for s in range(LR.STEPS):
            lr.append(rows.train_batch(s))
            li.append(ints.train_batch(s))
            l64.append(t64.train_step(s))
            assert rows.plan()['labels'] == 'rows' and ints.plan()['labels'] == 'int'
            assert abs(lr[-1] - li[-1]) <= 1e-5 * abs(li[-1]), (s, lr[-1], li[-1])
        print(U.check_tensor('one_hot losses', np.asarray(lr, np.float32).reshape(1, -1), np.asarray(li, np.float32).reshape(1, -1),
                             np.asarray(l64, np.float64).reshape(1, -1)))
        print(U.check_tensor('one_hot R_w', rows.get_rows(C.LL_WFOLD_ROWS), ints.get_rows(C.LL_WFOLD_ROWS), t64.Nv,
                             row_tol32=U.state_row_tol32('R_w'), row_tol64=U.ROW_TOL64))
        rows.close()
        ints.close()
    finally:
        eng.close()


def test_no_labels_loss_is_zero_and_nothing_moves(hip_lib):
    """no_labels (lambda = 0): no row of batch 0 has an entry -- the loss is exactly 0.0 and Nv and both accumulators keep
    their bits; batch 1 then trains."""
    c = LR.make_case('no_labels')
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        before = _state(f)
        loss = f.train_batch(0)
        assert loss == 0.0, loss
        assert f.eval_batch(0) == 0.0
        for a, b in zip(before, _state(f)):
            assert U.same_bits(a, b)
        assert f.train_batch(1) > 0.0 and not U.same_bits(before[0], _state(f)[0])
    finally:
        f.close()
        eng.close()


@pytest.mark.parametrize('name', ['mixed', 'wide', 've1025'])
def test_reproducible_and_train_batches(hip_lib, name):
    """Two handles hold the same bits after five steps over [0, 2, 1, 1, 0]; train_batches (one synchronisation) gives the
    bits of the train_batch loop."""
    c = LR.make_case(name)
    eng = _engine(c)
    order = [0, 2, 1, 1, 0]
    try:
        a, b = _foldin(c, eng), _foldin(c, eng)
        la = np.asarray([a.train_batch(i) for i in order], np.float32)
        lb = b.train_batches(order)
        assert U.same_bits(la, lb)
        for x, y in zip(_state(a), _state(b)):
            assert U.same_bits(x, y)
        assert not U.same_bits(_state(a)[0], c['Nv0'])
        a.close()
        b.close()
    finally:
        eng.close()


def test_switching_label_kinds_keeps_the_optimiser_state(hip_lib):
    """Rows, then integers, then rows on ONE handle, a step after each upload: every upload keeps Nv and both accumulators, the
    plan's 'labels' follows the upload, and after each step the handle holds the bits of a handle that only ever saw that
    upload, with the state before the step set through set_rows."""
    c = LR.make_case('one_hot')                    # (it carries y as well: both kinds on the same instances)
    m = LR.make_case('mixed')                      # the same shapes, other rows
    assert all(c[k] == m[k] for k in ('Vw', 'Nw', 'Ve', 'd', 'n', 'B'))
    eng = _engine(c)
    try:
        f = C.LlWordFoldIn(eng, c['Nv0'], c['B'], c['lam'])
        uploads = (('rows', lambda h: h.upload_csr(m['X'], m['indptr'], m['indices'], m['data'], m['w'])),
                   ('int', lambda h: h.upload(c['X'], c['y'], c['w'])),
                   ('rows', lambda h: h.upload_csr(c['X'], c['indptr'], c['indices'], c['data'], c['w'])))
        for step, (kind, upload) in enumerate(uploads):
            before = _state(f)
            upload(f)
            for x, y in zip(before, _state(f)):
                assert U.same_bits(x, y)
            only = C.LlWordFoldIn(eng, c['Nv0'], c['B'], c['lam'])
            upload(only)
            _set_state(only, before)
            got, same = f.train_batch(step), only.train_batch(step)
            assert f.plan()['labels'] == kind and only.plan()['labels'] == kind
            assert U.same_bits(np.float32(got), np.float32(same)), (step, kind, got, same)
            for x, y in zip(_state(f), _state(only)):
                assert U.same_bits(x, y)
            assert not U.same_bits(before[0], _state(f)[0])
            only.close()
        f.close()
    finally:
        eng.close()


def test_refusals_keep_the_earlier_upload(hip_lib):
    """Every fault of the rows is found on the host and comes back nonzero with its message; after each the earlier upload is
    kept, and the handle ends where a handle ends that never saw a refusal."""
    c = LR.make_case('mixed')
    Vw, Nw, Ve, B = c['Vw'], c['Nw'], c['Ve'], c['B']
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
        assert c['indptr'][4] >= 1
        bad = [
            ('csr_indptr\\[0\\] != 0', changed('indptr', 0, 1)),
            ('csr_indptr is not non-decreasing', changed('indptr', 5, c['indptr'][4] - 1)),
            ('label column out of range \\[0, num_entities\\)', changed('indices', a, -1)),
            ('label column out of range \\[0, num_entities\\)', changed('indices', a + 2, Ve)),      # (no new entity here)
            ('csr_indices of row %d are not strictly increasing \\(duplicate or unsorted label column %d\\)'
             % (row, c['indices'][a]), changed('indices', a + 1, c['indices'][a])),
            ('csr_indices of row %d are not strictly increasing \\(duplicate or unsorted label column %d\\)'
             % (row, swapped[a + 1]), dict(indices=swapped)),
            ('token id out of range', changed('X', (3, 1), -1)),
            ('token id out of range', changed('X', (3, 1), Vw + Nw)),
        ]
        for message, over in bad:
            with pytest.raises(C.SertError, match=message):
                _upload(f, c, **over)
            assert f.num_batches() == c['batches']
        # null arrays with M > 0 (the library's own check, behind the binding's)
        lib, M = C.load(), c['M']
        x, indptr, indices, data = (np.ascontiguousarray(c[k]) for k in ('X', 'indptr', 'indices', 'data'))
        for args in ((None, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data),
                     (x.ctypes.data, None, indices.ctypes.data, data.ctypes.data),
                     (x.ctypes.data, indptr.ctypes.data, None, data.ctypes.data),
                     (x.ctypes.data, indptr.ctypes.data, indices.ctypes.data, None)):
            with pytest.raises(C.SertError, match='bad argument'):
                C.check(lib.sert_ll_wfold_upload_csr(f._h, args[0], args[1], args[2], args[3], None, M))
            assert f.num_batches() == c['batches']
        with pytest.raises(C.SertError, match='more than 2\\^31 - 1 fold-in instances'):
            C.check(lib.sert_ll_wfold_upload_csr(f._h, x.ctypes.data, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, None,
                                                 2 ** 31))
        with pytest.raises(C.SertError, match='indptr'):
            f.upload_csr(c['X'], c['indptr'][:-1], c['indices'], c['data'], c['w'])          # (the binding: indptr is M + 1)
        # the frozen table: one byte below need is refused with the bytes needed and the earlier upload is kept
        distinct = np.unique(c['X'][c['X'] < Vw]).size
        need = distinct * Ve * 4
        capped = _foldin(c, eng, upload=False, max_cache_bytes=need - 1)
        with pytest.raises(C.SertError, match='needs %d bytes' % need):
            _upload(capped, c)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            capped.train_batch(0)
        first = c['X'][:B]
        assert np.unique(first[first < Vw]).size < distinct
        end = int(c['indptr'][B])
        capped.upload_csr(c['X'][:B], c['indptr'][:B + 1], c['indices'][:end], c['data'][:end], c['w'][:B])
        with pytest.raises(C.SertError, match='needs %d bytes' % need):
            _upload(capped, c)
        assert capped.num_batches() == 1 and capped.plan()['form'] == 'none'        # (the earlier upload is kept)
        exact = _foldin(c, eng, upload=False, max_cache_bytes=need)
        _upload(exact, c)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batch(c['batches'])
        # nothing above moved the handles: each trains as one that never saw a refusal
        for s in range(LR.STEPS):
            want = np.float32(clean.train_batch(s))
            assert U.same_bits(np.float32(f.train_batch(s)), want) and U.same_bits(np.float32(exact.train_batch(s)), want)
        for h in (f, exact):
            for x_, y_ in zip(_state(h), _state(clean)):
                assert U.same_bits(x_, y_)
        ref = LR.LlWordFoldInRowsTwin(c).train_step(0)
        got = capped.train_batch(0)
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        # a handle without an upload: refused uploads leave it without one
        g = _foldin(c, eng, upload=False)
        with pytest.raises(C.SertError, match='not strictly increasing'):
            _upload(g, c, indices=swapped)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            g.train_batch(0)
        for h in (f, clean, capped, exact, g):
            h.close()
    finally:
        eng.close()


@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_non_finite_row_reaches_the_loss(hip_lib, value):
    """A NaN, and separately a +inf, in a new row that the batch reads makes the train loss and the eval loss non-finite on a
    rows upload."""
    c = LR.make_case('mixed')
    # a row without an entry has loss 0 whatever J is: the word is one that an instance WITH labels of batch 0 reads
    B = c['B']
    labelled = np.diff(c['indptr'])[:B] > 0
    at = np.argwhere((c['X'][:B] >= c['Vw']) & labelled[:, None])
    assert len(at)
    word = int(c['X'][at[0][0], at[0][1]] - c['Vw'])
    rows = c['Nv0'].copy()
    rows[word, 1] = value
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        f.set_rows(C.LL_WFOLD_ROWS, rows)
        assert not np.isfinite(f.eval_batch(0))
        assert not np.isfinite(f.train_batch(0))
    finally:
        f.close()
        eng.close()


def test_python_loglinear_word_foldin_model_with_sparse_labels(hip_lib):
    """sert_amd.foldin.LogLinearWordFoldIn with a scipy.sparse y: two shuffled epochs track the twin on the traced batches; an
    unsorted COO input with a duplicate entry is canonicalised -- duplicates summed, as scipy does -- and holds the bits of the
    canonical input."""
    from sert_amd import foldin
    c = LR.make_case('mixed')

    def make(y):
        return foldin.LogLinearWordFoldIn(c['Rw'], c['W'], c['b'], c['Nv0'], (c['X'], y, c['w']), batch_size=c['B'],
                                          regularization_lambda=c['lam'], window_size=c['n'])

    np.random.seed(7)           # (the order of the batches inside an epoch)
    fold = make(c['Y'])
    trace, step = [], fold.train_fn
    fold.train_fn = lambda i: (trace.append(i), step(i))[1]
    first, _ = fold.train_error()
    for _ in range(2):
        num_batches, loss = fold.train()
        assert num_batches == c['batches'] and np.isfinite(loss)
    assert len(trace) == 2 * c['batches'] and np.isfinite(first) and fold._foldin.plan()['labels'] == 'rows'
    t32, t64 = _twins(c)
    for batch_index in trace:
        t32.train_step(batch_index)
        t64.train_step(batch_index)
    Nv = fold.get_new_word_representations()
    print(U.check_tensor('new word rows after %d steps' % len(trace), Nv, t32.Nv, t64.Nv))
    # the same matrix as COO, entries in reverse order, one entry split into two halves (exact in float32)
    coo = c['Y'].tocoo()
    rows_, cols, vals = coo.row[::-1].copy(), coo.col[::-1].copy(), coo.data[::-1].copy()
    vals[0] = vals[0] / 2
    messy = scipy.sparse.coo_matrix((np.append(vals, vals[0]), (np.append(rows_, rows_[0]), np.append(cols, cols[0]))),
                                    shape=c['Y'].shape)
    assert messy.nnz == c['Y'].nnz + 1
    other, clean = make(messy), make(c['Y'])
    assert messy.nnz == c['Y'].nnz + 1                      # (the caller's matrix is not modified)
    for s in range(LR.STEPS):
        assert U.same_bits(np.float32(other._foldin.train_batch(s)), np.float32(clean._foldin.train_batch(s)))
    for a, b in zip(_state(other._foldin), _state(clean._foldin)):
        assert U.same_bits(a, b)
    with pytest.raises(RuntimeError, match='label rows must have V_e = %d columns' % c['Ve']):
        make(scipy.sparse.csr_matrix((c['M'], c['Ve'] + 1), dtype=np.float32))
    for h in (fold, other, clean):
        h.close()


def test_python_loglinear_word_foldin_from_a_live_model_with_sparse_labels(hip_lib):
    """sert_amd.foldin.LogLinearWordFoldIn.from_model with rows: three steps track the twin and hold the bits of a fold-in built
    from the same parameters as host arrays."""
    from sert_amd import foldin, models
    c = LR.make_case('mixed')
    B, Vw = c['B'], c['Vw']
    y_int = np.zeros(c['M'], np.int32)
    trained = (np.minimum(c['X'], Vw - 1), y_int, c['w'])           # the model's own instances: trained words only
    model = models.LanguageModel(batch_size=B, window_size=c['n'], representations_init=c['Rw'], output_layer_size=c['Ve'],
                                 regularization_lambda=0.01, training_set=trained,
                                 validation_set=(trained[0][:B], trained[1][:B]))
    model.set_dense(c['W'], c['b'])
    live = foldin.LogLinearWordFoldIn.from_model(model, c['Nv0'], (c['X'], c['Y'], c['w']), B, c['lam'])
    host = foldin.LogLinearWordFoldIn(c['Rw'], c['W'], c['b'], c['Nv0'], (c['X'], c['Y'], c['w']), batch_size=B,
                                      regularization_lambda=c['lam'], window_size=c['n'])
    t32, t64 = _twins(c)
    for s in range(LR.STEPS):
        got, same = live._foldin.train_batch(s), host._foldin.train_batch(s)
        ref = t32.train_step(s)
        t64.train_step(s)
        assert U.same_bits(np.float32(got), np.float32(same)) and abs(got - ref) <= 1e-5 * abs(ref), (s, got, same, ref)
        assert live._foldin.plan()['labels'] == 'rows'
    _check_against_twins(live._foldin, t32, t64, 'from_model with rows after %d steps' % LR.STEPS)
    for a, b in zip(_state(live._foldin), _state(host._foldin)):
        assert U.same_bits(a, b)
    live.close()
    host.close()
