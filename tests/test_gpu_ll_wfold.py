"""GPU: folding unseen WORDS into a trained loglinear model (include/sert_hip_ll_wfold.h, csrc/kernels_ll_wfold.h) against its
oracle twin (tests/ll_wfold_cases.py: LogLinearOracle / Adadelta on the extended word table).  Loss 1e-5 relative; Nv and both
accumulators through tests.util.check_tensor with the bounds tests/util.py assigns to the loglinear model's word table and its
second moments, against the float32 twin and the float64 one."""
import ctypes

import numpy as np
import pytest

from sert_amd import _capi as C
from tests import ll_wfold_cases as LW
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own
_STATE = (('R_w', C.LL_WFOLD_ROWS), ('accu.R_w', C.LL_WFOLD_ACCU), ('delta.R_w', C.LL_WFOLD_DELTA))


def _engine(c, n=None):
    return U.ll_engine(dict(Rw=c['Rw'], W=c['W'], b=c['b'], X=c['X']), _MODEL_B, c['n'] if n is None else n, 0.01, keep_grads=0)


def _foldin(c, eng, upload=True, **kw):
    f = C.LlWordFoldIn(eng, c['Nv0'], c['B'], c['lam'], **kw)
    if upload:
        f.upload(c['X'], c['y'], c['w'])
    return f


def _state(f):
    return [f.get_rows(which) for _, which in _STATE]


def _check_against_twins(f, t32, t64, label):
    s32, s64 = t32.state(), t64.state()
    log = []
    for name, which in _STATE:
        square = name.rpartition('.')[0] in U.SECOND_MOMENTS
        log.append(U.check_tensor('%s %s' % (label, name), f.get_rows(which), s32[name], s64[name],
                                  row_tol32=U.state_row_tol32(name), row_tol64=(2 if square else 1) * U.ROW_TOL64))
    print('\n'.join(log))


@pytest.fixture(scope='module', params=sorted(LW.CASES))
def case(request):
    return LW.make_case(request.param)


def test_parity_and_plan(hip_lib, case):
    """Every case for three steps (step s trains batch s): the loss of each step and what the step launched -- the row
    kernel's form, the levels and items of the reduction against the case's constants --, then Nv and both accumulators."""
    c = case
    eng = _engine(c)
    try:
        f = _foldin(c, eng)
        assert f.num_batches() == c['batches']
        assert f.plan()['form'] == 'none'
        t32, t64 = LW.LlWordFoldInTwin(c), LW.LlWordFoldInTwin(c, np.float64)
        for s in range(LW.STEPS):
            got = f.train_batch(s)
            ref = t32.train_step(s)
            t64.train_step(s)
            print('%s step %d: loss %.7f oracle %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
            plan = f.plan()
            print('%s step %d: %r' % (c['name'], s, plan))
            for key, want in LW.expected_plan(c, s).items():
                assert plan[key] == want, (c['name'], s, key, plan[key], want)
            assert plan['gemm_z'] != 'none' and plan['gemm_g'] != 'none' and plan['splits'] >= 1
            if c['name'] == 've4100':
                assert plan['splits'] == c['Ve'] // 1024, plan           # (the K >= 4096 rule of gemm_long_k)
        _check_against_twins(f, t32, t64, c['name'])
        f.close()
    finally:
        eng.close()


def test_forms_at_the_threshold(hip_lib):
    """V_e = 1024 is the last shape of the register form and V_e = 1025 the first of the streaming one."""
    for name, form, vec in (('ve1024', 'reg', True), ('ve1025', 'stream', False)):
        c = LW.make_case(name)
        eng = _engine(c)
        f = _foldin(c, eng)
        try:
            f.eval_batch(0)
            plan = f.plan()
            assert (plan['form'], plan['vec'], plan['train'], plan['levels'], plan['gemm_g']) == (form, vec, False, 0, 'none'), plan
        finally:
            f.close()
            eng.close()


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch = the twin's eval_loss evaluated on the device's tensors (unweighted, unregularised), after one training
    step; no state bit changes."""
    c = case
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        f.train_batch(0)
        before = _state(f)
        tw = LW.LlWordFoldInTwin(c, Nv0=before[0])
        for batch in (1, 2):
            got, ref = f.eval_batch(batch), tw.eval_loss(batch)
            print('%s eval batch %d: %.7f oracle %.7f' % (c['name'], batch, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], batch, got, ref)
        for a, b in zip(before, _state(f)):
            assert U.same_bits(a, b)
    finally:
        f.close()
        eng.close()


def test_frozen_and_snapshot(hip_lib):
    """The model's three tensors hold the same bits before and after a fold-in; training the model after the handle was
    created, and closing it, does not change what the handle computes."""
    c = LW.make_case('base')
    results = []
    for disturb in (False, True):
        eng = _engine(c)
        ids = (C.T_RW, C.T_W, C.T_B)
        before = [eng.get_tensor(t).copy() for t in ids]
        f = _foldin(c, eng)
        losses = [f.train_batch(0)]
        if disturb:
            rng = np.random.RandomState(3)
            eng.upload_dataset(C.SPLIT_TRAIN, rng.randint(0, c['Vw'], (2 * _MODEL_B, c['n'])).astype(np.uint32),
                               y_int=rng.randint(0, c['Ve'], 2 * _MODEL_B).astype(np.int32), w=np.ones(2 * _MODEL_B, np.float32))
            eng.train_batch(0)
            assert not np.array_equal(eng.get_tensor(C.T_W), before[1])          # the model DID move
            losses.append(f.train_batch(1))
            eng.close()
            losses.append(f.train_batch(2))
        else:
            losses += [f.train_batch(1), f.train_batch(2)]
            for a, t in zip(before, ids):
                assert U.same_bits(a, eng.get_tensor(t))
            eng.close()
        results.append([np.asarray(losses, np.float32)] + _state(f))
        f.close()
    for a, b in zip(*results):
        assert U.same_bits(a, b)


@pytest.mark.parametrize('name', ['base', 'chunk65', 've1025'])
def test_reproducible_and_train_batches(hip_lib, name):
    """Two handles hold the same bits after five steps over [0, 2, 1, 1, 0]; train_batches (one synchronisation) gives the
    bits of the train_batch loop; the state round-trips through get_rows / set_rows."""
    c = LW.make_case(name)
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
        d = _foldin(c, eng)
        for (_, which), val in zip(_STATE, _state(a)):
            d.set_rows(which, val)
        assert U.same_bits(np.float32(a.train_batch(1)), np.float32(d.train_batch(1)))
        for x, y in zip(_state(a), _state(d)):
            assert U.same_bits(x, y)
        for h in (a, b, d):
            h.close()
    finally:
        eng.close()


def test_second_upload_keeps_the_optimiser_state(hip_lib):
    """An upload replaces the instances and keeps Nv and both accumulators: two steps with a re-upload of the same instances
    in between hold the bits of two steps without it; an upload of other instances trains on them."""
    c = LW.make_case('base')
    eng = _engine(c)
    try:
        a, b = _foldin(c, eng), _foldin(c, eng)
        la = [a.train_batch(0), a.train_batch(1)]
        lb = [b.train_batch(0)]
        kept = _state(b)
        b.upload(c['X'], c['y'], c['w'])
        for x, y in zip(kept, _state(b)):
            assert U.same_bits(x, y)
        lb.append(b.train_batch(1))
        assert U.same_bits(np.asarray(la, np.float32), np.asarray(lb, np.float32))
        for x, y in zip(_state(a), _state(b)):
            assert U.same_bits(x, y)
        # other instances: batch 0 of the new upload is the old batch 2
        B = c['B']
        tw = LW.LlWordFoldInTwin(c, Nv0=_state(b)[0])
        tw.opt.accu[0][...], tw.opt.delta[0][...] = _state(b)[1], _state(b)[2]
        b.upload(c['X'][2 * B:3 * B], c['y'][2 * B:3 * B], c['w'][2 * B:3 * B])
        assert b.num_batches() == 1
        got, ref = b.train_batch(0), tw.train_step(2)
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        a.close()
        b.close()
    finally:
        eng.close()


def test_refusals(hip_lib):
    """Every refusal of the contract comes back nonzero with its message -- validated on the host, nothing is launched on bad
    ids -- and the handle trains normally afterwards."""
    c = LW.make_case('base')
    B, Nw, d, n, Vw, Ve = c['B'], c['Nw'], c['d'], c['n'], c['Vw'], c['Ve']
    # a vectorspace model, the full-softmax kind, a model with a communicator, a window of 33
    kw = dict(batch_size=8, global_batch_size=8, window_size=n, vocab_size=Vw, num_entities=Ve, word_dim=d, entity_dim=8,
              id_bytes=4, device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
    vs = C.Engine(kind=C.KIND_VECTORSPACE, num_negatives=2, **kw)
    with pytest.raises(C.SertError, match='needs a loglinear model'):
        C.LlWordFoldIn(vs, c['Nv0'], B, 0.01)
    vs.close()
    fs = C.Engine(kind=C.KIND_VECTORSPACE_SOFTMAX, num_negatives=0, **kw)
    with pytest.raises(C.SertError, match='SOFTMAX'):
        C.LlWordFoldIn(fs, c['Nv0'], B, 0.01)
    fs.close()
    dp = _engine(c)
    dp.comm_init(C.comm_unique_id(), 0, 1)
    with pytest.raises(C.SertError, match='communicator'):
        C.LlWordFoldIn(dp, c['Nv0'], B, 0.01)
    dp.close()
    wide = _engine(c, n=33)
    with pytest.raises(C.SertError, match='window sizes up to 32'):
        C.LlWordFoldIn(wide, c['Nv0'], B, 0.01)
    wide.close()
    eng = _engine(c)
    try:
        with pytest.raises(C.SertError, match='at least one new word'):
            C.LlWordFoldIn(eng, np.zeros((0, d), np.float32), B, 0.01)
        with pytest.raises(C.SertError, match='batch_size >= 1'):
            C.LlWordFoldIn(eng, c['Nv0'], 0, 0.01)
        with pytest.raises(C.SertError, match='lambda must be >= 0'):
            C.LlWordFoldIn(eng, c['Nv0'], B, -0.5)
        with pytest.raises(C.SertError, match='rho'):
            C.LlWordFoldIn(eng, c['Nv0'], B, 0.01, rho=1.0)
        with pytest.raises(C.SertError, match='eps > 0'):
            C.LlWordFoldIn(eng, c['Nv0'], B, 0.01, eps=0.0)
        cfg = C.SertLlWFoldConfig()
        cfg.struct_size, cfg.batch_size, cfg.rho, cfg.eps = ctypes.sizeof(C.SertLlWFoldConfig) - 4, B, 0.95, 1e-6
        h = ctypes.c_void_p()
        with pytest.raises(C.SertError, match='size mismatch'):
            C.check(C.load().sert_ll_wfold_create(eng._h, Nw, c['Nv0'].ctypes.data, ctypes.byref(cfg), ctypes.byref(h)))
        assert not h
        # the size limits: each product alone above 2^31 - 1 (nothing is allocated before the checks)
        with pytest.raises(C.SertError, match=r'batch_size \* window_size > 2\^31 - 1'):
            C.LlWordFoldIn(eng, c['Nv0'], (1 << 31) // n + 1, 0.01)
        with pytest.raises(C.SertError, match=r'batch_size \* num_entities > 2\^31 - 1'):
            C.LlWordFoldIn(eng, c['Nv0'], (1 << 31) // Ve + 1, 0.01)
        cfg.struct_size = ctypes.sizeof(C.SertLlWFoldConfig)
        for count, text in (((1 << 31) // Ve + 1, 'num_new_words \\* num_entities > 2\\^31 - 1'),
                            ((1 << 31) - 1 - Vw + 1, 'rows in the extended word table')):
            with pytest.raises(C.SertError, match=text):
                C.check(C.load().sert_ll_wfold_create(eng._h, count, c['Nv0'].ctypes.data, ctypes.byref(cfg), ctypes.byref(h)))
            assert not h
        # the frozen table: one byte below need is refused with the bytes needed and the earlier upload is kept
        distinct = np.unique(c['X'][c['X'] < Vw]).size
        need = distinct * Ve * 4
        capped = _foldin(c, eng, upload=False, max_cache_bytes=need - 1)
        with pytest.raises(C.SertError, match='needs %d bytes' % need):
            capped.upload(c['X'], c['y'], c['w'])
        with pytest.raises(C.SertError, match='no fold-in instances'):
            capped.train_batch(0)
        first = c['X'][:B]
        assert np.unique(first[first < Vw]).size < distinct
        capped.upload(c['X'][:B], c['y'][:B], c['w'][:B])
        with pytest.raises(C.SertError, match='needs %d bytes' % need):
            capped.upload(c['X'], c['y'], c['w'])
        assert capped.num_batches() == 1                    # (the earlier upload is kept)
        exact = _foldin(c, eng, upload=False, max_cache_bytes=need)
        exact.upload(c['X'], c['y'], c['w'])
        f = _foldin(c, eng, upload=False)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.train_batch(0)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.eval_batch(0)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.train_batches([0])
        for bad in (-1, Ve):
            y = c['y'].copy()
            y[7] = bad
            with pytest.raises(C.SertError, match=r'label out of range'):
                f.upload(c['X'], y, c['w'])
        for bad in (-1, Vw + Nw):
            X = c['X'].copy()
            X[3, 1] = bad
            with pytest.raises(C.SertError, match='token id out of range'):
                f.upload(X, c['y'], c['w'])
        f.upload(c['X'], c['y'], c['w'])
        with pytest.raises(C.SertError, match='label out of range'):
            f.upload(c['X'], np.full_like(c['y'], Ve), c['w'])              # (a refused upload keeps the earlier one)
        # (M > 2^31 - 1 needs arrays no test can hold: the count is checked before the arrays are read)
        one = np.zeros(4, np.int32)
        with pytest.raises(C.SertError, match='more than 2\\^31 - 1 fold-in instances'):
            C.check(C.load().sert_ll_wfold_upload(f._h, one.ctypes.data, one.ctypes.data, None, 2 ** 31))
        assert f.num_batches() == c['batches']         # (the earlier upload is kept)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batch(c['batches'])               # (the trailing M mod B instances are no batch)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batches([0, c['batches']])
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.eval_batch(-1)
        with pytest.raises(C.SertError, match='element count'):
            f.set_rows(C.LL_WFOLD_ACCU, np.zeros(3, np.float32))
        out = np.zeros(Nw * d, np.float32)
        with pytest.raises(C.SertError, match='which must be'):
            C.check(C.load().sert_ll_wfold_get_rows(f._h, 3, out.ctypes.data, out.size))
        # nothing above moved the handles: each trains as a fresh one does
        ref = LW.LlWordFoldInTwin(c).train_step(0)
        for h in (f, capped, exact):
            assert U.same_bits(h.get_rows(C.LL_WFOLD_ROWS), c['Nv0'])
            got = h.train_batch(0)
            assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
            h.close()
    finally:
        eng.close()


@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_non_finite_row_reaches_the_loss(hip_lib, value):
    """A NaN, and separately a +inf, in a new row that the batch reads makes the train loss and the eval loss non-finite."""
    c = LW.make_case('base')
    word = int(c['X'][0, 0] - c['Vw'])                 # (base: instance 0 of batch 0 holds new word 0)
    assert word >= 0
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


def test_frozen_table_past_4_gib(hip_lib):
    """A frozen table of more than 2^32 bytes: V_e = 100 000, d = 4, 11 000 distinct frozen words, n = 2, B = 2.  The tested
    batch's frozen words are the highest rows of the table (the largest trained ids); the twin runs on that batch alone.
    What this shape can catch is 32-bit BYTE arithmetic: its largest ELEMENT offset, 10 999 * 100 000, is below 2^31, so a 32-bit
    element offset in llw_row's LDS table or in the upload's slab offsets would pass it too -- that those are 64 bits wide rests
    on reading the code (a table of more than 2^31 elements is 8 GiB and more, beyond what a test of a few seconds fills)."""
    Vw, Nw, Ve, d, n, B, lam = 11000, 3, 100000, 4, 2, 2, 0.01
    rng = np.random.RandomState(77)
    Rw = U.O.glorot_uniform(rng, (Vw, d))
    W = U.O.glorot_uniform(rng, (d, Ve))
    b = (0.1 * rng.randn(Ve)).astype(np.float32)
    Nv0 = (0.5 * rng.randn(Nw, d)).astype(np.float32)
    # every trained word once, in id order; each window holds a frozen word and a new one, the last window a word twice
    M = Vw
    X = np.stack([np.arange(Vw), Vw + rng.randint(0, Nw, size=M)], axis=1).astype(np.int32)
    X[M - 1] = (Vw - 1, Vw + 1)
    X[M - 2] = (Vw + 1, Vw - 2)
    y = rng.randint(0, Ve, size=M).astype(np.int32)
    w = rng.uniform(0.5, 2.0, M).astype(np.float32)
    assert Vw * Ve * 4 > (1 << 32) and (Vw - 2) * Ve * 4 > (1 << 32)
    last = M // B - 1
    c = dict(Rw=Rw, W=W, b=b, Nv0=Nv0, X=X[last * B:], y=y[last * B:], w=w[last * B:], Vw=Vw, Nw=Nw, Ve=Ve, d=d, n=n, B=B, lam=lam)
    eng = U.ll_engine(dict(Rw=Rw, W=W, b=b, X=X), _MODEL_B, n, 0.01, keep_grads=0)
    try:
        f = C.LlWordFoldIn(eng, Nv0, B, lam)
        f.upload(X, y, w)
        t32, t64 = LW.LlWordFoldInTwin(c), LW.LlWordFoldInTwin(c, np.float64)
        got_eval, ref_eval = f.eval_batch(last), t32.eval_loss(0)
        assert abs(got_eval - ref_eval) <= 1e-5 * abs(ref_eval), (got_eval, ref_eval)
        got, ref = f.train_batch(last), t32.train_step(0)
        t64.train_step(0)
        print('batch %d of a %.2f GiB table: loss %.7f oracle %.7f' % (last, Vw * Ve * 4 / 2.0 ** 30, got, ref))
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        assert f.plan()['form'] == 'stream' and f.plan()['vec'] and f.plan()['splits'] > 1
        _check_against_twins(f, t32, t64, 'past 4 GiB')
        f.close()
    finally:
        eng.close()


def test_a_frozen_table_that_cannot_be_allocated_keeps_the_earlier_upload(hip_lib):
    """The allocation branch of the upload, apart from the max_cache_bytes one: 800 000 distinct frozen words x 100 000 entities
    need 320 GB, more than the device holds.  One request, refused by hipMalloc before anything of the handle is touched: the
    message names the bytes needed, the earlier upload is kept and trains as before."""
    Vw, Nw, Ve, d, n, B = 800000, 2, 100000, 4, 2, 2
    rng = np.random.RandomState(78)
    p = dict(Rw=U.O.glorot_uniform(rng, (Vw, d)), W=U.O.glorot_uniform(rng, (d, Ve)), b=np.zeros(Ve, np.float32),
             X=np.zeros((1, n), np.int32))
    Nv0 = (0.5 * rng.randn(Nw, d)).astype(np.float32)
    eng = U.ll_engine(p, _MODEL_B, n, 0.01, keep_grads=0)
    try:
        f = C.LlWordFoldIn(eng, Nv0, B, 0.01)
        small_x = np.array([[0, Vw], [1, Vw + 1], [Vw, 2], [3, 4]], np.int32)
        small_y = np.array([5, 6, 7, 8], np.int32)
        f.upload(small_x, small_y, None)
        first = f.eval_batch(0)
        X = np.arange(Vw, dtype=np.int32).reshape(Vw // n, n)          # every trained word once
        need = Vw * Ve * 4
        with pytest.raises(C.SertError, match='needs %d bytes, which cannot be allocated' % need):
            f.upload(X, np.zeros(Vw // n, np.int32), None)
        assert f.num_batches() == 2
        assert U.same_bits(np.float32(first), np.float32(f.eval_batch(0))) and np.isfinite(f.train_batch(1))
        f.close()
    finally:
        eng.close()


def test_python_loglinear_word_foldin_model(hip_lib):
    """sert_amd.foldin.LogLinearWordFoldIn from host arrays: two shuffled epochs track the twin on the traced batches; the
    extended table, and the optimiser state through get_optimizer_state / set_optimizer_state into a second model, which then
    holds the bits of the first."""
    from sert_amd import foldin
    c = LW.make_case('base')

    def make():
        return foldin.LogLinearWordFoldIn(c['Rw'], c['W'], c['b'], c['Nv0'], (c['X'], c['y'], c['w']), batch_size=c['B'],
                                          regularization_lambda=c['lam'], window_size=c['n'])

    np.random.seed(7)           # (the order of the batches inside an epoch)
    fold = make()
    trace, step = [], fold.train_fn
    fold.train_fn = lambda i: (trace.append(i), step(i))[1]
    first, _ = fold.train_error()
    for _ in range(2):
        num_batches, loss = fold.train()
        assert num_batches == c['batches'] and np.isfinite(loss)
    assert len(trace) == 2 * c['batches'] and np.isfinite(first)
    t32, t64 = LW.LlWordFoldInTwin(c), LW.LlWordFoldInTwin(c, np.float64)
    for batch_index in trace:
        t32.train_step(batch_index)
        t64.train_step(batch_index)
    Nv = fold.get_new_word_representations()
    print(U.check_tensor('new word rows after %d steps' % len(trace), Nv, t32.Nv, t64.Nv))
    ext = fold.get_extended_word_representations(c['Rw'])
    assert ext.shape == (c['Vw'] + c['Nw'], c['d']) and U.same_bits(ext[:c['Vw']], c['Rw']) and U.same_bits(ext[c['Vw']:], Nv)
    st = fold.get_optimizer_state()
    assert sorted(st) == ['accu_Nv', 'delta_Nv'] and st['accu_Nv'].shape == Nv.shape and np.abs(st['accu_Nv']).max() > 0
    other = make()
    other._foldin.set_rows(C.LL_WFOLD_ROWS, Nv)
    other.set_optimizer_state(st)
    assert U.same_bits(np.float32(fold._foldin.train_batch(1)), np.float32(other._foldin.train_batch(1)))
    for a, b in zip(_state(fold._foldin), _state(other._foldin)):
        assert U.same_bits(a, b)
    with pytest.raises(RuntimeError, match='nothing says how many words are new'):
        foldin.LogLinearWordFoldIn(c['Rw'], c['W'], c['b'], None, (np.zeros((4, c['n']), np.int32), np.zeros(4, np.int32)),
                                   batch_size=2, regularization_lambda=0.0, window_size=c['n'])
    fold.close()
    other.close()


def test_python_loglinear_word_foldin_from_a_live_model(hip_lib):
    """sert_amd.foldin.LogLinearWordFoldIn.from_model: the parameters of a live models.LanguageModel are copied on the device as
    they are at that moment.  Three steps track the twin, hold the bits of a fold-in built from the same parameters as host
    arrays, and training the model on or dropping it afterwards changes nothing the handle computes."""
    from sert_amd import foldin, models
    c = LW.make_case('base')
    B, Vw = c['B'], c['Vw']
    trained = (np.minimum(c['X'], Vw - 1), c['y'], c['w'])          # the model's own instances: trained words only
    model = models.LanguageModel(batch_size=B, window_size=c['n'], representations_init=c['Rw'], output_layer_size=c['Ve'],
                                 regularization_lambda=0.01, training_set=trained,
                                 validation_set=(trained[0][:B], trained[1][:B]))
    model.set_dense(c['W'], c['b'])
    with pytest.raises(RuntimeError, match='needs a LanguageModel'):
        foldin.LogLinearWordFoldIn.from_model(object(), c['Nv0'], (c['X'], c['y'], c['w']), B, c['lam'])
    live = foldin.LogLinearWordFoldIn.from_model(model, c['Nv0'], (c['X'], c['y'], c['w']), B, c['lam'])
    host = foldin.LogLinearWordFoldIn(c['Rw'], c['W'], c['b'], c['Nv0'], (c['X'], c['y'], c['w']), batch_size=B,
                                      regularization_lambda=c['lam'], window_size=c['n'])
    assert live.num_new_words == c['Nw'] and live.vocab_size == Vw and live.window_size == c['n']
    t32, t64 = LW.LlWordFoldInTwin(c), LW.LlWordFoldInTwin(c, np.float64)
    for s in range(LW.STEPS):
        if s == 1:
            model.train()                   # the model moves on: the handle holds its own copy
        if s == 2:
            model._engine.close()           # ... and is dropped
        got, same = live._foldin.train_batch(s), host._foldin.train_batch(s)
        ref = t32.train_step(s)
        t64.train_step(s)
        assert U.same_bits(np.float32(got), np.float32(same)) and abs(got - ref) <= 1e-5 * abs(ref), (s, got, same, ref)
    _check_against_twins(live._foldin, t32, t64, 'from_model after %d steps' % LW.STEPS)
    for a, b in zip(_state(live._foldin), _state(host._foldin)):
        assert U.same_bits(a, b)
    live.close()
    host.close()
