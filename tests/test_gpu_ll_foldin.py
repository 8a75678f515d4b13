"""GPU: folding unseen entities into a trained loglinear model (include/sert_hip_ll_foldin.h, csrc/kernels_ll_foldin.h) against
its oracle twin (tests/ll_foldin_cases.py: LogLinearOracle / Adadelta on the extended tensors).  Loss 1e-5 relative; Wn, bn
and the four accumulators through tests.util.check_tensor with the bounds tests/util.py assigns to the loglinear model's W / b
and their second moments, against the float32 twin and the float64 one."""
import ctypes

import numpy as np
import pytest

from sert_amd import _capi as C
from tests import ll_foldin_cases as LC
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own
_STATE = (('W', C.LL_FOLDIN_W), ('b', C.LL_FOLDIN_B), ('accu.W', C.LL_FOLDIN_ACCU_W), ('accu.b', C.LL_FOLDIN_ACCU_B),
          ('delta.W', C.LL_FOLDIN_DELTA_W), ('delta.b', C.LL_FOLDIN_DELTA_B))


def _engine(c, n=None):
    return U.ll_engine(dict(Rw=c['Rw'], W=c['W'], b=c['b'], X=c['X']), _MODEL_B, c['n'] if n is None else n, 0.01, keep_grads=0)


def _foldin(c, eng, upload=True, **kw):
    f = C.LlFoldIn(eng, c['Wn0'], c['bn0'], c['B'], c['lam'], **kw)
    if upload:
        f.upload(c['X'], c['y'], c['w'])
    return f


def _state(f):
    return [f.get_tensor(which) for _, which in _STATE]


def _check_against_twins(f, t32, t64, label):
    s32, s64 = t32.state(), t64.state()
    log = []
    for name, which in _STATE:
        got = f.get_tensor(which)
        got = got.reshape(1, -1) if got.ndim == 1 else got
        square = name.rpartition('.')[0] in U.SECOND_MOMENTS
        log.append(U.check_tensor('%s %s' % (label, name), got, s32[name], s64[name], row_tol32=U.state_row_tol32(name),
                                  row_tol64=(2 if square else 1) * U.ROW_TOL64))
    print('\n'.join(log))


@pytest.fixture(scope='module', params=sorted(LC.CASES))
def case(request):
    return LC.make_case(request.param)


def test_parity(hip_lib, case):
    """Every case for three steps (step s trains batch s): the loss of each step, then Wn, bn and the four accumulators."""
    c = case
    eng = _engine(c)
    try:
        f = _foldin(c, eng)
        assert f.num_batches() == c['batches']
        t32, t64 = LC.LlFoldInTwin(c), LC.LlFoldInTwin(c, np.float64)
        for s in range(LC.STEPS):
            got = f.train_batch(s)
            ref = t32.train_step(s)
            t64.train_step(s)
            print('%s step %d: loss %.7f oracle %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
        _check_against_twins(f, t32, t64, c['name'])
        f.close()
    finally:
        eng.close()


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch = the twin's eval_loss evaluated on the device's tensors (unweighted, unregularised), after one training
    step; no state bit changes."""
    c = case
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        tw = LC.LlFoldInTwin(c)
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


def test_frozen_and_snapshot(hip_lib):
    """The model's three tensors hold the same bits before and after a fold-in; training the model after the handle was
    created, and closing it, does not change what the handle computes."""
    c = LC.make_case('base')
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


def test_reproducible_and_train_batches(hip_lib):
    """Two handles hold the same bits after five steps over [0, 2, 1, 1, 0]; train_batches (one synchronisation) gives the
    bits of the train_batch loop; the state round-trips through get_tensor / set_tensor."""
    c = LC.make_case('base')
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
        d = _foldin(c, eng)
        for (_, which), val in zip(_STATE, _state(a)):
            d.set_tensor(which, val)
        assert U.same_bits(np.float32(a.train_batch(1)), np.float32(d.train_batch(1)))
        for x, y in zip(_state(a), _state(d)):
            assert U.same_bits(x, y)
        for h in (a, b, d):
            h.close()
    finally:
        eng.close()


def test_refusals(hip_lib):
    """Every refusal of the contract comes back nonzero with its message -- validated on the host, nothing is launched on bad
    ids -- and the handle trains normally afterwards."""
    c = LC.make_case('base')
    B, N, d, n = c['B'], c['N'], c['d'], c['n']
    # a vectorspace model, the full-softmax kind, a model with a communicator, a window of 33
    kw = dict(batch_size=8, global_batch_size=8, window_size=n, vocab_size=c['Vw'], num_entities=c['Ve'], word_dim=d, entity_dim=8,
              id_bytes=4, device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
    vs = C.Engine(kind=C.KIND_VECTORSPACE, num_negatives=2, **kw)
    with pytest.raises(C.SertError, match='needs a loglinear model'):
        C.LlFoldIn(vs, c['Wn0'], None, B, 0.01)
    vs.close()
    fs = C.Engine(kind=C.KIND_VECTORSPACE_SOFTMAX, num_negatives=0, **kw)
    with pytest.raises(C.SertError, match='SOFTMAX'):
        C.LlFoldIn(fs, c['Wn0'], None, B, 0.01)
    fs.close()
    dp = _engine(c)
    dp.comm_init(C.comm_unique_id(), 0, 1)
    with pytest.raises(C.SertError, match='communicator'):
        C.LlFoldIn(dp, c['Wn0'], None, B, 0.01)
    dp.close()
    wide = _engine(c, n=33)
    with pytest.raises(C.SertError, match='window sizes up to 32'):
        C.LlFoldIn(wide, c['Wn0'], None, B, 0.01)
    wide.close()
    eng = _engine(c)
    try:
        with pytest.raises(C.SertError, match='at least one new entity'):
            C.LlFoldIn(eng, np.zeros((d, 0), np.float32), None, B, 0.01)
        with pytest.raises(C.SertError, match='batch_size >= 1'):
            C.LlFoldIn(eng, c['Wn0'], None, 0, 0.01)
        with pytest.raises(C.SertError, match='lambda must be >= 0'):
            C.LlFoldIn(eng, c['Wn0'], None, B, -0.5)
        with pytest.raises(C.SertError, match='rho'):
            C.LlFoldIn(eng, c['Wn0'], None, B, 0.01, rho=1.0)
        cfg = C.SertLlFoldInConfig()
        cfg.struct_size, cfg.batch_size, cfg.rho, cfg.eps = ctypes.sizeof(C.SertLlFoldInConfig) - 4, B, 0.95, 1e-6
        h = ctypes.c_void_p()
        with pytest.raises(C.SertError, match='size mismatch'):
            C.check(C.load().sert_ll_foldin_create(eng._h, N, c['Wn0'].ctypes.data, None, ctypes.byref(cfg), ctypes.byref(h)))
        assert not h
        # the logit cache: one byte below need is refused with the bytes needed; the handle takes a smaller upload afterwards
        distinct = np.unique(c['X']).size
        need = distinct * c['Ve'] * 4
        capped = _foldin(c, eng, upload=False, max_cache_bytes=need - 1)
        with pytest.raises(C.SertError, match='needs %d bytes' % need):
            capped.upload(c['X'], c['y'], c['w'])
        with pytest.raises(C.SertError, match='no fold-in instances'):
            capped.train_batch(0)
        assert np.unique(c['X'][:B]).size < distinct
        capped.upload(c['X'][:B], c['y'][:B], c['w'][:B])
        exact = _foldin(c, eng, upload=False, max_cache_bytes=need)
        exact.upload(c['X'], c['y'], c['w'])
        f = _foldin(c, eng, upload=False)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.train_batch(0)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.eval_batch(0)
        for bad in (-1, N):
            y = c['y'].copy()
            y[7] = bad
            with pytest.raises(C.SertError, match=r'label out of range'):
                f.upload(c['X'], y, c['w'])
        for bad in (-1, c['Vw']):
            X = c['X'].copy()
            X[3, 1] = bad
            with pytest.raises(C.SertError, match='token id out of range'):
                f.upload(X, c['y'], c['w'])
        f.upload(c['X'], c['y'], c['w'])
        with pytest.raises(C.SertError, match='label out of range'):
            f.upload(c['X'], np.full_like(c['y'], N), c['w'])              # (a refused upload keeps the earlier one)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batch(c['batches'])               # (the trailing M mod B instances are no batch)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batches([0, c['batches']])
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.eval_batch(-1)
        with pytest.raises(C.SertError, match='element count'):
            f.set_tensor(C.LL_FOLDIN_ACCU_W, np.zeros(3, np.float32))
        out = np.zeros(N, np.float32)
        with pytest.raises(C.SertError, match='which must be'):
            C.check(C.load().sert_ll_foldin_get_tensor(f._h, 6, out.ctypes.data, out.size))
        # nothing above moved the handles: each trains as a fresh one does
        tw = LC.LlFoldInTwin(c)
        ref = tw.train_step(0)
        for h in (f, capped, exact):
            assert U.same_bits(h.get_tensor(C.LL_FOLDIN_W), c['Wn0']) and U.same_bits(h.get_tensor(C.LL_FOLDIN_B), c['bn0'])
            got = h.train_batch(0)
            assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
            h.close()
    finally:
        eng.close()


def test_end_to_end_entity_foldin_and_ranker(hip_lib):
    """20 trained + 6 new entities with 10 characteristic words each (V_w = 240, d = 16, n = 4, B = 32, lambda = 0.01): the base
    loglinear model is trained for 8 epochs on 64 instances per entity, the new entities are folded in through
    sert_amd.foldin.LogLinearFoldIn for 10 epochs on 32 instances each.  Asserted: the evaluation loss after the last epoch is
    below the one before the first; Wn and bn track the twin within the tensor tolerances; LogLinearPredictFn.rank_queries on
    the extended dump returns indices in [0, V_e + N).  The mean reciprocal rank of the new entities is logged only."""
    from sert_amd import foldin
    rng = np.random.RandomState(0)
    Vw, Ve, N, d, n, B, lam = 240, 20, 6, 16, 4, 32, 0.01
    words = [rng.choice(Vw, 10, replace=False) for _ in range(Ve + N)]

    def data(ents, per):
        y = np.repeat(ents, per)
        X = np.stack([rng.choice(words[e], n) for e in y])
        p = rng.permutation(len(y))
        return X[p].astype(np.int32), y[p].astype(np.int32)

    Xb, yb = data(np.arange(Ve), 64)
    base = dict(Rw=U.O.glorot_uniform(rng, (Vw, d)), W=U.O.glorot_uniform(rng, (d, Ve)), b=np.zeros(Ve, np.float32), X=Xb)
    eng = U.ll_engine(base, B, n, lam, keep_grads=0)
    eng.upload_dataset(C.SPLIT_TRAIN, Xb.astype(np.uint32), y_int=yb, w=np.ones(len(yb), np.float32))
    for _ in range(8):
        for i in range(len(yb) // B):
            eng.train_batch(i)
    Rw, W, b = eng.get_tensor(C.T_RW, (Vw, d)).copy(), eng.get_tensor(C.T_W, (d, Ve)).copy(), eng.get_tensor(C.T_B, (Ve,)).copy()
    eng.close()

    Xn, yn = data(np.arange(Ve, Ve + N), 32)
    yn = yn - Ve
    wn = np.ones(len(yn), np.float32)
    Wn0 = U.O.glorot_uniform(rng, (d, N))
    nb = len(yn) // B
    np.random.seed(7)           # (the order of the batches inside an epoch)
    fold = foldin.LogLinearFoldIn(Rw, W, b, Wn0, None, (Xn, yn, wn), batch_size=B, regularization_lambda=lam, window_size=n)
    trace, step = [], fold.train_fn

    def traced(batch_index):
        trace.append(batch_index)
        return step(batch_index)

    fold.train_fn = traced
    first, _ = fold.train_error()
    for _ in range(10):
        num_batches, _ = fold.train()
        assert num_batches == nb
    last, _ = fold.train_error()
    print('evaluation loss %.4f -> %.4f' % (first, last))
    assert last < first
    assert len(trace) == 10 * nb
    # the twin, on the same batches
    c = dict(Rw=Rw, W=W, b=b, Wn0=Wn0, bn0=np.zeros(N, np.float32), X=Xn, y=yn, w=wn, B=B, n=n, Ve=Ve, N=N, d=d, lam=lam)
    t32, t64 = LC.LlFoldInTwin(c), LC.LlFoldInTwin(c, np.float64)
    for batch_index in trace:
        t32.train_step(batch_index)
        t64.train_step(batch_index)
    Wn, bn = fold.get_new_dense()
    print(U.check_tensor('Wn after %d steps' % len(trace), Wn, t32.Wn, t64.Wn))
    print(U.check_tensor('bn after %d steps' % len(trace), bn.reshape(1, -1), t32.bn.reshape(1, -1), t64.bn.reshape(1, -1)))
    Wx, bx = fold.get_extended_dense(W, b)
    assert Wx.shape == (d, Ve + N) and U.same_bits(Wx[:, :Ve], W) and U.same_bits(Wx[:, Ve:], Wn)
    assert bx.shape == (Ve + N,) and U.same_bits(bx[:Ve], b) and U.same_bits(bx[Ve:], bn)
    st = fold.get_optimizer_state()
    assert st['accu_W'].shape == (d, N) and st['delta_b'].shape == (N,)
    fold.close()
    # the ranker serves the extended dump unchanged: a query = four characteristic words of a new entity
    from sert_amd import models
    trained = models.LogLinearPredictFn(R_w=Rw, W=W, b=b, window_size=n)
    args, predict_fn, R_w = foldin.extend_ll_dump('args', trained, Rw, Wn, bn)
    assert args == 'args' and R_w is Rw and U.same_bits(predict_fn.W, Wx) and U.same_bits(predict_fn.b, bx)
    assert trained.W.shape == (d, Ve)                      # (the trained predict_fn is not modified)
    ranking = predict_fn.rank_queries([[int(t) for t in words[Ve + q][:4]] for q in range(N)])
    idx = np.asarray(ranking.idx)
    assert idx.shape == (N, Ve + N) and idx.min() >= 0 and idx.max() == Ve + N - 1
    assert all(sorted(r) == list(range(Ve + N)) for r in idx.tolist())
    rr = [1.0 / (1 + int(np.nonzero(idx[q] == Ve + q)[0][0])) for q in range(N)]
    print('mean reciprocal rank of the new entities: %.3f' % float(np.mean(rr)))
