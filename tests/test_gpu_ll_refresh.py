"""GPU: a loglinear fold-in that refreshes trained columns (sert_ll_foldin_create_refresh, include/sert_hip_ll_foldin.h;
csrc/kernels_ll_foldin.h: llf_compact; csrc/ll_label_remap.h) against its oracle twin (tests/ll_refresh_cases.py) with the
bounds of tests/test_gpu_ll_foldin.py -- loss 1e-5 relative, the six tensors through tests.util.check_tensor against the
float32 and the float64 twin -- and, bit for bit, against the plain handle on the column-deleted model: the step kernels are
the plain fold-in's, only the columns they see were permuted once."""
import ctypes

import numpy as np
import pytest

from sert_amd import _capi as C
from tests import ll_foldin_cases as LC
from tests import ll_foldin_label_cases as LL
from tests import ll_refresh_cases as RC
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own
_STATE = (('W', C.LL_FOLDIN_W), ('b', C.LL_FOLDIN_B), ('accu.W', C.LL_FOLDIN_ACCU_W), ('accu.b', C.LL_FOLDIN_ACCU_B),
          ('delta.W', C.LL_FOLDIN_DELTA_W), ('delta.b', C.LL_FOLDIN_DELTA_B))


def _engine(c):
    return U.ll_engine(dict(Rw=c['Rw'], W=c['W'], b=c['b'], X=c['X']), _MODEL_B, c['n'], 0.01, keep_grads=0)


def _upload(f, c):
    if RC.is_csr(c):
        f.upload_csr(c['X'], c['indptr'], c['indices'], c['data'], c['w'])
    else:
        f.upload(c['X'], c['y'], c['w'])


def _handle(c, eng, upload=True, **kw):
    """the refresh handle of a case of tests/ll_refresh_cases.py"""
    f = C.LlFoldIn(eng, c['Wn0'] if c['N'] else None, c['bn0'] if c['N'] else None, c['B'], c['lam'], refresh_ids=c['refresh'], **kw)
    assert (f.num_refresh, f.num_new, f.num_slots) == (c['R'], c['N'], c['Nt'])
    if upload:
        _upload(f, c)
    return f


def _plain(p, eng, upload=True):
    """the plain handle (sert_ll_foldin_create) of a case whose every new column is given"""
    f = C.LlFoldIn(eng, p['Wn0'], p['bn0'], p['B'], p['lam'])
    if upload:
        _upload(f, p)
    return f


def _state(f):
    return [f.get_tensor(which) for _, which in _STATE]


def _same(a, b):
    return len(a) == len(b) and all(U.same_bits(x, y) for x, y in zip(a, b))


@pytest.fixture(scope='module', params=sorted(RC.CASES))
def case(request):
    return RC.make_case(request.param)


@pytest.fixture(scope='module', params=sorted(k for k in RC.CASES if RC.make_case(k)['Vf'] >= 1))
def case_with_frozen(request):
    """(a loglinear engine needs at least one entity: the column-deleted model of a V_f = 0 case does not exist)"""
    return RC.make_case(request.param)


def test_parity(hip_lib, case):
    """Every case for three steps (step s trains batch s): the loss of each step, then Wt, bt and the four accumulators in
    slot order."""
    c = case
    eng = _engine(c)
    try:
        f = _handle(c, eng)
        assert f.num_batches() == c['batches']
        t32, t64 = RC.LlRefreshTwin(c), RC.LlRefreshTwin(c, np.float64)
        assert U.same_bits(f.get_tensor(C.LL_FOLDIN_W), t32.Wt) and U.same_bits(f.get_tensor(C.LL_FOLDIN_B), t32.bt)
        for s in range(RC.STEPS):
            got = f.train_batch(s)
            ref = t32.train_step(s)
            t64.train_step(s)
            print('%s step %d: loss %.7f oracle %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
        s32, s64 = t32.state(), t64.state()
        log = []
        for name, which in _STATE:
            got = f.get_tensor(which)
            got = got.reshape(1, -1) if got.ndim == 1 else got
            square = name.rpartition('.')[0] in U.SECOND_MOMENTS
            log.append(U.check_tensor('%s %s' % (c['name'], name), got, s32[name], s64[name], row_tol32=U.state_row_tol32(name),
                                      row_tol64=(2 if square else 1) * U.ROW_TOL64))
        print('\n'.join(log))
        if c['name'] == 'unvisited_slot':
            assert not U.same_bits(f.get_tensor(C.LL_FOLDIN_W)[:, 2], c['W'][:, c['refresh'][2]])
        f.close()
    finally:
        eng.close()


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch = the twin's eval_loss on the device's tensors (unweighted, unregularised), after one training step; no state
    bit changes."""
    c = case
    eng = _engine(c)
    f = _handle(c, eng)
    try:
        tw = RC.LlRefreshTwin(c)
        f.train_batch(0)
        before = _state(f)
        tw.Wt[...] = before[0]
        tw.bt[...] = before[1]
        for batch in (1, 2):
            got, ref = f.eval_batch(batch), tw.eval_loss(batch)
            print('%s eval batch %d: %.7f oracle %.7f' % (c['name'], batch, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], batch, got, ref)
        assert _same(before, _state(f))
    finally:
        f.close()
        eng.close()


def test_bits_of_the_plain_handle_on_the_column_deleted_model(hip_lib, case_with_frozen):
    """The refresh handle and C.LlFoldIn on an engine holding the frozen columns only, with num_new = Nt, hold the same bits in
    loss and all six tensors after three steps, through train_batch and through train_batches, for integer labels and label
    rows: no step kernel changed, and the host re-sort of the rows is right.  A second refresh handle: the same bits again."""
    c = case_with_frozen
    p = RC.deleted(c)
    eng, eng_deleted = _engine(c), _engine(p)
    try:
        a, a2, b = _handle(c, eng), _handle(c, eng), _plain(p, eng_deleted)
        assert _same(_state(a), _state(b))                                  # (the compaction wrote the trained columns)
        la = np.asarray([a.train_batch(s) for s in range(RC.STEPS)], np.float32)
        lb = np.asarray([b.train_batch(s) for s in range(RC.STEPS)], np.float32)
        l2 = a2.train_batches(list(range(RC.STEPS)))
        assert U.same_bits(la, lb) and U.same_bits(la, l2), (c['name'], la, lb, l2)
        assert _same(_state(a), _state(b)) and _same(_state(a), _state(a2))
        assert not U.same_bits(_state(a)[0], p['Wn0'])
        for e in (1, 2):
            assert U.same_bits(np.float32(a.eval_batch(e)), np.float32(b.eval_batch(e)))
        for h in (a, a2, b):
            h.close()
    finally:
        eng.close()
        eng_deleted.close()


def test_no_refreshed_id_is_the_plain_handle(hip_lib):
    """num_refresh == 0: the bits of sert_ll_foldin_create on the same inputs, for integer labels and for label rows."""
    for c in (LC.make_case('base'), LL.make_case('mixed')):
        eng = _engine(c)
        try:
            a = C.LlFoldIn(eng, c['Wn0'], c['bn0'], c['B'], c['lam'], refresh_ids=np.zeros(0, np.int32))
            b = _plain(c, eng, upload=False)
            assert (a.num_refresh, a.num_slots) == (0, c['N'])
            vf, nt, io = a.layout()
            assert (vf, nt) == (c['Ve'], c['N']) and np.array_equal(io, np.arange(c['Ve'] + c['N']))
            for h in (a, b):
                _upload(h, c)
            la = np.asarray([a.train_batch(s) for s in range(3)], np.float32)
            lb = np.asarray([b.train_batch(s) for s in range(3)], np.float32)
            assert U.same_bits(la, lb) and _same(_state(a), _state(b))
            a.close()
            b.close()
        finally:
            eng.close()


def test_layout(hip_lib, case):
    """sert_debug_ll_foldin_layout: V_f, Nt and the public-to-internal column map of every case."""
    c = case
    eng = _engine(c)
    try:
        f = _handle(c, eng, upload=False)
        vf, nt, io = f.layout()
        assert (vf, nt) == (c['Vf'], c['Nt']) and np.array_equal(io, RC.internal_of(c))
        out = np.zeros(3, np.int32)
        with pytest.raises(C.SertError, match='count must be'):
            C.check(C.load().sert_debug_ll_foldin_layout(f._h, None, None, out.ctypes.data, 3))
        f.close()
    finally:
        eng.close()


def test_frozen_tensors_stay_frozen(hip_lib):
    """mixed: the untouched columns of get_extended_dense and the engine's own R_w, W, b hold the same bits before and after;
    the refreshed columns moved; training the model after the handle was created, and closing it, does not change the handle."""
    from sert_amd import foldin
    c = RC.make_case('mixed')
    ids = (C.T_RW, C.T_W, C.T_B)
    results = []
    for disturb in (False, True):
        eng = _engine(c)
        before = [eng.get_tensor(t).copy() for t in ids]
        f = _handle(c, eng)
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
    assert _same(*results)
    # the Python layer on host arrays: refreshed columns replaced, new ones appended, everything else bit for bit
    W0, b0 = c['W'].copy(), c['b'].copy()
    fold = foldin.LogLinearFoldIn(c['Rw'], c['W'], c['b'], c['Wn0'], c['bn0'], (c['X'], c['y'], c['w']), batch_size=c['B'],
                                  regularization_lambda=c['lam'], window_size=c['n'], refresh=c['refresh'])
    for s in range(3):
        fold.train_fn(s)
    Wx, bx = fold.get_extended_dense(c['W'], c['b'])
    Wr, br = fold.get_refreshed_dense()
    Wn, bn = fold.get_new_dense()
    fold.close()
    Ve, frozen = c['Ve'], np.setdiff1d(np.arange(c['Ve']), c['refresh'])
    assert U.same_bits(c['W'], W0) and U.same_bits(c['b'], b0)                # (the caller's arrays are not modified)
    assert Wx.shape == (c['d'], Ve + c['N']) and bx.shape == (Ve + c['N'],)
    assert U.same_bits(Wx[:, frozen], W0[:, frozen]) and U.same_bits(bx[frozen], b0[frozen])
    assert U.same_bits(Wx[:, c['refresh']], Wr) and U.same_bits(bx[c['refresh']], br)
    assert U.same_bits(Wx[:, Ve:], Wn) and U.same_bits(bx[Ve:], bn)
    assert U.same_bits(Wr, results[0][1][:, :c['R']]) and U.same_bits(Wn, results[0][1][:, c['R']:])
    assert np.isfinite(Wx).all() and np.isfinite(bx).all()
    for s, e in enumerate(c['refresh']):
        assert not U.same_bits(Wr[:, s], W0[:, e]) and br[s] != b0[e]


def test_either_upload_form_after_the_other(hip_lib):
    """csr_mixed: integer labels, then label rows, then integer labels again on ONE handle -- the optimiser state is kept -- give
    the bits of the plain handle on the column-deleted model that is taken through the same uploads."""
    c = RC.make_case('csr_mixed')
    p = RC.deleted(c)
    y = np.random.RandomState(11).randint(0, c['Nt'], c['M']).astype(np.int32)
    eng, eng_deleted = _engine(c), _engine(p)
    try:
        a, b = _handle(c, eng, upload=False), _plain(p, eng_deleted, upload=False)
        losses = [[], []]
        for k, (h, q) in enumerate(((a, c), (b, p))):
            h.upload(q['X'], y, q['w'])
            losses[k].append(h.train_batch(0))
            _upload(h, q)
            losses[k] += [h.train_batch(1), h.eval_batch(0)]
            assert np.abs(h.get_tensor(C.LL_FOLDIN_ACCU_W)).max() > 0
            h.upload(q['X'], y, q['w'])
            losses[k].append(h.train_batch(2))
        assert U.same_bits(np.asarray(losses[0], np.float32), np.asarray(losses[1], np.float32))
        assert _same(_state(a), _state(b))
        # ... and the twin agrees on the first step of each form
        tw = RC.LlRefreshTwin(dict((k, v) for k, v in c.items() if k not in ('indptr', 'Ydense')), np.float32)
        tw.c['y'] = y
        ref = tw.train_step(0)
        assert abs(losses[0][0] - ref) <= 1e-5 * abs(ref)
        a.close()
        b.close()
    finally:
        eng.close()
        eng_deleted.close()


def test_refusals(hip_lib):
    """Every refusal of sert_ll_foldin_create_refresh and of the uploads on a refresh handle comes back nonzero with its message
    -- validated on the host, before any launch -- while the earlier upload still trains."""
    c = RC.make_case('mixed')
    B, N, R, Nt, Ve, d, n = c['B'], c['N'], c['R'], c['Nt'], c['Ve'], c['d'], c['n']
    lib = C.load()
    eng = _engine(c)
    try:
        cfg = C.SertLlFoldInConfig()
        cfg.struct_size, cfg.batch_size, cfg.lambda_, cfg.lr, cfg.rho, cfg.eps = ctypes.sizeof(C.SertLlFoldInConfig), B, 0.01, 1.0, 0.95, 1e-6
        ids, Wn = np.asarray(c['refresh'], np.int32), np.ascontiguousarray(c['Wn0'])

        def create(ids_ptr, num_refresh, num_new, w_ptr, config=cfg):
            h = ctypes.c_void_p()
            rc = lib.sert_ll_foldin_create_refresh(eng._h, ids_ptr, num_refresh, num_new, w_ptr, None, ctypes.byref(config), ctypes.byref(h))
            assert (rc != 0) == (not h)
            C.check(rc)
            return h

        with pytest.raises(C.SertError, match='num_refresh >= 0 and num_new >= 0'):
            create(ids.ctypes.data, -1, N, Wn.ctypes.data)
        with pytest.raises(C.SertError, match='num_refresh >= 0 and num_new >= 0'):
            create(ids.ctypes.data, R, -1, Wn.ctypes.data)
        with pytest.raises(C.SertError, match='at least one trainable column'):
            create(None, 0, 0, None)
        with pytest.raises(C.SertError, match='null refresh_ids'):
            create(None, R, N, Wn.ctypes.data)
        with pytest.raises(C.SertError, match='refresh_ids must be NULL'):
            create(ids.ctypes.data, 0, N, Wn.ctypes.data)
        with pytest.raises(C.SertError, match='null init_new_W'):
            create(ids.ctypes.data, R, N, None)
        with pytest.raises(C.SertError, match='init_new_W must be NULL'):
            create(ids.ctypes.data, R, 0, Wn.ctypes.data)
        for bad in (-1, Ve):
            with pytest.raises(C.SertError, match=r'refresh id out of range \[0, num_entities\)'):
                C.LlFoldIn(eng, c['Wn0'], None, B, 0.01, refresh_ids=[5, bad])
        with pytest.raises(C.SertError, match='duplicate refresh id'):
            C.LlFoldIn(eng, c['Wn0'], None, B, 0.01, refresh_ids=[5, 1, 5])
        with pytest.raises(C.SertError, match='1-d array of int32'):
            C.LlFoldIn(eng, c['Wn0'], None, B, 0.01, refresh_ids=[0.5])
        # what sert_ll_foldin_create refuses, the size limits on Nt
        with pytest.raises(C.SertError, match='batch_size >= 1'):
            C.LlFoldIn(eng, c['Wn0'], None, 0, 0.01, refresh_ids=c['refresh'])
        with pytest.raises(C.SertError, match='lambda must be >= 0'):
            C.LlFoldIn(eng, c['Wn0'], None, B, -0.5, refresh_ids=c['refresh'])
        with pytest.raises(C.SertError, match='rho'):
            C.LlFoldIn(eng, c['Wn0'], None, B, 0.01, rho=1.0, refresh_ids=c['refresh'])
        big = (2 ** 31 - 1) // (n * Nt) + 1              # B n Nt just above 2^31 - 1 (B n N alone is below)
        assert big * n * Nt > 2 ** 31 - 1 >= big * n * N
        with pytest.raises(C.SertError, match=r'batch_size \* window_size \* \(num_refresh \+ num_new\)'):
            C.LlFoldIn(eng, c['Wn0'], None, big, 0.01, refresh_ids=c['refresh'])
        short = C.SertLlFoldInConfig()
        short.struct_size, short.batch_size, short.rho, short.eps = ctypes.sizeof(C.SertLlFoldInConfig) - 4, B, 0.95, 1e-6
        with pytest.raises(C.SertError, match='size mismatch'):
            create(ids.ctypes.data, R, N, Wn.ctypes.data, short)
        kw = dict(batch_size=8, global_batch_size=8, window_size=n, vocab_size=c['Vw'], num_entities=Ve, word_dim=d, entity_dim=8,
                  id_bytes=4, device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
        vs = C.Engine(kind=C.KIND_VECTORSPACE, num_negatives=2, **kw)
        with pytest.raises(C.SertError, match='needs a loglinear model'):
            C.LlFoldIn(vs, c['Wn0'], None, B, 0.01, refresh_ids=c['refresh'])
        vs.close()
        # the logit cache counts the V_f frozen columns
        distinct = np.unique(c['X']).size
        need = distinct * c['Vf'] * 4
        capped = _handle(c, eng, upload=False, max_cache_bytes=need - 1)
        with pytest.raises(C.SertError, match='needs %d bytes .%d distinct words x %d entities' % (need, distinct, c['Vf'])):
            _upload(capped, c)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            capped.train_batch(0)
        exact = _handle(c, eng, upload=False, max_cache_bytes=need)
        _upload(exact, c)
        # the uploads: y is a slot in [0, Nt)
        f = _handle(c, eng, upload=False)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.eval_batch(0)
        _upload(f, c)
        for bad in (-1, Nt):
            y = c['y'].copy()
            y[7] = bad
            with pytest.raises(C.SertError, match=r'label out of range \[0, num_refresh \+ num_new\): y is a slot'):
                f.upload(c['X'], y, c['w'])
        X = c['X'].copy()
        X[3, 1] = c['Vw']
        with pytest.raises(C.SertError, match='token id out of range'):
            f.upload(X, c['y'], c['w'])
        # label rows: the PUBLIC columns [0, V_e + num_new), strictly increasing in the public order
        indptr = np.arange(c['M'] + 1, dtype=np.int64)
        cols = np.full(c['M'], 1, np.int32)
        ones = np.ones(c['M'], np.float32)
        for bad in (-1, Ve + N):
            cols2 = cols.copy()
            cols2[5] = bad
            with pytest.raises(C.SertError, match=r'label column out of range \[0, V_e \+ num_new\)'):
                f.upload_csr(c['X'], indptr, cols2, ones, c['w'])
        two = np.arange(0, 2 * c['M'] + 1, 2, dtype=np.int64)
        with pytest.raises(C.SertError, match='not strictly increasing'):
            # (5 then 1: slots 0 then 1 -- increasing in slot order, not in the public order the contract is stated in)
            f.upload_csr(c['X'], two, np.tile(np.asarray([5, 1], np.int32), c['M']), np.ones(2 * c['M'], np.float32), c['w'])
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batch(c['batches'])
        with pytest.raises(C.SertError, match='element count'):
            f.set_tensor(C.LL_FOLDIN_W, np.zeros((d, N), np.float32))              # (d Nt values, not d num_new)
        # nothing above moved the handles: the earlier upload still trains, as a fresh handle does
        ref = RC.LlRefreshTwin(c).train_step(0)
        for h in (f, exact):
            got = h.train_batch(0)
            assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
            h.close()
        capped.close()
    finally:
        eng.close()
