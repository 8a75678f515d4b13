"""GPU: folding unseen words into a trained vectorspace model (include/sert_hip_wfold.h, csrc/kernels_wfold.h) against its
oracle twin (tests/wfold_cases.py: VectorSpaceOracle / Adam on the extended word table).  Loss 1e-5 relative; the new rows
and Adam's moments through tests.util.check_tensor, against the float32 twin and the float64 one."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import util as U
from tests import wfold_cases as WC

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own


def _engine(c, seed=99, batch_size=_MODEL_B, Rw=None, z=2):
    Rw = c['Rw'] if Rw is None else Rw
    e = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=batch_size, global_batch_size=batch_size, window_size=c['n'],
                 vocab_size=Rw.shape[0], num_entities=c['Ve'], word_dim=c['dw'], entity_dim=c['de'], num_negatives=z, id_bytes=4,
                 device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=seed)
    for which, val in ((C.T_RW, Rw), (C.T_RE, c['Re']), (C.T_W, c['W']), (C.T_B, c['b'])):
        e.set_tensor(which, val)
    return e


def _wfold(c, eng, seed=WC.SEED, upload=True):
    f = C.WordFoldIn(eng, c['Nv0'], c['B'], c['z'], c['lam'], lr=c['lr'], seed=seed)
    if upload:
        f.upload(c['X'], c['y'], c['w'])
    return f


def _state(f):
    return f.get_rows(C.WFOLD_ROWS), f.get_rows(C.WFOLD_M), f.get_rows(C.WFOLD_V)


def _check_against_twins(f, t32, t64, label):
    Nv, m, v = _state(f)
    log = [U.check_tensor(label + ' Nv', Nv, t32.Nv, t64.Nv),
           U.check_tensor(label + ' m', m, t32.m, t64.m),
           # (a second moment: twice the row-wise bound, as tests.util.check_state)
           U.check_tensor(label + ' v', v, t32.v, t64.v, row_tol32=2 * U.ROW_TOL32, row_tol64=2 * U.ROW_TOL64)]
    print('\n'.join(log))


def _check_plan(c, plan, batch, train=True):
    """The instances the case exists for, as the launches recorded them."""
    de, dw, Nw = c['de'], c['dw'], c['Nw']
    vector = de % 4 == 0
    assert plan['project'] == ('vector' if vector else 'scalar')
    assert plan['loss'] == ('per_candidate' if vector else 'scalar') and plan['train'] == train
    assert plan['k'] == (-(-(de // 4) // 16) if vector else -(-de // 64))
    assert plan['gemm_p'] == C.debug_gemm_route(C.GEMM_FORM_PLAIN, Nw, de, dw)
    if not train:
        assert plan['levels'] == 0 and plan['gemm_g'] == 'none' and plan['segsum'] == 'none'
        return
    assert plan['gemm_g'] == C.debug_gemm_route(C.GEMM_FORM_PLAIN, Nw, dw, de, tb=1)
    _, levels = WC.index_of_batch(c, batch)
    assert plan['levels'] == len(levels) and plan['items'] == [len(l) for l in levels]
    assert plan['segsum'] == ('none' if not levels else 'rows32' if vector else 'scalar')
    want = {'heavy': 2, 'heavy3': 3}.get(c['name'], 0 if (c['name'], batch) == ('empty_batch', 1) else 1)
    assert plan['levels'] == want


@pytest.fixture(scope='module', params=sorted(WC.CASES))
def case(request):
    return WC.make_case(request.param)


def test_parity_explicit_and_replayed_negatives(hip_lib, case):
    """Every case for three steps: the loss of each step, then Nv, m and v -- with explicit negatives, and with
    device-drawn negatives replayed into the twin through sert_wfold_negatives_of_step."""
    c = case
    eng = _engine(c)
    try:
        for drawn in (False, True):
            f = _wfold(c, eng)
            assert f.num_batches() == c['batches']
            t32, t64 = WC.WordFoldInTwin(c), WC.WordFoldInTwin(c, np.float64)
            for s in range(WC.STEPS):
                assert f.get_step() == s
                if drawn:
                    neg = f.negatives_of_step(s)
                    assert neg.shape == (c['B'], c['z']) and neg.min() >= 0 and neg.max() < c['Ve']
                    got = f.train_batch(s)
                else:
                    neg = c['neg'][s]
                    got = f.train_batch(s, neg)
                _check_plan(c, f.plan(), s)
                ref = t32.train_step(s, neg)
                t64.train_step(s, neg)
                print('%s %s step %d: loss %.7f oracle %.7f' % (c['name'], 'drawn' if drawn else 'explicit', s, got, ref))
                assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], drawn, s, got, ref)
            assert f.get_step() == WC.STEPS
            _check_against_twins(f, t32, t64, '%s %s' % (c['name'], 'drawn' if drawn else 'explicit'))
            f.close()
    finally:
        eng.close()


def test_many_words_takes_the_gemm_the_dispatch_picks(hip_lib):
    """P and G of 300 rows go where the dispatch sends 300 rows; where that is another kernel than base's 5 rows get, the plans
    differ."""
    plans = {}
    for name in ('base', 'many_words'):
        c = WC.make_case(name)
        eng = _engine(c)
        f = _wfold(c, eng)
        f.train_batch(0, c['neg'][0])
        plans[name] = f.plan()
        f.close()
        eng.close()
    b, m = WC.make_case('base'), WC.make_case('many_words')
    for key, shape in (('gemm_p', lambda c: (c['Nw'], c['de'], c['dw'], 0)), ('gemm_g', lambda c: (c['Nw'], c['dw'], c['de'], 1))):
        route = lambda c: C.debug_gemm_route(C.GEMM_FORM_PLAIN, *shape(c)[:3], tb=shape(c)[3])
        assert plans['base'][key] == route(b) and plans['many_words'][key] == route(m)
        assert (plans['base'][key] != plans['many_words'][key]) == (route(b) != route(m))
    print('gemm_p %s / %s, gemm_g %s / %s' % (plans['base']['gemm_p'], plans['many_words']['gemm_p'], plans['base']['gemm_g'],
                                              plans['many_words']['gemm_g']))


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch = the twin's eval_loss on the extended word table (unweighted, unregularised), after one training step so
    that Nv differs from Nv0; no state changes, bit for bit; the evaluation stream is not the training stream."""
    c = case
    eng = _engine(c)
    f = _wfold(c, eng)
    try:
        tw = WC.WordFoldInTwin(c)
        f.train_batch(0, c['neg'][0])
        tw.train_step(0, c['neg'][0])
        before = _state(f)
        tw.Nv[...] = before[0]              # (evaluate the twin ON the device's rows: this test is about the loss)
        got = f.eval_batch(1, c['eval_neg'])
        _check_plan(c, f.plan(), 1, train=False)
        ref = tw.eval_loss(1, c['eval_neg'])
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        drawn = f.negatives_of_step(0, evaluation=True)
        got = f.eval_batch(2)
        assert f.get_eval_draws() == 1 and f.get_step() == 1
        ref = tw.eval_loss(2, drawn)
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        assert not np.array_equal(drawn, f.negatives_of_step(0))           # the odd stream is not the training stream
        for a, b in zip(before, _state(f)):
            assert U.same_bits(a, b)
    finally:
        f.close()
        eng.close()


def test_frozen_and_snapshot(hip_lib):
    """The model's four tensors hold the same bits before and after a fold-in; training the model after the handle was
    created, and destroying it, does not change what the handle computes: it ends with the bits of a handle created from an
    identical model that was left alone."""
    c = WC.make_case('base')
    results = []
    for disturb in (False, True):
        eng = _engine(c)
        before = [eng.get_tensor(t).copy() for t in (C.T_RW, C.T_RE, C.T_W, C.T_B)]
        f = _wfold(c, eng)
        losses = [f.train_batch(0)]
        if disturb:
            rng = np.random.RandomState(3)
            eng.upload_dataset(C.SPLIT_TRAIN, rng.randint(0, c['Vw'], (2 * _MODEL_B, c['n'])).astype(np.uint32),
                               y_int=rng.randint(0, c['Ve'], 2 * _MODEL_B).astype(np.int32), w=np.ones(2 * _MODEL_B, np.float32))
            eng.train_batch(0)
            assert not np.array_equal(eng.get_tensor(C.T_RE), before[1])          # the model DID move
            losses.append(f.train_batch(1))
            eng.close()
            losses.append(f.train_batch(2))
        else:
            losses += [f.train_batch(1), f.train_batch(2)]
            after = [eng.get_tensor(t) for t in (C.T_RW, C.T_RE, C.T_W, C.T_B)]
            for a, b in zip(before, after):
                assert U.same_bits(a, b)
            eng.close()
        results.append((np.asarray(losses, np.float32),) + _state(f))
        f.close()
    for a, b in zip(*results):
        assert U.same_bits(a, b)


@pytest.mark.parametrize('name', ['base', 'heavy'])
def test_reproducible_and_train_batches(hip_lib, name):
    """Two handles with one seed hold the same bits after five steps, in Nv, m, v and every loss, and train_batches (one
    synchronisation) gives the bits of the train_batch loop; another seed draws other negatives; a round trip through get_rows /
    set_rows / set_step continues with the same bits."""
    c = WC.make_case(name)
    eng = _engine(c)
    order = [0, 2, 1, 1, 0]
    try:
        a, b, d = _wfold(c, eng), _wfold(c, eng), _wfold(c, eng, seed=WC.SEED + 1)
        la = np.asarray([a.train_batch(i) for i in order], np.float32)
        lb = b.train_batches(order)
        assert U.same_bits(la, lb) and a.get_step() == b.get_step() == 5
        for x, y in zip(_state(a), _state(b)):
            assert U.same_bits(x, y)
        assert not np.array_equal(a.negatives_of_step(0), d.negatives_of_step(0))
        assert np.array_equal(a.negatives_of_step(3), b.negatives_of_step(3))
        d2 = _wfold(c, eng)
        for which, val in zip((C.WFOLD_ROWS, C.WFOLD_M, C.WFOLD_V), _state(a)):
            d2.set_rows(which, val)
        d2.set_step(5)
        assert U.same_bits(np.float32(a.train_batch(1)), np.float32(d2.train_batch(1)))
        for x, y in zip(_state(a), _state(d2)):
            assert U.same_bits(x, y)
        for h in (a, b, d, d2):
            h.close()
    finally:
        eng.close()


def test_upload_without_a_new_token_is_the_models_evaluation(hip_lib):
    """An upload with no new token at all: eval_batch with explicit negatives equals the model's own evaluation loss on the same
    instances and negatives within 1e-5 (T = tanh(A0): the model's forward), and a training step moves the rows by L2 and its
    moments only."""
    c = WC.make_case('base')
    X = np.where(c['X'] >= c['Vw'], c['X'] - c['Vw'], c['X']).astype(np.int32)
    eng = _engine(c, batch_size=c['B'], z=c['z'])
    f = _wfold(c, eng, upload=False)
    try:
        f.upload(X, c['y'], c['w'])
        eng.upload_dataset(C.SPLIT_TRAIN, X.astype(np.uint32), y_int=c['y'], w=c['w'])
        for batch in range(c['batches']):
            got, ref = f.eval_batch(batch, c['eval_neg']), eng.eval_batch(C.SPLIT_TRAIN, batch, c['eval_neg'])
            assert abs(got - ref) <= 1e-5 * abs(ref), (batch, got, ref)
        f.train_batch(0, c['neg'][0])
        assert f.plan()['levels'] == 0
        k = np.float32(c['lam'] / c['B'])
        assert np.allclose(f.get_rows(C.WFOLD_M), 0.1 * k * c['Nv0'], rtol=1e-5, atol=0)
    finally:
        f.close()
        eng.close()


def test_the_extended_table_is_the_model(hip_lib):
    """An Engine created with V_w + Nw words and R_w = get_extended_word_representations evaluates the uploaded batches, on the
    same negatives, to the handle's eval_batch within 1e-5."""
    c = WC.make_case('base')
    eng = _engine(c)
    f = _wfold(c, eng)
    for s in range(WC.STEPS):
        f.train_batch(s, c['neg'][s])
    ext = np.concatenate([c['Rw'], f.get_rows()], axis=0)
    eng.close()
    full = _engine(c, batch_size=c['B'], Rw=ext, z=c['z'])
    try:
        full.upload_dataset(C.SPLIT_TRAIN, c['X'].astype(np.uint32), y_int=c['y'], w=c['w'])
        for batch in range(c['batches']):
            got, ref = f.eval_batch(batch, c['eval_neg']), full.eval_batch(C.SPLIT_TRAIN, batch, c['eval_neg'])
            print('batch %d: fold-in %.7f full model %.7f' % (batch, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (batch, got, ref)
    finally:
        f.close()
        full.close()


def test_refusals(hip_lib):
    """Everything the contract puts out of scope comes back nonzero with a message -- validated on the host, nothing is
    launched on bad ids -- and the handle works afterwards."""
    c = WC.make_case('base')
    B, z, Ve, Vw, Nw = c['B'], c['z'], c['Ve'], c['Vw'], c['Nw']
    p = U.make_ll_problem(1, 16, c['n'], Vw, Ve, c['dw'], 'int')
    ll = U.ll_engine(p, 8, c['n'], 0.01)
    with pytest.raises(C.SertError, match='loglinear'):
        C.WordFoldIn(ll, c['Nv0'], B, z, 0.01)
    ll.close()
    fs = C.Engine(kind=C.KIND_VECTORSPACE_SOFTMAX, batch_size=8, global_batch_size=8, window_size=c['n'], vocab_size=Vw,
                  num_entities=Ve, word_dim=c['dw'], entity_dim=c['de'], num_negatives=0, id_bytes=4, device=0, keep_grads=0,
                  deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
    with pytest.raises(C.SertError, match='SOFTMAX'):
        C.WordFoldIn(fs, c['Nv0'], B, z, 0.01)
    fs.close()
    dp = _engine(c)
    dp.comm_init(C.comm_unique_id(), 0, 1)
    with pytest.raises(C.SertError, match='communicator'):
        C.WordFoldIn(dp, c['Nv0'], B, z, 0.01)
    dp.close()
    # (d_e > 512: sert_create itself refuses such a model, so no model can carry it to sert_wfold_create's own check)
    with pytest.raises(C.SertError, match=r'entity_dim must be in \[1, 512\]'):
        _engine(dict(c, de=516, Re=np.zeros((Ve, 516), np.float32), W=np.zeros((c['dw'], 516), np.float32), b=np.zeros(516, np.float32)))
    eng = _engine(c)
    try:
        with pytest.raises(C.SertError, match='at least one new word'):
            C.WordFoldIn(eng, np.zeros((0, c['dw']), np.float32), B, z, 0.01)
        with pytest.raises(C.SertError, match='num_negatives >= 1'):
            C.WordFoldIn(eng, c['Nv0'], B, 0, 0.01)
        with pytest.raises(C.SertError, match='batch_size >= 1'):
            C.WordFoldIn(eng, c['Nv0'], 0, z, 0.01)
        with pytest.raises(C.SertError, match='lambda'):
            C.WordFoldIn(eng, c['Nv0'], B, z, -1.0)
        with pytest.raises(C.SertError, match=r'2\^30'):
            C.WordFoldIn(eng, c['Nv0'], 1 << 28, 4, 0.01)
        # (the int32 entry offsets of the index: B n <= 2^31 - 1.  B (1 + z) = 2^30 passes the check before it)
        wide_window = _engine(dict(c, n=5))
        try:
            with pytest.raises(C.SertError, match=r'batch_size \* window_size > 2\^31 - 1'):
                C.WordFoldIn(wide_window, c['Nv0'], 1 << 29, 1, 0.01)
        finally:
            wide_window.close()
        # (V_w + Nw > 2^31 - 1 and M > 2^31 - 1 need arrays no test can hold: the count is checked before the arrays are read)
        import ctypes
        cfg = C.SertWFoldConfig()
        cfg.struct_size = ctypes.sizeof(cfg)
        cfg.batch_size, cfg.num_negatives, cfg.lambda_ = B, z, 0.01
        h = ctypes.c_void_p()
        one = np.zeros(4, np.float32)
        assert hip_lib.sert_wfold_create(eng._h, 2 ** 31 - 1 - Vw + 1, one.ctypes.data, ctypes.byref(cfg), ctypes.byref(h)) != 0
        assert b'2^31 - 1 rows' in hip_lib.sert_last_error() and not h.value
        cfg.struct_size -= 4
        assert hip_lib.sert_wfold_create(eng._h, 1, one.ctypes.data, ctypes.byref(cfg), ctypes.byref(h)) != 0
        assert b'size mismatch' in hip_lib.sert_last_error()
        f = _wfold(c, eng, upload=False)
        assert hip_lib.sert_wfold_upload(f._h, one.ctypes.data, one.ctypes.data, None, 2 ** 31) != 0
        assert b'2^31 - 1 fold-in instances' in hip_lib.sert_last_error()
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.train_batch(0)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.eval_batch(0)
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
        for bad in (-1, Ve):
            neg = c['neg'][0].copy()
            neg[5, 2] = bad
            with pytest.raises(C.SertError, match='negative sample out of range'):
                f.train_batch(0, neg)
            with pytest.raises(C.SertError, match='negative sample out of range'):
                f.eval_batch(0, neg)
        for bad in (-1, c['batches']):               # (the trailing M mod B instances are no batch)
            with pytest.raises(C.SertError, match='batch index out of range'):
                f.train_batch(bad)
            with pytest.raises(C.SertError, match='batch index out of range'):
                f.eval_batch(bad)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batches([0, c['batches']])
        with pytest.raises(C.SertError, match='element count'):
            f.set_rows(C.WFOLD_M, np.zeros(3, np.float32))
        # nothing above moved the handle: it trains as a fresh one does
        assert f.get_step() == 0 and f.get_eval_draws() == 0 and U.same_bits(f.get_rows(), c['Nv0'])
        tw = WC.WordFoldInTwin(c)
        got, ref = f.train_batch(0, c['neg'][0]), tw.train_step(0, c['neg'][0])
        assert abs(got - ref) <= 1e-5 * abs(ref)
        f.close()
    finally:
        eng.close()


def test_python_word_foldin_tracks_the_twin(hip_lib):
    """sert_amd.foldin.WordFoldIn on host arrays: two epochs with a host sampler whose negatives are replayed into the twin;
    the new rows track it within the tensor tolerances, the extended table is the trained rows bit for bit with the new rows
    behind, the optimiser and sampler state round-trip into a second object that continues with the same bits."""
    from sert_amd import foldin
    c = WC.make_case('base')
    rng = np.random.RandomState(5)
    trace = []

    def sampler(batch_index):
        neg = rng.randint(0, c['Ve'], (c['B'], c['z'])).astype(np.int64)
        trace.append((batch_index, neg))
        return neg

    def make():
        return foldin.WordFoldIn(c['Rw'], c['Re'], c['W'], c['b'], c['Nv0'], (c['X'], c['y'], c['w']), batch_size=c['B'],
                                 num_negative_samples=c['z'], regularization_lambda=c['lam'], window_size=c['n'], seed=1, lr=c['lr'])

    np.random.seed(7)           # (the order of the batches inside an epoch)
    fold = make()
    fold.negative_sampler = sampler
    fold.eval_negative_sampler = lambda i: c['eval_neg']
    first, _ = fold.train_error()
    for _ in range(2):
        num_batches, loss = fold.train()
        assert num_batches == c['batches'] and np.isfinite(loss)
    assert len(trace) == 2 * c['batches'] and np.isfinite(first)
    t32, t64 = WC.WordFoldInTwin(c), WC.WordFoldInTwin(c, np.float64)
    for batch_index, neg in trace:
        t32.train_step(batch_index, neg)
        t64.train_step(batch_index, neg)
    Nv = fold.get_new_word_representations()
    print(U.check_tensor('new word rows after %d steps' % len(trace), Nv, t32.Nv, t64.Nv))
    ext = fold.get_extended_word_representations(c['Rw'])
    assert ext.shape == (c['Vw'] + c['Nw'], c['dw']) and U.same_bits(ext[:c['Vw']], c['Rw']) and U.same_bits(ext[c['Vw']:], Nv)
    st, sm = fold.get_optimizer_state(), fold.get_sampler_state()
    assert st['step'] == len(trace) and sm == {'seed': 1, 'eval_draws': 0}
    other = make()
    other._foldin.set_rows(C.WFOLD_ROWS, Nv)
    other.set_optimizer_state(st)
    other.set_sampler_state(sm)
    with pytest.raises(RuntimeError, match='seed is fixed'):
        other.set_sampler_state({'seed': 2, 'eval_draws': 0})
    assert U.same_bits(np.float32(fold._foldin.train_batch(1)), np.float32(other._foldin.train_batch(1)))
    assert U.same_bits(fold.get_new_word_representations(), other.get_new_word_representations())
    with pytest.raises(RuntimeError, match='nothing says how many words are new'):
        foldin.WordFoldIn(c['Rw'], c['Re'], c['W'], c['b'], None, (np.zeros((4, c['n']), np.int32), np.zeros(4, np.int32)),
                          batch_size=2, num_negative_samples=2, regularization_lambda=0.0, window_size=c['n'])
    fold.close()
    other.close()


def test_python_word_foldin_from_a_live_model(hip_lib):
    """sert_amd.foldin.WordFoldIn.from_model: the parameters of a live models.VectorSpaceLanguageModel are copied on the device
    as they are at that moment.  Three steps on explicit negatives track the twin, hold the bits of a fold-in built from the
    same parameters as host arrays, and training the model on or dropping it afterwards changes nothing the handle computes."""
    from sert_amd import foldin, models
    c = WC.make_case('base')
    B, Vw = c['B'], c['Vw']
    trained = (np.minimum(c['X'], Vw - 1), c['y'], c['w'])          # the model's own instances: trained words only
    model = models.VectorSpaceLanguageModel(
        batch_size=B, window_size=c['n'], num_negative_samples=c['z'], representations_init=c['Rw'],
        entity_representations_init=c['Re'], regularization_lambda=0.01, training_set=trained,
        validation_set=(trained[0][:B], trained[1][:B]))
    model.set_dense(c['W'], c['b'])
    with pytest.raises(RuntimeError, match='needs a VectorSpaceLanguageModel'):
        foldin.WordFoldIn.from_model(object(), c['Nv0'], (c['X'], c['y'], c['w']), B, c['z'], c['lam'])
    kw = dict(batch_size=B, num_negative_samples=c['z'], regularization_lambda=c['lam'], seed=1, lr=c['lr'])
    live = foldin.WordFoldIn.from_model(model, c['Nv0'], (c['X'], c['y'], c['w']), **kw)
    host = foldin.WordFoldIn(c['Rw'], c['Re'], c['W'], c['b'], c['Nv0'], (c['X'], c['y'], c['w']), window_size=c['n'], **kw)
    assert live.num_new_words == c['Nw'] and live.vocab_size == Vw and live.window_size == c['n']
    t32, t64 = WC.WordFoldInTwin(c), WC.WordFoldInTwin(c, np.float64)
    for s in range(WC.STEPS):
        if s == 1:
            model.train()                   # the model moves on: the handle holds its own copy
        if s == 2:
            model._engine.close()           # ... and is dropped
        got, same = live._foldin.train_batch(s, c['neg'][s]), host._foldin.train_batch(s, c['neg'][s])
        ref = t32.train_step(s, c['neg'][s])
        t64.train_step(s, c['neg'][s])
        assert U.same_bits(np.float32(got), np.float32(same)) and abs(got - ref) <= 1e-5 * abs(ref), (s, got, same, ref)
    _check_against_twins(live._foldin, t32, t64, 'from_model after %d steps' % WC.STEPS)
    for a, b in zip(_state(live._foldin), _state(host._foldin)):
        assert U.same_bits(a, b)
    ext = live.get_extended_word_representations(c['Rw'])
    assert U.same_bits(ext[:Vw], c['Rw']) and U.same_bits(ext[Vw:], live.get_new_word_representations())
    live.close()
    host.close()
