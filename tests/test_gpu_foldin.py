"""GPU: folding unseen entities into a trained vectorspace model (include/sert_hip_foldin.h, csrc/kernels_foldin.h) against
its oracle twin (tests/foldin_cases.py: VectorSpaceOracle / Adam on the extended table).  Loss 1e-5 relative; the new rows
and Adam's moments through tests.util.check_tensor, against the float32 twin and the float64 one."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import foldin_cases as FC
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the fold-in has its own


def _engine(c, seed=99):
    e = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=_MODEL_B, global_batch_size=_MODEL_B, window_size=c['n'],
                 vocab_size=c['Vw'], num_entities=c['Ve'], word_dim=c['dw'], entity_dim=c['de'], num_negatives=2, id_bytes=4,
                 device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=seed)
    for which, key in ((C.T_RW, 'Rw'), (C.T_RE, 'Re'), (C.T_W, 'W'), (C.T_B, 'b')):
        e.set_tensor(which, c[key])
    return e


def _foldin(c, eng, seed=FC.SEED, upload=True):
    f = C.FoldIn(eng, c['E0'], c['B'], c['z'], c['lam'], lr=c['lr'], seed=seed)
    if upload:
        f.upload(c['X'], c['y'], c['w'])
    return f


def _state(f):
    return f.get_rows(C.FOLDIN_ROWS), f.get_rows(C.FOLDIN_M), f.get_rows(C.FOLDIN_V)


def _check_against_twins(f, t32, t64, label):
    E, m, v = _state(f)
    log = [U.check_tensor(label + ' E', E, t32.E, t64.E),
           U.check_tensor(label + ' m', m, t32.m, t64.m),
           # (a second moment: twice the row-wise bound, as tests.util.check_state)
           U.check_tensor(label + ' v', v, t32.v, t64.v, row_tol32=2 * U.ROW_TOL32, row_tol64=2 * U.ROW_TOL64)]
    print('\n'.join(log))


@pytest.fixture(scope='module', params=sorted(FC.CASES))
def case(request):
    return FC.make_case(request.param)


def test_parity_explicit_and_replayed_negatives(hip_lib, case):
    """Every case for three steps: the loss of each step, then E, m and v -- with explicit negatives, and with
    device-drawn negatives replayed into the twin through sert_foldin_negatives_of_step."""
    c = case
    eng = _engine(c)
    try:
        for drawn in (False, True):
            f = _foldin(c, eng)
            assert f.num_batches() == c['batches']
            t32, t64 = FC.FoldInTwin(c), FC.FoldInTwin(c, np.float64)
            for s in range(FC.STEPS):
                assert f.get_step() == s
                if drawn:
                    neg = f.negatives_of_step(s)
                    assert neg.shape == (c['B'], c['z']) and neg.min() >= 0 and neg.max() < c['Ve'] + c['N']
                    got = f.train_batch(s)
                else:
                    neg = c['neg'][s]
                    got = f.train_batch(s, neg)
                ref = t32.train_step(s, neg)
                t64.train_step(s, neg)
                print('%s %s step %d: loss %.7f oracle %.7f' % (c['name'], 'drawn' if drawn else 'explicit', s, got, ref))
                assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], drawn, s, got, ref)
            assert f.get_step() == FC.STEPS
            _check_against_twins(f, t32, t64, '%s %s' % (c['name'], 'drawn' if drawn else 'explicit'))
            f.close()
    finally:
        eng.close()


def test_evaluation_loss_changes_nothing(hip_lib, case):
    """eval_batch = the twin's eval_loss on the extended table (unweighted, unregularised), after one training step so that
    E differs from E0; no state changes, bit for bit."""
    c = case
    eng = _engine(c)
    f = _foldin(c, eng)
    try:
        tw = FC.FoldInTwin(c)
        f.train_batch(0, c['neg'][0])
        tw.train_step(0, c['neg'][0])
        before = _state(f)
        tw.E[...] = before[0]               # (evaluate the twin ON the device's rows: this test is about the loss)
        got = f.eval_batch(1, c['eval_neg'])
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
    c = FC.make_case('base')
    results = []
    for disturb in (False, True):
        eng = _engine(c)
        before = [eng.get_tensor(t).copy() for t in (C.T_RW, C.T_RE, C.T_W, C.T_B)]
        f = _foldin(c, eng)
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


def test_reproducible_and_train_batches(hip_lib):
    """Two handles with one seed hold the same bits after five steps, and train_batches (one synchronisation) gives the bits
    of the train_batch loop; another seed draws other negatives."""
    c = FC.make_case('base')
    eng = _engine(c)
    order = [0, 2, 1, 1, 0]
    try:
        a, b, d = _foldin(c, eng), _foldin(c, eng), _foldin(c, eng, seed=FC.SEED + 1)
        la = np.asarray([a.train_batch(i) for i in order], np.float32)
        lb = b.train_batches(order)
        assert U.same_bits(la, lb) and a.get_step() == b.get_step() == 5
        for x, y in zip(_state(a), _state(b)):
            assert U.same_bits(x, y)
        assert not np.array_equal(a.negatives_of_step(0), d.negatives_of_step(0))
        assert np.array_equal(a.negatives_of_step(3), b.negatives_of_step(3))
        # the optimiser state round-trips: a third handle set to a's state continues with a's bits
        d2 = _foldin(c, eng)
        for which, val in zip((C.FOLDIN_ROWS, C.FOLDIN_M, C.FOLDIN_V), _state(a)):
            d2.set_rows(which, val)
        d2.set_step(5)
        assert U.same_bits(np.float32(a.train_batch(1)), np.float32(d2.train_batch(1)))
        assert U.same_bits(_state(a)[0], _state(d2)[0])
        for h in (a, b, d, d2):
            h.close()
    finally:
        eng.close()


def test_refusals(hip_lib):
    """Everything the contract puts out of scope comes back nonzero with a message -- validated on the host, nothing is
    launched on bad ids -- and the handle works afterwards."""
    c = FC.make_case('base')
    B, z, Ve, N = c['B'], c['z'], c['Ve'], c['N']
    # a loglinear model, the full-softmax kind, a model with a communicator
    p = U.make_ll_problem(1, 16, c['n'], c['Vw'], c['Ve'], c['dw'], 'int')
    ll = U.ll_engine(p, 8, c['n'], 0.01)
    with pytest.raises(C.SertError, match='loglinear'):
        C.FoldIn(ll, np.zeros((N, 0), np.float32), B, z, 0.01)          # (a loglinear model has entity_dim 0)
    ll.close()
    fs = C.Engine(kind=C.KIND_VECTORSPACE_SOFTMAX, batch_size=8, global_batch_size=8, window_size=c['n'], vocab_size=c['Vw'],
                  num_entities=Ve, word_dim=c['dw'], entity_dim=c['de'], num_negatives=0, id_bytes=4, device=0, keep_grads=0,
                  deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
    with pytest.raises(C.SertError, match='SOFTMAX'):
        C.FoldIn(fs, c['E0'], B, z, 0.01)
    fs.close()
    dp = _engine(c)
    dp.comm_init(C.comm_unique_id(), 0, 1)
    with pytest.raises(C.SertError, match='communicator'):
        C.FoldIn(dp, c['E0'], B, z, 0.01)
    dp.close()
    eng = _engine(c)
    try:
        with pytest.raises(C.SertError, match='at least one new entity'):
            C.FoldIn(eng, np.zeros((0, c['de']), np.float32), B, z, 0.01)
        with pytest.raises(C.SertError, match='num_negatives >= 1'):
            C.FoldIn(eng, c['E0'], B, 0, 0.01)
        f = _foldin(c, eng, upload=False)
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.train_batch(0)
        for bad in (-1, N):
            y = c['y'].copy()
            y[7] = bad
            with pytest.raises(C.SertError, match=r'label out of range'):
                f.upload(c['X'], y, c['w'])
        X = c['X'].copy()
        X[3, 1] = c['Vw']
        with pytest.raises(C.SertError, match='token id out of range'):
            f.upload(X, c['y'], c['w'])
        f.upload(c['X'], c['y'], c['w'])
        for bad in (-1, Ve + N):
            neg = c['neg'][0].copy()
            neg[5, 2] = bad
            with pytest.raises(C.SertError, match='negative sample out of range'):
                f.train_batch(0, neg)
            with pytest.raises(C.SertError, match='negative sample out of range'):
                f.eval_batch(0, neg)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batch(c['batches'])               # (the trailing M mod B instances are no batch)
        with pytest.raises(C.SertError, match='batch index out of range'):
            f.train_batches([0, c['batches']])
        with pytest.raises(C.SertError, match='element count'):
            f.set_rows(C.FOLDIN_M, np.zeros(3, np.float32))
        # nothing above moved the handle: it trains as a fresh one does
        assert f.get_step() == 0 and f.get_eval_draws() == 0 and U.same_bits(f.get_rows(), c['E0'])
        tw = FC.FoldInTwin(c)
        got, ref = f.train_batch(0, c['neg'][0]), tw.train_step(0, c['neg'][0])
        assert abs(got - ref) <= 1e-5 * abs(ref)
        f.close()
    finally:
        eng.close()


def test_end_to_end_entity_foldin_and_scorer(hip_lib):
    """20 trained + 6 new entities with 10 characteristic words each (V_w = 240, d_w = 16, d_e = 8, n = 4, z = 4, B = 32,
    lambda = lr = 0.01): the base is trained for 8 epochs on 64 instances per entity, the new entities are folded in through
    sert_amd.foldin.EntityFoldIn for 10 epochs on 32 instances each.  On the CPU oracle this construction took the mean
    evaluation loss over fixed evaluation negatives from about 1.65 to about 1.44 in every seed tried.  Asserted: the
    evaluation loss after the last epoch is below the one before the first; the new rows track the twin within the tensor
    tolerances; the Scorer over the extended table returns new-entity indices in range.  The mean reciprocal rank of the new
    entities is logged only (0.3 .. 0.8 on the oracle)."""
    from sert_amd import foldin
    rng = np.random.RandomState(0)
    Vw, Ve, N, dw, de, n, z, B = 240, 20, 6, 16, 8, 4, 4, 32
    words = [rng.choice(Vw, 10, replace=False) for _ in range(Ve + N)]

    def data(ents, per):
        y = np.repeat(ents, per)
        X = np.stack([rng.choice(words[e], n) for e in y])
        p = rng.permutation(len(y))
        return X[p].astype(np.int32), y[p].astype(np.int32)

    Xb, yb = data(np.arange(Ve), 64)
    base = dict(Rw=U.O.glorot_uniform(rng, (Vw, dw)), Re=U.O.glorot_uniform(rng, (Ve, de)), W=U.O.glorot_uniform(rng, (dw, de)),
                b=np.zeros(de, np.float32), X=Xb.astype(np.uint32))
    eng = U.vs_engine(base, B, n, z, 0.01, keep_grads=0, lr=0.01)
    eng.upload_dataset(C.SPLIT_TRAIN, base['X'], y_int=yb, w=np.ones(len(yb), np.float32))
    for _ in range(8):
        for i in range(len(yb) // B):
            eng.train_batch(i, rng.randint(0, Ve, (B, z)).astype(np.int64))
    Rw, Re = eng.get_tensor(C.T_RW, (Vw, dw)).copy(), eng.get_tensor(C.T_RE, (Ve, de)).copy()
    W, b = eng.get_tensor(C.T_W, (dw, de)).copy(), eng.get_tensor(C.T_B, (de,)).copy()
    eng.close()

    Xn, yn = data(np.arange(Ve, Ve + N), 32)
    yn = yn - Ve
    E0 = U.O.glorot_uniform(rng, (N, de))
    nb = len(yn) // B
    evneg = [rng.randint(0, Ve + N, (B, z)).astype(np.int64) for _ in range(nb)]
    trace = []

    def sampler(batch_index):
        neg = rng.randint(0, Ve + N, (B, z)).astype(np.int64)
        trace.append((batch_index, neg))
        return neg

    np.random.seed(7)           # (the order of the batches inside an epoch)
    fold = foldin.EntityFoldIn(Rw, Re, W, b, E0, (Xn, yn, np.ones(len(yn), np.float32)), batch_size=B, num_negative_samples=z,
                               regularization_lambda=0.01, window_size=n, seed=1, lr=0.01)
    fold.negative_sampler = sampler
    fold.eval_negative_sampler = lambda i: evneg[i]
    first, _ = fold.train_error()
    for _ in range(10):
        num_batches, _ = fold.train()
        assert num_batches == nb
    last, _ = fold.train_error()
    print('evaluation loss %.4f -> %.4f' % (first, last))
    assert last < first
    assert len(trace) == 10 * nb
    st = fold.get_optimizer_state()
    assert st['step'] == 10 * nb and fold.get_sampler_state()['seed'] == 1
    # the twin, on the same batches and negatives
    c = dict(Rw=Rw, Re=Re, W=W, b=b, E0=E0, X=Xn, y=yn, w=np.ones(len(yn), np.float32), B=B, n=n, z=z, Ve=Ve, N=N, dw=dw, de=de,
             lam=0.01, lr=0.01)
    t32, t64 = FC.FoldInTwin(c), FC.FoldInTwin(c, np.float64)
    for batch_index, neg in trace:
        t32.train_step(batch_index, neg)
        t64.train_step(batch_index, neg)
    E = fold.get_new_representations()
    print(U.check_tensor('new rows after %d steps' % len(trace), E, t32.E, t64.E))
    ext = fold.get_extended_representations(Re)
    assert ext.shape == (Ve + N, de) and U.same_bits(ext[:Ve], Re) and U.same_bits(ext[Ve:], E)
    fold.close()
    # the scorer serves the extended table unchanged: query = the mean word vector of an entity's characteristic words
    hv = np.stack([Rw[words[e]].mean(axis=0) for e in range(Ve, Ve + N)])
    proj = np.tanh(hv @ W + b).astype(np.float32)
    sc = C.Scorer(ext)
    idx, _ = sc.topk(proj, Ve + N)
    idx = np.array(idx)
    sc.close()
    assert idx.min() >= 0 and idx.max() == Ve + N - 1 and all(sorted(r) == list(range(Ve + N)) for r in idx.tolist())
    rr = [1.0 / (1 + int(np.nonzero(idx[q] == Ve + q)[0][0])) for q in range(N)]
    print('mean reciprocal rank of the new entities: %.3f' % float(np.mean(rr)))
