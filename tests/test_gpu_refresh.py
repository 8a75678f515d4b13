"""-m gpu: refreshing trained entity rows in a fold-in (sert_foldin_create_refresh, include/sert_hip_foldin.h; the loss kernels
foldin_nce_map* of csrc/kernels_foldin.h) against the oracle twin of tests/refresh_cases.py.  The bounds are those of
tests/test_gpu_foldin_keys.py: each loss within 1e-5 of the float32 twin; every row against its own norm through
tests.util.check_tensor (ROW_TOL32 against the float32 twin, ROW_TOL64 against the float64 one, twice either for a second
moment).  From zero moments m = (1 - beta1) g, so the moments after step 1 are the gradient itself; then E, m and v after
step 2.  tests/test_refresh_inputs_cpu.py proves the inputs and that the row bound tells slot order from id order."""
import ctypes

import numpy as np
import pytest

from sert_amd import _capi as C
from tests import foldin_cases as FC
from tests import refresh_cases as RC
from tests import util as U

pytestmark = pytest.mark.gpu

_MODEL_B = 8          # the MODEL's batch size: the handle has its own
_NO_PLAN = dict(loss='none', k=0, train=False, sort_bits=0, passes=0, vec=0, nch=0, col_passes=0, fixup='none', tiles=0)
_CHECKED = {0: ('m', 'v'), 1: ('E', 'm', 'v')}        # as tests/test_gpu_foldin_keys.py


def _engine(c):
    e = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=_MODEL_B, global_batch_size=_MODEL_B, window_size=c['n'],
                 vocab_size=c['Vw'], num_entities=c['Ve'], word_dim=c['dw'], entity_dim=c['de'], num_negatives=2, id_bytes=4,
                 device=0, keep_grads=0, deterministic=1, lambda_=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=99)
    for which, key in ((C.T_RW, 'Rw'), (C.T_RE, 'Re'), (C.T_W, 'W'), (C.T_B, 'b')):
        e.set_tensor(which, c[key])
    return e


def _refresh(c, eng, lam=None, seed=RC.SEED):
    f = C.FoldIn(eng, c['New0'], c['B'], c['z'], c['lam'] if lam is None else lam, lr=c['lr'], seed=seed,
                 refresh_ids=c['refresh'])
    assert f.table() == c['table'] and f.plan() == _NO_PLAN, (c['name'], 'before the first step')
    # the slots start from the model's rows, in the order of refresh, and from the new rows given
    assert U.same_bits(f.get_rows(C.FOLDIN_ROWS), c['E0'])
    f.upload(c['X'], c['y'], c['w_upload'])
    return f


def _state(f):
    return dict(E=f.get_rows(C.FOLDIN_ROWS), m=f.get_rows(C.FOLDIN_M), v=f.get_rows(C.FOLDIN_V))


def _check(label, got, r32, r64, keys):
    for key in keys:
        mult = 2 if key == 'v' else 1       # (a second moment: twice the row-wise bound, as tests/test_gpu_foldin_keys.py)
        print(U.check_tensor('%s %s' % (label, key), got[key], r32[key], r64[key], row_tol32=mult * U.ROW_TOL32,
                             row_tol64=mult * U.ROW_TOL64))


def _two_steps(c, f, refs=None):
    """Both steps on the case's explicit negatives; table() and plan() after each; with refs = (float32 run, float64 run) each
    loss against the float32 twin and the state behind it, every row, against both."""
    losses, states = [], []
    for s in range(RC.STEPS):
        got = f.train_batch(s, c['neg'][s])
        assert f.plan() == c['plan'], (c['name'], 'step', s, 'launched', f.plan(), 'the case is there for', c['plan'])
        assert f.table() == c['table']
        losses.append(got)
        states.append(_state(f))
        if refs is not None:
            ref = refs[0][s]['loss']
            print('%s step %d: loss %.7f twin %.7f' % (c['name'], s, got, ref))
            assert abs(got - ref) <= 1e-5 * abs(ref), (c['name'], s, got, ref)
            _check('%s step %d' % (c['name'], s), states[s], refs[0][s], refs[1][s], _CHECKED[s])
    return np.asarray(losses, np.float32), states


@pytest.mark.parametrize('name', list(RC.CASES))
def test_refresh_step_in_every_case(hip_lib, name):
    """Per case: table() and plan(); each loss; the gradient after step 1; E, m and v after step 2; then an evaluation against
    the twin's eval_loss on the device's rows, which changes no state."""
    c = RC.make_case(name)
    refs = RC.case_reference(name, np.float32), RC.case_reference(name, np.float64)
    eng = _engine(c)
    f = _refresh(c, eng)
    try:
        assert f.num_batches() == RC.STEPS
        _, states = _two_steps(c, f, refs)
        tw = RC.RefreshTwin(c, E0=states[1]['E'])           # (evaluate the twin ON the device's rows)
        got, ref = f.eval_batch(1, c['eval_neg']), tw.eval_loss(1, c['eval_neg'])
        print('%s evaluation: loss %.7f twin %.7f' % (name, got, ref))
        assert abs(got - ref) <= 1e-5 * abs(ref), (name, got, ref)
        assert f.plan() == dict(c['plan'], train=False), (name, 'after an evaluation', f.plan())
        after = _state(f)
        assert all(U.same_bits(after[k], states[1][k]) for k in after) and f.get_step() == RC.STEPS
    finally:
        f.close()
        eng.close()


def test_device_negatives_replayed_into_the_twin(hip_lib):
    """Negatives drawn on the device over V_e + num_new ids, read back through negatives_of_step, then the twin on them."""
    c = RC.make_case(RC.DEVICE_NEGATIVES_CASE)
    eng = _engine(c)
    f = _refresh(c, eng)
    try:
        t32, t64 = RC.RefreshTwin(c), RC.RefreshTwin(c, np.float64)
        seen = []
        for s in range(RC.STEPS):
            neg = f.negatives_of_step(s)
            assert neg.shape == (c['B'], c['z']) and neg.min() >= 0 and neg.max() < c['Ve'] + c['num_new']
            seen.append(neg)
            got = f.train_batch(s)
            ref = t32.train_step(s, neg)
            t64.train_step(s, neg)
            assert abs(got - ref) <= 1e-5 * abs(ref), (s, got, ref)
        allneg = np.concatenate(seen).ravel()
        assert np.isin(allneg, c['refresh']).any() and (allneg >= c['Ve']).any()      # the draws reach both kinds of slot
        _check('drawn', _state(f), dict(E=t32.E, m=t32.m, v=t32.v), dict(E=t64.E, m=t64.m, v=t64.v), ('E', 'm', 'v'))
        drawn = f.negatives_of_step(0, evaluation=True)
        got = f.eval_batch(0)
        tw = RC.RefreshTwin(c, E0=f.get_rows())
        ref = tw.eval_loss(0, drawn)
        assert abs(got - ref) <= 1e-5 * abs(ref) and f.get_eval_draws() == 1 and f.get_step() == RC.STEPS
    finally:
        f.close()
        eng.close()


def test_unhit_slots_keep_their_bits_at_lambda_zero(hip_lib):
    """lambda = 0: a slot no pair of either step hit keeps the bits of its initial row and has bit-zero moments."""
    name = RC.LAMBDA0_CASE
    c = RC.make_case(name)
    refs = RC.case_reference(name, np.float32, lam=0.0), RC.case_reference(name, np.float64, lam=0.0)
    eng = _engine(c)
    f = _refresh(c, eng, lam=0.0)
    try:
        _, states = _two_steps(c, f, refs)
        hit = np.zeros(c['Nt'], bool)
        for s in range(RC.STEPS):
            keys = RC.slot_keys(c, s)
            hit[np.unique(keys[keys < c['Nt']])] = True
        absent = np.nonzero(~hit)[0]
        assert len(absent) >= 6 and hit.sum() >= 3
        E, m, v = (states[1][k] for k in ('E', 'm', 'v'))
        zero = np.zeros((len(absent), c['de']), np.float32)
        assert U.same_bits(E[absent], c['E0'][absent]) and U.same_bits(m[absent], zero) and U.same_bits(v[absent], zero)
        assert np.all(np.abs(m[hit]).max(axis=1) > 0)
    finally:
        f.close()
        eng.close()


def test_no_refreshed_row_is_the_fold_in_bit_for_bit(hip_lib):
    """create_refresh(num_refresh = 0, num_new = N) against sert_foldin_create(N) on the same inputs and seed, two
    train_batches steps with device-drawn negatives: the same bits in the losses, E, m and v -- through the other loss
    kernel (map form 1 against 0)."""
    for name in ('base', 'odd_de'):                  # (the vector and the scalar kernel)
        c = FC.make_case(name)
        eng = _engine(c)
        try:
            a = C.FoldIn(eng, c['E0'], c['B'], c['z'], c['lam'], lr=c['lr'], seed=FC.SEED, refresh_ids=np.zeros(0, np.int32))
            b = C.FoldIn(eng, c['E0'], c['B'], c['z'], c['lam'], lr=c['lr'], seed=FC.SEED)
            assert a.table() == dict(map=True, num_refresh=0, num_new=c['N'], rows=c['N'])
            assert b.table() == dict(map=False, num_refresh=0, num_new=c['N'], rows=c['N'])
            for h in (a, b):
                h.upload(c['X'], c['y'], c['w'])
            la, lb = a.train_batches([0, 1]), b.train_batches([0, 1])
            assert U.same_bits(la, lb) and a.plan() == b.plan() and a.plan()['train']
            assert np.array_equal(a.negatives_of_step(1), b.negatives_of_step(1))
            sa, sb = _state(a), _state(b)
            assert all(U.same_bits(sa[k], sb[k]) for k in sa) and not U.same_bits(sa['E'], c['E0'])
            a.close()
            b.close()
        finally:
            eng.close()


def test_frozen_rows_and_the_model_are_never_written(hip_lib):
    """After the steps the model's R_w, W, b, R_e hold the bits they had; EntityFoldIn.get_extended_representations differs
    from R_e exactly on the refreshed rows and does not modify the caller's array."""
    from sert_amd import foldin
    c = RC.make_case('mixed')
    eng = _engine(c)
    before = [eng.get_tensor(t).copy() for t in (C.T_RW, C.T_RE, C.T_W, C.T_B)]
    f = _refresh(c, eng)
    try:
        _two_steps(c, f)
        for a, b in zip(before, [eng.get_tensor(t) for t in (C.T_RW, C.T_RE, C.T_W, C.T_B)]):
            assert U.same_bits(a, b)
    finally:
        f.close()
        eng.close()
    fold = foldin.EntityFoldIn(c['Rw'], c['Re'], c['W'], c['b'], c['New0'], (c['X'], c['y'], c['w']), batch_size=c['B'],
                               num_negative_samples=c['z'], regularization_lambda=c['lam'], window_size=c['n'], seed=RC.SEED,
                               lr=c['lr'], refresh=c['refresh'])
    try:
        fold.negative_sampler = lambda i: c['neg'][i]
        for s in range(RC.STEPS):
            fold.train_fn(s)
        Re = c['Re'].copy()
        ext = fold.get_extended_representations(Re)
        assert np.array_equal(Re, c['Re']) and ext.shape == (c['Ve'] + c['num_new'], c['de'])
        changed = np.nonzero((ext[:c['Ve']] != Re).any(axis=1))[0]
        assert sorted(changed.tolist()) == sorted(c['refresh'].tolist())
        frozen = np.setdiff1d(np.arange(c['Ve']), c['refresh'])
        assert U.same_bits(ext[frozen], Re[frozen])
        assert U.same_bits(ext[c['refresh']], fold.get_refreshed_representations())
        assert U.same_bits(ext[c['Ve']:], fold.get_new_representations())
        # the state is in slot order: the rows of the reference after step 2
        st = fold.get_optimizer_state()
        r32, r64 = RC.case_reference('mixed', np.float32)[1], RC.case_reference('mixed', np.float64)[1]
        assert st['step'] == RC.STEPS and st['m_E'].shape == (c['Nt'], c['de'])
        print(U.check_tensor('EntityFoldIn m', st['m_E'], r32['m'], r64['m']))
        print(U.check_tensor('EntityFoldIn E', ext[c['ext_of_slot']], r32['E'], r64['E']))
    finally:
        fold.close()


def test_two_handles_with_one_seed_hold_the_same_bits(hip_lib):
    c = RC.make_case('wave_fixup')
    eng = _engine(c)
    try:
        runs = []
        for _ in range(2):
            f = _refresh(c, eng)
            losses = f.train_batches([0, 1, 0])
            runs.append([losses] + list(_state(f).values()))
            f.close()
        for a, b in zip(*runs):
            assert U.same_bits(a, b)
    finally:
        eng.close()


def test_refusals(hip_lib):
    """Each comes back as an error with a message, nothing is launched, and the handle works afterwards."""
    c = RC.make_case('mixed')
    B, z, Ve, Nt = c['B'], c['z'], c['Ve'], c['Nt']
    eng = _engine(c)
    try:
        make = lambda ids, rows: C.FoldIn(eng, rows, B, z, 0.01, refresh_ids=np.asarray(ids, np.int32))
        with pytest.raises(C.SertError, match='duplicate refresh id'):
            make([5, 1, 5], c['New0'])
        for bad in (Ve, -1):
            with pytest.raises(C.SertError, match='refresh id out of range'):
                make([5, bad], c['New0'])
        with pytest.raises(C.SertError, match='at least one trainable row'):
            make([], None)
        with pytest.raises(C.SertError, match='num_negatives >= 1'):
            C.FoldIn(eng, c['New0'], B, 0, 0.01, refresh_ids=c['refresh'])
        # a null init_new_rows with num_new = 1, a null refresh_ids with num_refresh = 1, negative counts: the C ABI itself
        lib = C.load()
        cfg = C.SertFoldInConfig()
        cfg.struct_size = ctypes.sizeof(cfg)
        cfg.batch_size, cfg.num_negatives, cfg.lambda_, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps = B, z, 0.01, 0.01, 0.9, 0.999, 1e-8
        ids = np.array([5, 1], np.int32)
        for args, message in (((ids.ctypes.data, 2, 1, None), b'null init_new_rows'),
                              ((None, 1, 0, None), b'null refresh_ids'),
                              ((ids.ctypes.data, -1, 1, c['New0'].ctypes.data), b'num_refresh >= 0'),
                              ((ids.ctypes.data, 2, -1, None), b'num_new >= 0'),
                              ((None, 0, 0, None), b'at least one trainable row')):
            h = ctypes.c_void_p()
            assert lib.sert_foldin_create_refresh(eng._h, *args, ctypes.byref(cfg), ctypes.byref(h)) != 0
            assert message in lib.sert_last_error() and not h.value, (message, lib.sert_last_error())
        f = C.FoldIn(eng, c['New0'], B, z, c['lam'], lr=c['lr'], refresh_ids=c['refresh'])
        for bad in (Nt, -1):
            y = c['y'].copy()
            y[7] = bad
            with pytest.raises(C.SertError, match='label out of range'):
                f.upload(c['X'], y, c['w'])
        with pytest.raises(C.SertError, match='no fold-in instances'):
            f.train_batch(0)
        f.upload(c['X'], c['y'], c['w_upload'])
        for bad in (-1, Ve + c['num_new']):
            neg = c['neg'][0].copy()
            neg[5, 2] = bad
            with pytest.raises(C.SertError, match='negative sample out of range'):
                f.train_batch(0, neg)
        with pytest.raises(C.SertError, match='element count'):
            f.set_rows(C.FOLDIN_M, np.zeros((c['num_new'], c['de']), np.float32))       # (Nt rows, not num_new)
        # nothing above moved the handle
        assert f.get_step() == 0 and U.same_bits(f.get_rows(), c['E0']) and f.plan() == _NO_PLAN
        got, ref = f.train_batch(0, c['neg'][0]), RC.case_reference('mixed', np.float32)[0]['loss']
        assert abs(got - ref) <= 1e-5 * abs(ref)
        f.close()
    finally:
        eng.close()
    p = U.make_ll_problem(1, 16, c['n'], c['Vw'], Ve, c['dw'], 'int')
    ll = U.ll_engine(p, 8, c['n'], 0.01)
    try:
        with pytest.raises(C.SertError, match='loglinear'):
            C.FoldIn(ll, None, B, z, 0.01, refresh_ids=np.array([1], np.int32))
    finally:
        ll.close()


def test_end_to_end_a_refreshed_entity_rises_for_its_new_words(hip_lib):
    """20 trained entities with 10 characteristic words each (the construction of tests/test_gpu_foldin.py).  The entity
    that the query of entity 11's words ranks last gains documents made of those words.  After EntityFoldIn(refresh=[it]) on
    those instances, the Scorer over the extended table ranks it above its position before the refresh for that query;
    every other row of the table is untouched."""
    from sert_amd import foldin
    rng = np.random.RandomState(0)
    Vw, Ve, dw, de, n, z, B = 240, 20, 16, 8, 4, 4, 32
    words = [rng.choice(Vw, 10, replace=False) for _ in range(Ve)]
    y = np.repeat(np.arange(Ve), 64)
    X = np.stack([rng.choice(words[e], n) for e in y])
    p = rng.permutation(len(y))
    Xb, yb = X[p].astype(np.int32), y[p].astype(np.int32)
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

    query_of = 11
    query = np.tanh(Rw[words[query_of]].mean(axis=0) @ W + b).astype(np.float32)[None, :]

    def ranking(table):
        sc = C.Scorer(table)
        idx, _ = sc.topk(query, Ve)
        order = np.array(idx)[0].tolist()        # (a copy: the result is a view of a buffer that close() frees)
        sc.close()
        return order

    entity = ranking(Re)[-1]                     # the trained entity that query ranks LAST
    position = lambda table: ranking(table).index(entity)
    before = position(Re)
    assert before == Ve - 1 and entity != query_of
    Xn = np.stack([rng.choice(words[query_of], n) for _ in range(4 * B)]).astype(np.int32)
    np.random.seed(7)
    fold = foldin.EntityFoldIn(Rw, Re, W, b, None, (Xn, np.zeros(len(Xn), np.int32), None), batch_size=B,
                               num_negative_samples=z, regularization_lambda=0.01, window_size=n, seed=1, lr=0.01,
                               refresh=[entity])
    assert fold.num_new == 0 and fold.num_refresh == 1
    for _ in range(10):
        fold.train()
    ext = fold.get_extended_representations(Re)
    fold.close()
    assert ext.shape == Re.shape
    others = np.arange(Ve) != entity
    assert U.same_bits(ext[others], Re[others]) and not U.same_bits(ext[entity], Re[entity])
    after = position(ext)
    print('entity %d for the query of entity %d: position %d -> %d' % (entity, query_of, before, after))
    assert after < before
