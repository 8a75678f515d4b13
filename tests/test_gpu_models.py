"""-m gpu: the sert.models / sert.inference / bin/*.py surface end to end on the
MI355X, against the oracle and the reference-derived golden vectors."""
import importlib.util
import io
import json
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import sert_oracle as O
from sert_amd import _capi as C
from sert_amd import inference, models, scoring
from tests import util as U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def gold():
    arrays = np.load(os.path.join(HERE, 'golden', 'reference_vectors.npz'))
    with open(os.path.join(HERE, 'golden', 'reference_vectors.json')) as f:
        meta = json.load(f)
    return arrays, meta


def test_vectorspace_model_epoch_matches_oracle(hip_lib):
    """train() over a shuffled epoch + train_error()/validation_error() through
    the class surface, explicit negatives, vs the oracle driven the same way."""
    B, n, z, Vw, Ve, dw, de = 64, 4, 5, 400, 30, 32, 32
    N, Nv = B * 5 + 7, B * 2
    p = U.make_vs_problem(11, N + Nv, n, z, Vw, Ve, dw, de)
    Xt, yt, wt = p['X'][:N], p['y'][:N], p['w'][:N]
    Xv, yv = p['X'][N:], p['y'][N:]
    negs = {('t', j): p['rng'].randint(0, Ve, (B, z)).astype(np.int64) for j in range(5)}
    negs.update({('e', j): p['rng'].randint(0, Ve, (B, z)).astype(np.int64) for j in range(5)})
    np.random.seed(3)
    m = models.VectorSpaceLanguageModel(
        batch_size=B, window_size=n, num_negative_samples=z, representations_init=p['Rw'],
        entity_representations_init=p['Re'], regularization_lambda=0.01,
        training_set=(Xt, yt, wt), validation_set=(Xv, yv))
    m.negative_sampler = lambda j: negs[('t', j)]
    m.eval_negative_sampler = lambda j: negs[('e', j)]
    W0, b0 = m.get_dense_weights(), m.get_dense_bias()
    assert isinstance(m, models.ModelInterface)
    ora = O.VectorSpaceOracle(B, n, z, p['Rw'], p['Re'], W0, b0, 0.01)
    order = list(range(5))
    np.random.seed(99)
    np.random.shuffle(order)
    ref_losses = [ora.train_step(Xt[j*B:(j+1)*B], yt[j*B:(j+1)*B], wt[j*B:(j+1)*B], negs[('t', j)])
                  for j in order]
    np.random.seed(99)
    nb, mean_loss = m.train()
    assert nb == 5
    assert abs(mean_loss - np.mean(ref_losses)) < 1e-5 * abs(np.mean(ref_losses))
    Rw, Re = m.get_representations()
    assert U.rel_err(Rw, ora.R_w) < 1e-4 and U.rel_err(Re, ora.R_e) < 1e-4
    # every parameter (W, b too) and both Adam moments after the epoch
    print('\n'.join(U.check_state(U.engine_state(m._engine), U.oracle_state(ora))))
    te_mean, te_std = m.train_error()
    ref = [ora.eval_loss(Xt[j*B:(j+1)*B], yt[j*B:(j+1)*B], negs[('e', j)]) for j in range(5)]
    assert abs(te_mean - np.mean(ref)) < 1e-5 * abs(np.mean(ref))
    assert abs(te_std - np.std(ref)) < 1e-4 * max(1e-3, abs(np.std(ref)))
    ve_mean, _ = m.validation_error()
    refv = [ora.eval_loss(Xv[j*B:(j+1)*B], yv[j*B:(j+1)*B], negs[('e', j)]) for j in range(2)]
    assert abs(ve_mean - np.mean(refv)) < 1e-5 * abs(np.mean(refv))
    # get_state: [predict_fn, R_w, R_e]; predict_fn pickles and still predicts
    state = m.get_state()
    assert len(state) == 3 and state[1].shape == (Vw, dw) and state[2].shape == (Ve, de)
    fn = pickle.loads(pickle.dumps(state[0]))
    avg = Rw[[1, 2, 3]].mean(axis=0)
    out = fn(avg)
    assert out.shape == (1, de)
    assert U.rel_err(out, ora.predict(avg)[None, :]) < 1e-5
    # optimiser state round trip (additive)
    st = m.get_optimizer_state()
    assert st['step'] == 5 and st['m_R_w'].shape == (Vw, dw)
    m.set_optimizer_state(st)
    assert U.rel_err(st['m_R_w'], ora.opt.m[1]) < 1e-4


def test_loglinear_model_csr_labels(hip_lib):
    B, n, Vw, Ve, d = 32, 3, 200, 20, 16
    p = U.make_ll_problem(4, B * 3, n, Vw, Ve, d, 'csr')
    empty = (np.zeros((0, n), p['X'].dtype), sp.csr_matrix((0, Ve), dtype=np.float32))
    np.random.seed(1)
    m = models.LanguageModel(batch_size=B, window_size=n, representations_init=p['Rw'],
                             output_layer_size=Ve, regularization_lambda=0.01,
                             training_set=(p['X'], p['y'], p['w']), validation_set=empty)
    ora = O.LogLinearOracle(B, n, p['Rw'], m.get_dense_weights(), m.get_dense_bias(), 0.01)
    for j in range(3):
        ref = ora.train_step(p['X'][j*B:(j+1)*B], p['ydense'][j*B:(j+1)*B], p['w'][j*B:(j+1)*B])
        got = m.train_fn(j)
        assert abs(got - ref) <= 1e-5 * abs(ref)
    assert U.rel_err(m.get_representations(), ora.R_w) < 1e-4
    # every parameter and Adadelta's accu / delta
    print('\n'.join(U.check_state(U.engine_state(m._engine), U.oracle_state(ora))))
    # validation set empty -> mean of nothing, as in the reference (nan + warning)
    state = m.get_state()
    assert len(state) == 2
    fn = pickle.loads(pickle.dumps(state[0]))
    batch = p['X'][:B]
    P = fn(batch, np.ones((B, n), np.int8))
    _, Pref = ora.token_distributions(batch)
    assert P.shape == (B, n, Ve) and U.rel_err(P, Pref) < 1e-5


def test_vectorspace_callback_matches_reference_golden(hip_lib, gold):
    """VectorSpaceCallback on the GPU scorer vs the reference's own callback
    (sklearn brute kNN / cdist), captured in tests/golden."""
    arrays, _ = gold
    E, projs = arrays['vs_E'], arrays['vs_proj']
    de = E.shape[1]
    for tag, top in [('10', 10), ('all', None), ('100', 100)]:
        ranked = []
        cb = scoring.VectorSpaceCallback(
            E.copy(), types.SimpleNamespace(top=top),
            types.SimpleNamespace(entity_representation_size=de),
            {i: 'w%d' % i for i in range(20)}, io.StringIO(),
            lambda t, idx, val: ranked.append((t, np.array(idx), np.array(val))))
        assert cb.should_average_input()
        for qi in range(projs.shape[0]):
            cb([1, 2], projs[qi][None, :].copy(), topic_id='q%d' % qi)
        for qi, (tid, idx, val) in enumerate(ranked):
            gidx = arrays['vs_top%s_idx_%d' % (tag, qi)]
            gval = arrays['vs_top%s_val_%d' % (tag, qi)]
            assert tid == 'q%d' % qi and len(idx) == len(gidx)
            for r in np.nonzero(idx != gidx)[0]:
                assert abs(gval[r] - val[r]) < 1e-6     # only near-ties may swap
            assert np.abs(val - gval).max() < 1e-6
        # batched path gives the same rankings
        ranked_b = []
        cb2 = scoring.VectorSpaceCallback(
            E.copy(), types.SimpleNamespace(top=top),
            types.SimpleNamespace(entity_representation_size=de), {}, None,
            lambda t, idx, val: ranked_b.append((t, np.array(idx), np.array(val))))
        cb2.process_batch([[1]] * projs.shape[0], projs.copy(),
                          [{'topic_id': 'q%d' % i} for i in range(projs.shape[0])])
        for a, b in zip(ranked, ranked_b):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_ndcg_parity_on_synthetic_queries(hip_lib):
    """Query-time nDCG@100 of the GPU ranking within 1e-4 of the oracle's."""
    rng = np.random.RandomState(12)
    V, d, Q, k = 2000, 64, 50, 100
    E = rng.randn(V, d).astype(np.float32)
    Pj = np.tanh(rng.randn(Q, d)).astype(np.float32)
    idx, val = C.score_topk(E, Pj, k)
    diffs = []
    for q in range(Q):
        rel = set(rng.choice(V, 30, replace=False).tolist()) | set(idx[q][:5].tolist())
        order, _ = O.vectorspace_rank(Pj[q].astype(np.float64), E.astype(np.float64), top=k)
        diffs.append(abs(O.ndcg_at_k(list(idx[q]), rel, k) - O.ndcg_at_k(list(order), rel, k)))
    assert max(diffs) <= 1e-4


def test_large_scoring_properties(hip_lib):
    """BASELINE configs[4]-shaped (reduced Q): sortedness, score range, and the
    top-1 of a query equal to an entity row is that entity."""
    rng = np.random.RandomState(13)
    V, d, Q, k = 100000, 128, 256, 100
    E = rng.randn(V, d).astype(np.float32)
    Pj = np.tanh(rng.randn(Q, d)).astype(np.float32)
    Pj[:8] = E[1000:1008]
    idx, val = C.score_topk(E, Pj, k)
    assert np.all(np.diff(val, axis=1) <= 0)
    assert val.min() >= 0.0 and val.max() <= 1.0 + 1e-6
    assert np.array_equal(idx[:8, 0], np.arange(1000, 1008))
    assert np.all(np.abs(val[:8, 0] - 1.0) < 1e-6)
    for q in range(8, 12):     # spot-check a few full rankings against fp64
        order, sc = O.vectorspace_rank(Pj[q].astype(np.float64), E.astype(np.float64), top=k)
        assert np.abs(val[q] - sc).max() < 1e-6
        assert len(set(idx[q]) ^ set(order)) <= 2


def test_full_c5_scoring_against_the_cpu_restatements(hip_lib):
    """BASELINE configs[4] at FULL size through the product's scorer object (the one VectorSpaceCallback holds,
    bin/query.py:239-370): 10 000 query projections x 100 000 entities, d_e = 128, top 100 in one call -- two
    5 000-row chunks on two streams, bf16 prefilter + exact fp32 re-scoring.  Checked on 640 queries spread over
    both chunks (the first 256, 128 around the chunk boundary, the last 256) against (a) oracle/sert_cpu.c, the
    multithreaded C restatement bench.py times beside it -- fp32 cosines, ties to the lowest index -- and (b) float64
    cosines: scores (cos + 1) / 2 (query.py:352-357) within 1e-6, the ranked list identical except where two
    neighbours' float64 scores are closer than 1e-6; all 10 000 rows: sorted, in range."""
    from oracle import cpu_baseline as CB
    rng = np.random.RandomState(7)
    Q, V, d, k = 10000, 100000, 128, 100
    E = rng.randn(V, d).astype(np.float32)
    Pj = np.tanh(rng.randn(Q, d)).astype(np.float32)
    sc = C.Scorer(E)
    idx, val = sc.topk(Pj, k)
    idx, val = idx.copy(), val.copy()
    sc.close()
    assert idx.shape == (Q, k) and np.all(np.diff(val, axis=1) <= 0)
    assert val.min() >= 0.0 and val.max() <= 1.0 + 1e-6
    rows = np.r_[0:256, 4936:5064, Q - 256:Q]
    En = E.astype(np.float64)
    En /= np.linalg.norm(En, axis=1, keepdims=True)
    Pn = Pj[rows].astype(np.float64)
    Pn /= np.linalg.norm(Pn, axis=1, keepdims=True)
    S = (Pn @ En.T + 1.0) / 2.0                                  # (640, V) float64
    ci = CB.score_topk(E, Pj[rows], k)
    swaps = 0
    for j, q in enumerate(rows):
        ref = S[j]
        got = idx[q]
        assert np.abs(val[q] - ref[got]).max() < 1e-6           # the reported scores are the exact ones
        kth = np.partition(ref, V - k)[V - k]
        assert ref[got].min() >= kth - 1e-6                      # nothing outside the true top k (up to a tie)
        order = np.argsort(-ref, kind='stable')[:k]
        for a, b in ((got, order), (ci[j], order)):              # the HIP path and the C restatement, each vs float64
            diff = np.nonzero(a != b)[0]
            swaps += len(diff) if a is got else 0
            for pos in diff:                                     # a disagreement must be a near-tie in float64
                assert abs(ref[a[pos]] - ref[b[pos]]) < 1e-6, (q, pos)
    assert swaps <= 0.001 * len(rows) * k                        # and they are rare: < 0.1 % of the positions


def test_c2_sized_training_is_deterministic_and_learns(hip_lib):
    """BASELINE configs[1] full size: two identical runs are BIT-identical (no
    atomics anywhere on the path) and the loss goes down."""
    B, n, z, Vw, Ve, d = 65536, 10, 10, 100000, 1000, 128
    rng = np.random.RandomState(0)
    ranks = np.minimum(rng.zipf(1.1, size=(2 * B, n)) - 1, Vw - 1)
    X = rng.permutation(Vw).astype(np.uint32)[ranks]
    # learnable structure: the label is a function of the first token
    y = (X[:, 0] % Ve).astype(np.int32)
    w = np.ones(2 * B, dtype=np.float32)
    p = dict(Rw=O.glorot_uniform(rng, (Vw, d)), Re=O.glorot_uniform(rng, (Ve, d)),
             W=O.glorot_uniform(rng, (d, d)), b=np.zeros(d, np.float32), X=X)
    finals, losses = [], []
    for run in range(2):
        eng = U.vs_engine(p, B, n, z, 0.01, keep_grads=0, seed=77, lr=0.01)
        eng.upload_dataset(C.SPLIT_TRAIN, X, y_int=y, w=w)
        ls = [eng.train_batch(s % 2) for s in range(12)]
        finals.append((eng.get_tensor(C.T_RW).copy(), eng.get_tensor(C.T_RE).copy(),
                       eng.get_tensor(C.T_W).copy()))
        losses.append(ls)
        eng.close()
    assert np.all(np.isfinite(losses[0]))
    assert losses[0] == losses[1]
    for a, b in zip(finals[0], finals[1]):
        assert np.array_equal(a, b)
    assert np.mean(losses[0][-2:]) < np.mean(losses[0][:2])


def test_device_sampler_is_uniform(hip_lib):
    """Device Philox negatives: iid uniform over entities (models.py:970-973) --
    chi-square over 64 entities, checked through the loss at W=0 (any sample
    gives (1+z) log 2) and through the entity-gradient row sums."""
    B, n, z, Vw, Ve, dw, de = 4096, 2, 16, 50, 64, 8, 8
    p = U.make_vs_problem(21, B, n, z, Vw, Ve, dw, de, weights='ones')
    p['W'][:] = 0
    p['b'][:] = 0.5           # p = tanh(0.5) constant => dR_e[e] = count(e) * du * p
    p['Re'][:] = 0
    p['y'][:] = 0
    eng = U.vs_engine(p, B, n, z, 0.0, seed=5)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    loss = eng.train_batch(0)
    assert abs(loss - (1 + z) * np.log(2)) < 1e-5
    g = eng.get_tensor(C.T_GRAD_RE, (Ve, de))
    per_neg = (0.5 / B) * np.tanh(0.5)           # du for a negative with sigma = 1/2
    counts = g[:, 0] / per_neg
    counts[0] += B                                # the positives (entity 0) pull the other way
    assert abs(counts.sum() - B * z) < 1e-2 * B * z
    expected = B * z / Ve
    chi2 = ((counts - expected) ** 2 / expected).sum()
    assert chi2 < 130.0                           # 63 dof: p(chi2 > 130) ~ 1e-6
    eng.close()


@pytest.mark.parametrize('chunks,exchange', [(None, 'zero1'), ('1', 'zero1'), ('3', 'zero1'), ('16', 'zero1'), (None, 'rows')])
def test_rccl_single_rank_communicator(hip_lib, monkeypatch, chunks, exchange):
    """ncclCommInitRank / ncclReduceScatter / ncclAllGather / ncclAllReduce / grouped ncclSend-ncclRecv
    through the C ABI with world=1 (all a 1-GPU box can run): the data-parallel exchange -- the word
    table's gradient reduce-scattered slab by slab, the optimiser on the owned pieces with the
    piece-sized state, the updated slabs all-gathered ('zero1'), or the word table owned by rows
    with its pack / all-to-all / rank-ordered sum / row-filtered optimiser and the all-gather behind
    the evaluation and the read-back ('rows': keep_grads off) -- and the small tensors all-reduced,
    is exercised and is the identity.  The communicator is attached AFTER the parameters were set
    (they move into the padded allocation) and the optimiser state is read back through the
    collective gather."""
    if chunks is not None:
        monkeypatch.setenv('SERT_AR_CHUNKS', chunks)
    monkeypatch.setenv('SERT_DP_EXCHANGE', exchange)
    keep = 0 if exchange == 'rows' else 1
    B, n, z, Vw, Ve, dw, de = 64, 3, 4, 101, 12, 16, 16
    p = U.make_vs_problem(31, B * 2, n, z, Vw, Ve, dw, de)
    neg = p['rng'].randint(0, Ve, (B, z)).astype(np.int64)
    outs = []
    for use_comm in (False, True):
        eng = U.vs_engine(p, B, n, z, 0.01, keep_grads=keep)
        if use_comm:
            eng.comm_init(C.comm_unique_id(), 0, 1)
            assert eng.comm_stats()['exchange'] == exchange
        eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
        l0 = eng.train_batch(0, neg)
        l1 = eng.train_batch(1, neg)
        ev = eng.eval_batch(C.SPLIT_TRAIN, 0, neg)
        outs.append((l0, l1, ev, eng.get_tensor(C.T_RW).copy(), eng.get_tensor(C.T_STATE0_RW).copy(),
                     eng.get_tensor(C.T_STATE1_RW).copy(), eng.get_tensor(C.T_RE).copy()))
        if use_comm:   # the state round-trips through the sharded layout
            m0 = outs[-1][4]
            eng.set_tensor(C.T_STATE0_RW, m0 * 2)
            assert np.array_equal(eng.get_tensor(C.T_STATE0_RW), m0 * 2)
        eng.close()
    # the regulariser's sum of squares is grouped per piece: losses agree to fp32 rounding
    np.testing.assert_allclose(outs[0][:3], outs[1][:3], rtol=2e-6)
    for a, b in zip(outs[0][3:], outs[1][3:]):
        assert np.array_equal(a, b)


def _write_tiny_corpus(tmp_path, kind):
    """data.npz + meta in the bin/prepare.py formats (Appendix B)."""
    rng = np.random.RandomState(5)
    Vw, Ve, n, N, Nv = 120, 12, 4, 600, 128
    words = {'w%d' % i: types.SimpleNamespace(id=i) for i in range(Vw)}
    tokens = {i: 'w%d' % i for i in range(Vw)}
    ent_inv = {i: 'E%03d' % i for i in range(Ve)}

    def make(N):
        yi = rng.randint(0, Ve, N)
        x = np.stack([(yi * 10 + rng.randint(0, 10, N)) % Vw for _ in range(n)], axis=1)
        y = sp.csr_matrix((np.ones(N, np.float32), (np.arange(N), yi)), shape=(N, Ve))
        return x.astype(np.uint8), y
    xt, yt = make(N)
    xv, yv = make(Nv)
    yo = np.empty((), dtype=object)
    yo[()] = yt
    yvo = np.empty((), dtype=object)
    yvo[()] = yv
    np.savez(str(tmp_path / 'data.npz'), x_train=xt, y_train=yo, x_validate=xv, y_validate=yvo)
    with open(str(tmp_path / 'meta'), 'wb') as f:
        for obj in (argparse_ns(window_size=n), words, tokens, ent_inv, {}):
            pickle.dump(obj, f)
    with open(str(tmp_path / 'topics'), 'w') as f:
        for e in range(Ve):
            f.write('%d;w%d w%d zzz-oov\n' % (e, e * 10 + 1, e * 10 + 2))
    with open(str(tmp_path / 'qrel'), 'w') as f:
        for e in range(Ve):
            f.write('%d 0 E%03d 1.0\n' % (e, e))
    return Ve


def argparse_ns(**kw):
    import argparse
    return argparse.Namespace(**kw)


@pytest.mark.parametrize('kind', ['vectorspace', 'loglinear'])
def test_cli_train_then_query(hip_lib, tmp_path, kind):
    """bin/train.py -> model_<epoch>.bin -> bin/query.py -> TREC run; the learned
    ranking puts the right entity first for most topics."""
    Ve = _write_tiny_corpus(tmp_path, kind)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'),
           '--meta', str(tmp_path / 'meta'), '--type', kind, '--iterations', '40', '--batch_size', '32',
           '--word_representation_size', '16', '--model_output', str(tmp_path / 'model'),
           '--seed', '1', '--loglevel', 'WARNING', '--regularization_lambda', '0.0']
    if kind == 'vectorspace':
        cmd += ['--num_negative_samples', '5', '--one_hot_classes', '--entity_representation_size', '16']
    subprocess.check_call(cmd, env=env)
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith('model_'))
    assert files[0] == 'model_0.bin' and len(files) >= 2
    last = sorted(files, key=lambda f: int(f.split('_')[1].split('.')[0]))[-1]
    with open(str(tmp_path / last), 'rb') as f:
        n_pickles = 0
        while True:
            try:
                pickle.load(f)
                n_pickles += 1
            except EOFError:
                break
    assert n_pickles == (4 if kind == 'vectorspace' else 3)
    cmdq = [sys.executable, os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'),
            '--model', str(tmp_path / last), '--topics', str(tmp_path / 'topics'),
            '--run_out', str(tmp_path / 'run'), '--loglevel', 'WARNING']
    if kind == 'vectorspace':
        cmdq += ['--top', '5']
    subprocess.check_call(cmdq, env=env)
    from sert_amd.utils import trec_utils
    with open(str(tmp_path / 'run_ef')) as f:
        run = trec_utils.parse_run(f)
    with open(str(tmp_path / 'qrel')) as f:
        qrels = trec_utils.parse_qrels(f)
    assert len(run) == Ve
    res = trec_utils.evaluate_run(run, qrels, k=100)
    assert res['ndcg_cut_100'] > 0.5, res
    assert os.path.exists(str(tmp_path / 'run_ep')) and os.path.exists(str(tmp_path / 'run_debug'))


@pytest.mark.parametrize('kind', ['vectorspace', 'loglinear'])
def test_cli_train_with_a_representation_initializer(hip_lib, tmp_path, kind):
    """bin/train.py --representation_initializer <word2vec binary> (reference bin/train.py:131-151), end to end on the GPU:
    the dump taken BEFORE the first epoch (model_0.bin, train.py:289-300) carries the pre-trained vectors in the rows of the
    words the file knows -- looked up lower-cased, the last duplicate wins -- and Glorot rows elsewhere; one epoch of training
    moves both kinds of rows, and bin/query.py reads the result."""
    from sert_amd import training
    from sert_amd.utils import embedding_utils as EU
    _write_tiny_corpus(tmp_path, kind)
    dim = 16
    rng = np.random.RandomState(3)
    known = ['w%d' % i for i in range(0, 120, 2)]                  # every second word of the vocabulary ...
    names = known + ['not-in-the-vocabulary', 'w4']                 # ... an unknown one, and w4 a second time (the last one wins)
    vecs = rng.uniform(-0.5, 0.5, (len(names), dim)).astype(np.float32)
    EU.save_binary_representations(str(tmp_path / 'pre.bin'), names, vecs)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'),
           '--meta', str(tmp_path / 'meta'), '--type', kind, '--iterations', '1', '--batch_size', '32',
           '--word_representation_size', str(dim), '--representation_initializer', str(tmp_path / 'pre.bin'),
           '--model_output', str(tmp_path / 'model'), '--seed', '2', '--loglevel', 'WARNING']
    if kind == 'vectorspace':
        cmd += ['--num_negative_samples', '5', '--one_hot_classes', '--entity_representation_size', '12']
    subprocess.check_call(cmd, env=env)
    Rw0 = training.read_checkpoint(str(tmp_path / 'model_0.bin'))['tables'][0]
    Rw1 = training.read_checkpoint(str(tmp_path / 'model_1.bin'))['tables'][0]
    assert Rw0.shape == (120, dim) and Rw0.dtype == np.float32
    want = {w: v for w, v in zip(names, vecs)}                      # (dict: the later 'w4' overrides the earlier one)
    for i in range(120):
        if 'w%d' % i in want:
            assert np.array_equal(Rw0[i], want['w%d' % i]), i
        else:
            # a Glorot row: inside +-sqrt(6 / (rows + cols)) and not one of the file's vectors
            assert np.abs(Rw0[i]).max() <= np.sqrt(6.0 / (120 + dim)) + 1e-6 and not (vecs == Rw0[i]).all(axis=1).any(), i
    assert not np.array_equal(Rw0[4], vecs[2]) and np.array_equal(Rw0[4], vecs[-1])
    moved = np.abs(Rw1 - Rw0).max(axis=1)
    assert (moved[0::2] > 0).all() and (moved[1::2] > 0).all()      # training moved pre-trained and random rows alike
    cmdq = [sys.executable, os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'),
            '--model', str(tmp_path / 'model_1.bin'), '--topics', str(tmp_path / 'topics'),
            '--run_out', str(tmp_path / 'run'), '--loglevel', 'WARNING']
    subprocess.check_call(cmdq + (['--top', '5'] if kind == 'vectorspace' else []), env=env)
    assert os.path.getsize(str(tmp_path / 'run_ef')) > 0


@pytest.mark.parametrize('kind', ['vectorspace', 'loglinear'])
def test_resumed_run_equals_uninterrupted_run(hip_lib, tmp_path, kind):
    """bin/train.py --iterations 2  ==  --iterations 1, then --resume model_1.bin --iterations 2:
    parameters, optimiser tensors and step, sampler positions and the batch shuffle continue
    exactly where the dump was taken (bit-identical tables and predict_fn weights; the reference
    cannot resume, bin/train.py:289-300 only dumps).  bin/query.py still reads the file."""
    _write_tiny_corpus(tmp_path, kind)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def train(prefix, iterations, resume=None):
        cmd = [sys.executable, os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'),
               '--meta', str(tmp_path / 'meta'), '--type', kind, '--iterations', str(iterations),
               '--batch_size', '64', '--word_representation_size', '16', '--regularization_lambda', '0.01',
               '--model_output', str(tmp_path / prefix), '--seed', '11', '--save_optimizer_state',
               '--loglevel', 'WARNING']
        if kind == 'vectorspace':
            cmd += ['--num_negative_samples', '3', '--one_hot_classes', '--entity_representation_size', '24']
        if resume:
            cmd += ['--resume', str(tmp_path / resume)]
        subprocess.check_call(cmd, env=env)

    def load(name):
        from sert_amd import training
        ck = training.read_checkpoint(str(tmp_path / name))
        return ck['tables'], ck['predict_fn'].__getstate__(), ck['trailer']

    train('full', 2)
    train('part', 1)
    train('cont', 2, resume='part_1.bin')
    assert not os.path.exists(str(tmp_path / 'cont_0.bin')) and not os.path.exists(str(tmp_path / 'cont_1.bin'))
    (ta, fa, tra), (tb, fb, trb) = load('full_2.bin'), load('cont_2.bin')
    assert len(ta) == (2 if kind == 'vectorspace' else 1)
    for a, b in zip(ta, tb):
        assert np.array_equal(a, b)
    assert np.array_equal(fa['W'], fb['W']) and np.array_equal(fa['b'], fb['b'])
    assert tra['optimizer_state']['step'] == trb['optimizer_state']['step'] > 0
    for k, v in tra['optimizer_state'].items():
        assert np.array_equal(v, trb['optimizer_state'][k]), k
    assert tra['sampler_state'] == trb['sampler_state']
    assert tra['errors']['means'] == trb['errors']['means']          # error history carried over
    # one epoch really happened in between
    t1, _, _ = load('part_1.bin')
    assert not np.array_equal(t1[0], ta[0])
    cmdq = [sys.executable, os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'),
            '--model', str(tmp_path / 'cont_2.bin'), '--topics', str(tmp_path / 'topics'),
            '--run_out', str(tmp_path / 'run'), '--loglevel', 'WARNING']
    subprocess.check_call(cmdq + (['--top', '5'] if kind == 'vectorspace' else []), env=env)
    assert os.path.getsize(str(tmp_path / 'run_ef')) > 0


def test_full_pipeline_prepare_train_query(hip_lib, tmp_path):
    """bin/prepare.py -> bin/train.py -> bin/query.py on a toy TREC corpus: the
    three stages agree on the file formats and the right entity is found."""
    from tests.test_prepare_cpu import _corpus
    _corpus(tmp_path, ndocs=60)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *cmd: subprocess.check_call([sys.executable] + list(cmd), env=env)
    run(os.path.join(ROOT, 'bin', 'prepare.py'), '--seed', '3', str(tmp_path / 'docs.trectext'),
        '--assoc_path', str(tmp_path / 'assocs'), '--window_size', '4', '--overlapping',
        '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1', '--no_instance_weights',
        '--meta_output', str(tmp_path / 'meta'), '--data_output', str(tmp_path / 'data.npz'),
        '--loglevel', 'ERROR')
    run(os.path.join(ROOT, 'bin', 'train.py'), '--data', str(tmp_path / 'data.npz'), '--meta',
        str(tmp_path / 'meta'), '--type', 'vectorspace', '--iterations', '30', '--batch_size', '64',
        '--word_representation_size', '16', '--entity_representation_size', '16',
        '--num_negative_samples', '2', '--one_hot_classes', '--regularization_lambda', '0.0',
        '--model_output', str(tmp_path / 'model'), '--seed', '1', '--loglevel', 'ERROR')
    (tmp_path / 'topics').write_text('t0;alpha beta gamma\nt1;kappa lambda sigma\nt2;red green blue\n')
    last = sorted((f for f in os.listdir(str(tmp_path)) if f.startswith('model_')),
                  key=lambda f: int(f.split('_')[1].split('.')[0]))[-1]
    run(os.path.join(ROOT, 'bin', 'query.py'), '--meta', str(tmp_path / 'meta'), '--model',
        str(tmp_path / last), '--topics', str(tmp_path / 'topics'), '--top', '3', '--run_out',
        str(tmp_path / 'run'), '--loglevel', 'ERROR')
    from sert_amd.utils import trec_utils
    with open(str(tmp_path / 'run_ef')) as f:
        ranked = {t: [e for _, e in sorted(v, reverse=True)] for t, v in trec_utils.parse_run(f).items()}
    assert ranked['t0'][0] == 'E0' and ranked['t1'][0] == 'E1' and ranked['t2'][0] == 'E2'


def test_trained_model_ndcg_parity_with_oracle(hip_lib):
    """north_star: query-time nDCG@100 within +-1e-4 of the CPU path on the same
    inputs.  Train the SAME vectorspace model (same init, batches, negatives) for
    40 steps on the GPU and with the oracle, rank 64 queries with each model's own
    parameters (GPU: device scorer; oracle: fp64 cosine), compare nDCG@100."""
    B, n, z, Vw, Ve, d = 256, 4, 5, 600, 300, 32
    steps = 40
    p = U.make_vs_problem(51, B * 8, n, z, Vw, Ve, d, d)
    # learnable structure: entity = f(first token)
    p['y'] = (p['X'][:, 0].astype(np.int64) % Ve).astype(np.int32)
    eng = U.vs_engine(p, B, n, z, 0.01, lr=0.01)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    ora = O.VectorSpaceOracle(B, n, z, p['Rw'], p['Re'], p['W'], p['b'], 0.01,
                              adam_kwargs=dict(lr=0.01))
    for s in range(steps):
        j = s % 8
        sl = slice(j * B, (j + 1) * B)
        neg = p['rng'].randint(0, Ve, size=(B, z)).astype(np.int64)
        ref = ora.train_step(p['X'][sl], p['y'][sl], p['w'][sl], neg)
        got = eng.train_batch(j, neg)
        assert abs(got - ref) <= 5e-5 * abs(ref), (s, got, ref)
    Rw_g = eng.get_tensor(C.T_RW, (Vw, d))
    Re_g = eng.get_tensor(C.T_RE, (Ve, d))
    assert U.rel_err(Rw_g, ora.R_w) < 1e-3 and U.rel_err(Re_g, ora.R_e) < 1e-3
    rng = np.random.RandomState(3)
    queries = [rng.randint(0, Vw, size=rng.randint(1, 6)) for _ in range(64)]
    avg_g = np.stack([Rw_g[q].mean(axis=0) for q in queries])
    proj_g = eng.predict_project(avg_g)
    idx, _ = C.score_topk(Re_g, proj_g, 100)
    diffs = []
    for qi, q in enumerate(queries):
        proj_o = ora.predict(ora.R_w[q].mean(axis=0))
        order, _ = O.vectorspace_rank(proj_o.astype(np.float64), ora.R_e.astype(np.float64), top=100)
        rel = set(int(t) % Ve for t in q) | set(order[:3].tolist())
        diffs.append(abs(O.ndcg_at_k(list(idx[qi]), rel, 100) - O.ndcg_at_k(list(order), rel, 100)))
    assert max(diffs) <= 1e-4, max(diffs)
    eng.close()


def test_deferred_loss_readback_gives_identical_results(hip_lib):
    """steps_per_sync > 1 (additive): same batch order, same losses, same parameters."""
    B, n, z, Vw, Ve, d = 64, 3, 4, 200, 20, 16
    p = U.make_vs_problem(61, B * 7, n, z, Vw, Ve, d, d)
    outs = []
    for sps in (1, 4):
        np.random.seed(5)
        m = models.VectorSpaceLanguageModel(
            batch_size=B, window_size=n, num_negative_samples=z, representations_init=p['Rw'],
            entity_representations_init=p['Re'], regularization_lambda=0.01,
            training_set=(p['X'], p['y'], p['w']),
            validation_set=(np.zeros((0, n), p['X'].dtype), np.zeros((0,), np.int32)))
        m.sampler_seed = 9
        m.steps_per_sync = sps
        np.random.seed(7)
        nb, mean = m.train()
        outs.append((nb, mean, m.get_representations()[0].copy()))
    assert outs[0][0] == outs[1][0] == 7
    assert outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2], outs[1][2])


def test_full_size_known_answers(hip_lib):
    """Size-independent properties at BASELINE.json's full sizes.
    C2 vectorspace: W = 0, b = 0  =>  every score is 0, loss = (1+z) log 2 exactly
    (+ the L2 term, checked through lambda = 0), whatever the tokens and negatives.
    C2-dims loglinear: W = 0, b = 0  =>  uniform distributions, loss = log V_e.
    C4-sized entity vocabulary (streaming loss path): the same, loss = log 100000;
    and a one-hot bias makes the loss of the matching label ~ 0."""
    rng = np.random.RandomState(3)
    # --- C2, vectorspace ------------------------------------------------------
    B, n, z, Vw, Ve, d = 65536, 10, 10, 100000, 1000, 128
    X = rng.randint(0, Vw, size=(B, n)).astype(np.uint32)
    p = dict(Rw=O.glorot_uniform(rng, (Vw, d)), Re=O.glorot_uniform(rng, (Ve, d)),
             W=np.zeros((d, d), np.float32), b=np.zeros(d, np.float32), X=X)
    eng = U.vs_engine(p, B, n, z, 0.0, keep_grads=0, seed=1)
    eng.upload_dataset(C.SPLIT_TRAIN, X, y_int=rng.randint(0, Ve, B).astype(np.int32),
                       w=np.ones(B, np.float32))
    assert abs(eng.train_batch(0) - (1 + z) * np.log(2)) < 2e-5
    eng.close()
    # --- C2 dims, loglinear (fused LDS path), B = 8192 -------------------------
    B = 8192
    X = rng.randint(0, Vw, size=(B, n)).astype(np.uint32)
    y = rng.randint(0, Ve, B).astype(np.int32)
    q = dict(Rw=O.glorot_uniform(rng, (Vw, d)), W=np.zeros((d, Ve), np.float32),
             b=np.zeros(Ve, np.float32), X=X)
    eng = U.ll_engine(q, B, n, 0.0)
    eng.upload_dataset(C.SPLIT_TRAIN, X, y_int=y, w=np.ones(B, np.float32))
    assert abs(eng.eval_batch(C.SPLIT_TRAIN, 0) - np.log(Ve)) < 1e-4
    assert abs(eng.train_batch(0) - np.log(Ve)) < 1e-4
    eng.close()
    # --- V_e = 100k: streaming loss path ---------------------------------------
    B, Ve, d, Vw = 64, 100000, 32, 5000
    X = rng.randint(0, Vw, size=(B, n)).astype(np.uint16)
    y = np.full(B, 77777, np.int32)
    q = dict(Rw=O.glorot_uniform(rng, (Vw, d)), W=np.zeros((d, Ve), np.float32),
             b=np.zeros(Ve, np.float32), X=X)
    eng = U.ll_engine(q, B, n, 0.0)
    eng.upload_dataset(C.SPLIT_TRAIN, X, y_int=y, w=np.ones(B, np.float32))
    assert abs(eng.eval_batch(C.SPLIT_TRAIN, 0) - np.log(Ve)) < 2e-4
    bias = np.zeros(Ve, np.float32)
    bias[77777] = 40.0                      # every token's distribution ~ one-hot on the label
    eng.set_tensor(C.T_B, bias)
    assert eng.eval_batch(C.SPLIT_TRAIN, 0) < 1e-3
    eng.close()


@pytest.mark.parametrize('kind,launcher,world,exchange,chunks', [
    ('vectorspace', 'own', 2, 'rows', None), ('loglinear', 'own', 2, 'rows', None),
    ('vectorspace', 'own', 4, 'rows', None), ('loglinear', 'own', 3, 'rows', None),
    ('vectorspace', 'own', 2, 'zero1', None), ('vectorspace', 'own', 4, 'zero1', '3'), ('loglinear', 'own', 2, 'zero1', '2'),
    ('loglinear_bigw', 'own', 2, 'rows', None), ('loglinear_bigw', 'own', 2, 'zero1', None),
    ('vectorspace', 'torchrun', 2, 'rows', None),
    ('vectorspace', 'own', 8, 'rows', None)])       # the world size of the scaling target (C3), eight ranks on one GPU
def test_ranks_on_one_gpu_match_single_process(hip_lib, tmp_path, kind, launcher, world, exchange, chunks):
    """The data-parallel step with 2-4 real ranks (one process each) on the one GPU of the test box,
    through the host-mediated exchange (RCCL refuses duplicate devices), every rank receiving exactly
    its pieces: row sharding of the batch, global 1/B scaling, rank-invariant negatives, L2 applied
    once; the word table owned BY ROWS (all-to-all of the touched parameter rows and of their gradient
    rows over the static lists, rank-ordered sum at the owner, dense optimiser on the owned rows, the
    collective all-gather behind the evaluation passes and the parameter read-back) or ZeRO-1 style
    (piecewise reduce-scatter, optimiser and its state on the owned pieces, all-gather; one slab,
    two or three); a dense W of more than 4 M elements beside an absent R_e (loglinear_bigw: sharded
    W, small bias); the loss and eval-loss reductions; the collective read-back of the sharded
    optimiser state -- against the same code run single-process.  Ranks are started by the product's
    own launcher (sert_amd.distributed, no PyTorch) and, once, by torch.distributed.run as the driver
    does.  Tolerance: fp32 reassociation of the sums."""
    import socket
    from tests import dp_worker
    out = str(tmp_path / 'dp.npz')
    env = dict(os.environ, SERT_COMM='host', OMP_NUM_THREADS='1', SERT_DP_EXCHANGE=exchange)
    if chunks:
        env['SERT_AR_CHUNKS'] = chunks
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'SERT_RDZV_DIR'):
        env.pop(k, None)
    worker = [os.path.join(U.ROOT, 'tests', 'dp_worker.py'), kind, out]
    if launcher == 'own':
        cmd = [sys.executable, '-m', 'sert_amd.distributed', str(world)] + worker
    else:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
               '--master-addr', '127.0.0.1', '--master-port', str(port)] + worker
    subprocess.run(cmd, check=True, env=env, cwd=U.ROOT, timeout=900)
    two = np.load(out)
    one = dp_worker.run(kind)
    assert str(two['exchange']) == (exchange if chunks is None else 'zero1')
    assert int(two['comm_world']) == world and float(two['comm_bytes_per_step']) > 0
    scalars = ('epoch1', 'epoch2', 'train_error', 'validation_error')
    for key in scalars:
        assert abs(float(two[key]) - float(one[key])) <= 2e-5 * abs(float(one[key])), key
    for key in [k for k in one if k not in scalars and k not in ('exchange', 'comm_world', 'comm_bytes_per_step', 'transport', 'rccl_ranks', 'rccl_lib')]:
        assert U.rel_err(two[key], one[key]) < 2e-5, key
    assert int(two['step']) == int(one['step'])


def test_two_ranks_at_c2_size_match_single_process(hip_lib, tmp_path):
    """The same check ONCE at the headline size (V_w = 100k, V_e = 1k, d = 128, window 10, global
    batch 65536 -> 32768 rows per rank): three steps, the evaluation of a batch and the full tables,
    two ranks through the host-mediated exchange by rows against one process.  At this size a rank
    serves and fetches ~20 k rows per step through lists of ~10 MB -- the offsets, counts and the
    rank-ordered sums are exercised at their real extents, not on a 200-word toy."""
    from tests import dp_worker
    out = str(tmp_path / 'dp_c2.npz')
    env = dict(os.environ, SERT_COMM='host', OMP_NUM_THREADS='1', SERT_DP_EXCHANGE='rows')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'SERT_RDZV_DIR'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'sert_amd.distributed', '2', os.path.join(U.ROOT, 'tests', 'dp_worker.py'), 'c2', out]
    subprocess.run(cmd, check=True, env=env, cwd=U.ROOT, timeout=1200)
    two = np.load(out)
    one = dp_worker.run('c2')
    assert str(two['exchange']) == 'rows'
    # by rows a rank moves fewer bytes than ZeRO-1 would
    assert float(two['comm_bytes_per_step']) < 0.8 * float(two['zero1_bytes_per_step'])
    for key in ('loss0', 'loss1', 'loss2', 'eval0'):
        assert abs(float(two[key]) - float(one[key])) <= 2e-5 * abs(float(one[key])), key
    for key in ('Rw', 'Re', 'W', 'b', 'opt_state0_rw', 'opt_state1_rw', 'opt_state0_re', 'opt_state1_re',
                'opt_state0_w', 'opt_state1_w', 'opt_state0_b', 'opt_state1_b'):
        assert U.rel_err(two[key], one[key]) < 2e-5, key


def test_bench_launches_its_own_ranks(hip_lib):
    """python bench.py --gpus 2 starts two ranks itself (no torch.distributed.run), runs the
    data-parallel C2-shaped step through the host-mediated exchange on the one GPU and prints
    exactly one JSON line."""
    import json
    env = dict(os.environ, SERT_COMM='host', SERT_DEVICE='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'SERT_RDZV_DIR'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(U.ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1',
                        '--batch', '4096', '--vocab', '20000', '--num-batches', '2', '--full'],
                       env=env, cwd=U.ROOT, stdout=subprocess.PIPE, timeout=900)
    assert r.returncode == 0
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    # the headline keeps the GLOBAL batch (strong scaling); the weak case is the sub-record
    assert rec['n_gpus'] == 2 and rec['scaling'] == 'strong'
    assert rec['config']['global_batch'] == 4096 and rec['config']['per_gpu_batch'] == 2048
    assert rec['value'] > 0 and np.isfinite(rec['last_loss'])
    # both readings of "scaling" in the top level of the (short) line: the fixed global batch and the fixed per-GPU batch
    assert rec['weak']['global_batch'] == 8192 and rec['weak']['per_gpu_batch'] == 4096 and rec['weak']['value'] > 0
    assert rec['strong']['global_batch'] == 4096 and rec['strong']['value'] == rec['value']
    assert 'rccl_ranks' in rec and len(lines[0]) < 8000

    def fracs(o):
        if isinstance(o, dict):
            for k, v in o.items():
                if k.startswith('frac') and isinstance(v, (int, float)):
                    yield k, v
                else:
                    for x in fracs(v):
                        yield x
    # two ranks on one device: no ceilings, and no fraction above 1 anywhere in the line or in the full record (sidecar file)
    assert rec['full_record']
    with open(os.path.join(U.ROOT, rec['full_record'])) as f:
        full = json.load(f)
    assert full['memory_ceilings'] is None and full['weak_scaling']['global_batch'] == 8192
    assert all(v <= 1.0 for _, v in fracs(full)), [kv for kv in fracs(full) if kv[1] > 1.0]

    assert all(v <= 1.0 for _, v in fracs(rec)), [kv for kv in fracs(rec) if kv[1] > 1.0]


def test_plain_bench_line_and_its_dumped_outputs(hip_lib, tmp_path):
    """python bench.py without --full: one line with the headline keys and none of the extra records, exactly --steps timed
    steps; --dump-outputs writes the last timed step's loss and parameters, bit for bit the same in a second run and in a
    --full run (its extra records switched off) of the same arguments."""
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'SERT_RDZV_DIR'):
        env.pop(k, None)
    full = ['--full', '--no-cpu-baseline', '--no-loglinear-extra', '--no-query-extra', '--no-c4-extra', '--no-small-extra',
            '--no-seed-extra', '--no-live-pmc']
    recs, dumps = [], []
    for tag, extra in (('a', []), ('b', []), ('full', full)):
        out = str(tmp_path / tag)
        r = subprocess.run([sys.executable, os.path.join(U.ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2',
                            '--batch', '4096', '--vocab', '20000', '--num-batches', '4', '--dump-outputs', out] + extra,
                           env=env, cwd=U.ROOT, stdout=subprocess.PIPE, timeout=600)
        assert r.returncode == 0
        lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
        assert len(lines) == 1
        recs.append(json.loads(lines[0]))
        dumps.append({f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)})
    rec = recs[0]
    assert rec['metric'] == 'training_pairs_per_sec' and rec['unit'] == 'pairs/s' and rec['higher_is_better'] is True
    assert rec['dtype'] == 'f32' and rec['steps'] == 7 and rec['warmup'] == 2 and rec['n_gpus'] == 1
    assert rec['ms_per_step'] > 0 and abs(rec['value'] - 7 * 4096 / (7 * rec['ms_per_step'] / 1000.0)) <= 1e-4 * rec['value']
    assert rec['config']['global_batch'] == 4096 and np.isfinite(rec['last_loss'])
    for k in ('kernel_us', 'loglinear', 'c4', 'query', 'seeds', 'gemm_fp32_mfma_path', 'full_record'):
        assert k not in rec, k
    assert rec['roofline'] is None and rec['cpu_baseline'] is None
    assert sorted(dumps[0]) == ['R_e', 'R_w', 'W', 'b', 'loss']
    assert dumps[0]['R_w'].shape == (20000, 128) and dumps[0]['R_w'].dtype == np.float32
    assert float(dumps[0]['loss'][0]) == pytest.approx(rec['last_loss'], rel=1e-5)
    assert 'kernel_us' in recs[2] and recs[2]['last_loss'] == rec['last_loss']
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]) and np.array_equal(dumps[0][k], dumps[2][k]), k


def test_loglinear_distinct_word_path_is_deterministic_and_matches_per_token_path(hip_lib, tmp_path):
    """C2-dims loglinear (B=2048 to keep it quick): the distinct-word path is bit-reproducible
    run to run, and agrees with the per-token path (SERT_LL_NODEDUP=1, separate process) to
    fp32 reassociation."""
    B, n, Vw, Ve, d = 2048, 10, 100000, 1000, 128
    code = '''
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import util as U
rng = np.random.RandomState(0)
B, n, Vw, Ve, d = %d, %d, %d, %d, %d
ranks = np.minimum(rng.zipf(1.1, size=(2 * B, n)) - 1, Vw - 1)
X = rng.permutation(Vw).astype(np.uint32)[ranks]
y = (X[:, 0] %% Ve).astype(np.int32)
p = dict(Rw=O.glorot_uniform(rng, (Vw, d)), W=O.glorot_uniform(rng, (d, Ve)), b=np.zeros(Ve, np.float32), X=X)
eng = U.ll_engine(p, B, n, 0.01, keep_grads=0)
eng.upload_dataset(C.SPLIT_TRAIN, X, y_int=y, w=np.ones(2 * B, np.float32))
losses = [eng.train_batch(s %% 2) for s in range(6)]
np.savez(sys.argv[1], losses=np.array(losses), Rw=eng.get_tensor(C.T_RW), W=eng.get_tensor(C.T_W))
''' % (U.ROOT, B, n, Vw, Ve, d)
    outs = []
    for tag, extra in (('a', {}), ('b', {}), ('c', {'SERT_LL_NODEDUP': '1'})):
        out = str(tmp_path / (tag + '.npz'))
        subprocess.run([sys.executable, '-c', code, out], check=True, env=dict(os.environ, **extra), cwd=U.ROOT)
        outs.append(np.load(out))
    assert np.array_equal(outs[0]['losses'], outs[1]['losses'])
    assert np.array_equal(outs[0]['Rw'], outs[1]['Rw']) and np.array_equal(outs[0]['W'], outs[1]['W'])
    assert np.allclose(outs[0]['losses'], outs[2]['losses'], rtol=2e-5)
    assert U.rel_err(outs[0]['W'], outs[2]['W']) < 1e-4
    assert U.rel_err(outs[0]['Rw'], outs[2]['Rw']) < 1e-4
    assert outs[0]['losses'][-1] < outs[0]['losses'][0]


@pytest.mark.gpu
def test_every_benchmarked_configuration_repeats_bit_for_bit(hip_lib):
    """The configurations bench.py and the README time -- C2, C4, loglinear and full softmax at C2's dims, loglinear at C4's
    tables, the reference's product-search and W3C settings -- through the Python surface as the epoch loop drives it (next-batch
    hints, loss read every step): six steps twice in fresh models, representations, optimiser state and losses bit for bit
    (tools/experiments/r04_repeat_sweep.py).  Round 4 found two schedule races by re-running at these sizes -- the previous
    step's entity chain against the next projection, a big loglinear W against its own dW GEMM -- that the small-shape tests
    never lost."""
    import subprocess
    import sys
    digests = []
    for extra in ({}, {'SERT_STREAMS': '1'}):      # ... and the same bits with the whole step on ONE stream
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'experiments', 'r04_repeat_sweep.py')], cwd=ROOT,
                           env=dict(os.environ, **extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        text = r.stdout.decode()
        assert r.returncode == 0, text[-2000:]
        lines = [l for l in text.splitlines() if 'bit-identical' in l or 'DIFFERENT' in l]
        assert len(lines) == 8 and not any('DIFFERENT' in l for l in lines), '\n'.join(lines)
        digests.append([l.split('digest')[1].strip() for l in lines])
    assert digests[0] == digests[1], digests
