"""CPU: the inputs of the loglinear word fold-in tests on label ROWS have the structure they exist for
(tests/ll_wfold_rows_cases.py), and the identity the device path rests on holds in float64 with a dense Y: with
    qdq_il = Q_il dQ_il,   s_i = sum_l qdq_il,   dJ_i = -Q_i s_i + qdq_i
the new word rows' gradient is S_v = sum of dJ over v's occurrences, Rsum_v = <mask_v, S_v>, dZ_v = mask_v S_v - P_v Rsum_v,
G = dZ W^T + lambda / B Nv -- what tests/test_ll_wfold_inputs_cpu.py shows for integer labels, at its tolerance.  No device.
"""
import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi
from tests import ll_wfold_rows_cases as LR

upload_csr = _capi.LlWordFoldIn.upload_csr      # the binding everything here is about: without it there is nothing to prove inputs for


@pytest.fixture(scope='module')
def cases():
    return {name: LR.make_case(name) for name in LR.CASES}


def _counts(c):
    return np.diff(c['indptr'])


@pytest.mark.parametrize('name', sorted(LR.CASES))
def test_case_has_its_structure(cases, name):
    c = cases[name]
    Vw, Nw, Ve, d, n, B = (c[k] for k in ('Vw', 'Nw', 'Ve', 'd', 'n', 'B'))
    X, tok = c['X'], LR.new_tokens(c)
    M = c['M']
    assert X.shape == (M, n) and X.min() >= 0 and X.max() < Vw + Nw and c['Nv0'].shape == (Nw, d)
    assert M == 3 * B + LR.TRAILING and M // B == c['batches'] >= LR.STEPS
    # canonical CSR over the trained entities: what sert_ll_wfold_upload_csr accepts
    indptr, indices, data = c['indptr'], c['indices'], c['data']
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.shape == (M + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all() and indptr[-1] == indices.size == data.size
    assert indices.size == 0 or (indices.min() >= 0 and indices.max() < Ve)
    for i in range(M):
        assert (np.diff(indices[indptr[i]:indptr[i + 1]]) > 0).all(), (name, i)
    assert c['Y'].shape == (M, Ve) and c['Y'].nnz == indices.size and c['Y'].has_sorted_indices
    assert np.array_equal(c['Ydense'], c['Y'].toarray()) and np.isfinite(data).all() and (data >= 0).all()
    counts = _counts(c)
    per_batch = [counts[i * B:(i + 1) * B] for i in range(c['batches'])]
    plans = [LR.expected_plan(c, i) for i in range(c['batches'])]
    # the form and vec each V_e selects
    stream = name in ('ve1025', 've1028')
    assert all(p['form'] == ('stream' if stream else 'reg') and p['vec'] == (Ve % 4 == 0) and p['labels'] == 'rows' for p in plans)
    assert (Ve > LR.REG_MAX_VE) == stream
    row = lambda i: indices[indptr[i]:indptr[i + 1]].tolist()
    if name == 'mixed':
        for k in per_batch[:LR.STEPS]:
            assert set(k.tolist()) == {0, 1, 2, 3, Ve}
        assert row(2) == [0, Ve - 1] and (tok[2] < 0).all()
        assert np.bincount(tok[0][tok[0] >= 0], minlength=Nw).max() >= 2
        sums = np.asarray(c['Ydense'].sum(axis=1))
        assert (np.abs(sums[counts > 0] - 1.0) > 1e-3).all()
    elif name == 've8':
        assert Ve == 8 and plans[0]['vec'] and row(1) == [4, 5, 6, 7] and 1 < B
    elif name == 'wide':
        assert Ve == 700 and Ve % 4 == 0
        for k in per_batch:
            assert tuple(k[:4]) == LR.WIDE_COUNTS
        assert min(LR.WIDE_COUNTS) < LR.WG and LR.WG in LR.WIDE_COUNTS and max(LR.WIDE_COUNTS) > 2 * LR.WG
        for i in range(4):
            assert abs(float(c['Ydense'][i].sum()) - 0.55) < 0.2          # (mean of U(0.1, 1) over the count)
    elif name == 've1024':
        assert Ve == LR.REG_MAX_VE and plans[0]['vec']
    elif name == 've1025':
        assert Ve == LR.REG_MAX_VE + 1 and not plans[0]['vec']
    elif name == 've1028':
        assert Ve == LR.REG_MAX_VE + 4 and plans[0]['vec']
    elif name == 'no_labels':
        assert c['lam'] == 0.0 and (per_batch[0] == 0).all() and all((k > 0).all() for k in per_batch[1:])
        assert (tok[:B] >= 0).any()                    # (the batch does hold new words: their gradient is zero, not absent)
    elif name == 'one_hot':
        base = LR.LW.make_case('base')
        assert (counts == 1).all() and np.array_equal(indices, base['y']) and (data == 1).all()
        assert all(c[k] is base[k] for k in ('X', 'w', 'Rw', 'W', 'b', 'Nv0'))
    elif name == 'stored_zero':
        zero_rows = np.repeat(np.arange(M), counts)[data == 0]
        assert np.array_equal(zero_rows, np.arange(0, M, 3)) and c['Y'].nnz > np.count_nonzero(c['Ydense'])
    elif name == 'n1':
        assert n == 1 and (counts == 2).all()
    elif name == 'n32':
        assert n == 32 and (counts == 2).all()
    elif name == 'all_new':
        assert X.min() >= Vw
    elif name == 'batch_of_one':
        assert B == 1
    elif name == 'clip_live_rows':
        assert (counts == 2).all() and (data == 0.5).all()
    if stream:
        assert counts[0] == Ve and counts[1] == 0 and row(0) == list(range(Ve))


def reassociated_gradient(c, Nv, batch, dt):
    """The gradient of Nv on `batch` in the association of the device path with label rows, restated in NumPy: the distinct
    words' log distributions once, J as a sum of clipped rows, per entry Q dQ and their row sum, the dense dJ plus the entries,
    S / Rsum / dZ per new word, G = dZ W^T + L2.  -> (G, data loss)."""
    dt = np.dtype(dt)
    T = dt.type
    lo, hi = O.clip_bounds(dt)
    Vw, Nw, B, lam = c['Vw'], c['Nw'], c['B'], c['lam']
    X = c['X'][batch * B:(batch + 1) * B].astype(np.int64)
    Y = c['Ydense'][batch * B:(batch + 1) * B].astype(dt)
    w = c['w'][batch * B:(batch + 1) * B].astype(dt)
    W, b = c['W'].astype(dt), c['b'].astype(dt)
    ext = np.concatenate([c['Rw'].astype(dt), np.asarray(Nv, dtype=dt)], axis=0)
    P = O.softmax_rows((ext @ W + b).astype(dt))                    # one row per word of the extended vocabulary
    inside = ((P >= lo) & (P <= hi)).astype(dt)
    Lc = np.log(np.clip(P, lo, hi))
    J = np.zeros((B, W.shape[1]), dtype=dt)
    for j in range(X.shape[1]):
        J += Lc[X[:, j]]
    Q = O.softmax_rows(J)
    Qc = np.clip(Q, lo, hi)
    g = (w / T(B)).astype(dt)
    qdq = Q * np.where((Q >= lo) & (Q <= hi), -(g[:, None] * Y) / Qc, T(0))      # zero off the row's entries
    s = qdq.sum(axis=1, dtype=dt)
    dJ = -Q * s[:, None] + qdq
    S = np.zeros((Nw, W.shape[1]), dtype=dt)
    for j in range(X.shape[1]):                                     # a word twice in a window counts dJ_i twice
        new = X[:, j] >= Vw
        np.add.at(S, X[new, j] - Vw, dJ[new])
    Pn, Mn = P[Vw:], inside[Vw:]
    Rsum = (Mn * S).sum(axis=1, dtype=dt)
    dZ = Mn * S - Pn * Rsum[:, None]
    G = (dZ @ W.T).astype(dt)
    if lam > 0.0:
        G = G + T(lam) / T(B) * np.asarray(Nv, dtype=dt)
    loss = T((-(Y * np.log(Qc)).sum(axis=1, dtype=dt) * w).sum(dtype=dt) / T(B))
    return G.astype(dt), loss


@pytest.mark.parametrize('name', sorted(LR.CASES))
def test_identity_in_float64(cases, name):
    """S, Rsum = <mask, S> and G = dZ W^T with a dense Y equal the twin's gradient (LogLinearOracle on ExtW) in float64 to
    1e-12, over the three steps of the twin's own trajectory."""
    c = cases[name]
    tw = LR.LlWordFoldInRowsTwin(c, np.float64)
    for s in range(LR.STEPS):
        G, loss = reassociated_gradient(c, tw.Nv, s, np.float64)
        data, g, _ = tw.loss_and_grads(s)
        scale = max(1e-300, float(np.abs(g).max()))
        assert float(np.abs(G - g).max()) <= 1e-12 * scale, (name, s, float(np.abs(G - g).max()), scale)
        assert abs(loss - data) <= 1e-12 * abs(data)
        tw.train_step(s)


def test_no_labels_moves_nothing_in_the_twin(cases):
    """no_labels: the twin's loss on batch 0 is exactly 0 and its step leaves Nv and both accumulators as they were."""
    c = cases['no_labels']
    for dt in (np.float32, np.float64):
        tw = LR.LlWordFoldInRowsTwin(c, dt)
        before = [a.copy() for a in (tw.Nv, tw.opt.accu[0], tw.opt.delta[0])]
        assert tw.train_step(0) == 0.0
        for a, b in zip(before, (tw.Nv, tw.opt.accu[0], tw.opt.delta[0])):
            assert np.array_equal(a, b)


def test_one_hot_twin_is_the_integer_twin(cases):
    """one_hot: the rows twin and ll_wfold_cases' integer twin compute the same float64 trajectory (the oracle builds the
    same dense Y from the integer labels)."""
    c = cases['one_hot']
    a, b = LR.LlWordFoldInRowsTwin(c, np.float64), LR.LW.LlWordFoldInTwin(LR.LW.make_case('base'), np.float64)
    for s in range(LR.STEPS):
        la, lb = a.train_step(s), b.train_step(s)
        assert abs(la - lb) <= 1e-12 * abs(lb)
    assert np.abs(a.Nv - b.Nv).max() <= 1e-12 * np.abs(b.Nv).max()


def test_clip_live_rows_report(cases):
    c = cases['clip_live_rows']
    rep = LR.clip_report(c)
    print('clip_live_rows (seed attempt %d): %r' % (c['attempt'], rep))
    assert LR.clip_ok(rep)
    assert rep['frozen_clipped'] > 0 and rep['new_clipped'] > 0 and rep['margin'] > LR.CLIP_MARGIN
    assert all(0 < k < total for k, total in zip(rep['labels_clipped'], rep['labels_total']))
    assert rep['labels_total'] == [2 * c['B']] * LR.STEPS
