"""-m gpu: full rankings of the cosine scorer on the device (sert_scorer_rank: k = None, k > 1024) -- DESIGN.md, "One ranking
order".  Every comparison is exact: indices equal, values bit-equal (any NaN equal to any NaN).  The references are the host
ordering of the same scorer's cosines (Scorer.rank(..., on_device=False)) and oracle.rank_order; which path ran is asserted
through sert_debug_scorer_rank_counts.  tests/test_score_rank_cpu.py checks the inputs."""
import types

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi as C
from sert_amd import scoring
from tests import score_rank_cases as K
from tests import util as U

pytestmark = pytest.mark.gpu

CALLS, CHUNKS, TOPK_ROWS, LDS_ROWS, CSORT_ROWS = range(5)
PATH_COUNTER = {K.PATH_TOPK: TOPK_ROWS, K.PATH_LDS: LDS_ROWS, K.PATH_CSORT: CSORT_ROWS}


def _same(got, want, what):
    (idx, val), (widx, wval) = got, want
    assert idx.shape == widx.shape and idx.dtype == np.int32 and val.dtype == np.float32, (what, idx.shape, widx.shape)
    bad = np.nonzero((idx != widx).any(axis=1))[0]
    assert bad.size == 0, (what, 'queries with a wrong index', bad[:8].tolist(), idx[bad[0]][:12].tolist(),
                           'want', widx[bad[0]][:12].tolist())
    assert U.same_bits(val, wval), (what, 'values differ in their bits')


def _counted(sc, fn):
    """fn()'s result and what it added to the first five rank counters."""
    before = sc.debug_rank_counts()
    out = fn()
    return out, [a - b for a, b in zip(sc.debug_rank_counts()[:5], before[:5])]


def _problem(case):
    if isinstance(case, str):
        p = U.exact_score_problem(case)
        return p['E'], p['P']
    V, Q = case
    return U.gaussian_score_problem(V, 16, Q)


# ---- 1. device equals host, every kernel form ------------------------------------------------------------------------------

FORMS = [('tiny', K.PATH_TOPK), ('k_is_v', K.PATH_TOPK), ((1024, 3), K.PATH_TOPK), ((1025, 3), K.PATH_LDS),
         ((4096, 3), K.PATH_LDS), ('unaligned_rows', K.PATH_LDS), ('mid', K.PATH_LDS), ('radix_fallback', K.PATH_LDS),
         ((8192, 3), K.PATH_LDS), ((8193, 3), K.PATH_CSORT), ('fused_smallest', K.PATH_CSORT), ('prefix', K.PATH_CSORT),
         ((8193, 1), K.PATH_CSORT), ((5000, 1), K.PATH_LDS)]


@pytest.mark.parametrize('case,path', FORMS, ids=[str(c) for c, _ in FORMS])
def test_device_ranking_equals_the_host_ordering(hip_lib, case, path):
    """top-k path (V <= 1024), the LDS sort in its four sizes -- with and without padding ('V 4096', 'V 8192': every slot
    used), rows that start off 16 bytes ('unaligned_rows'), thousands of exact ties ('radix_fallback': stability) -- and the
    counting-sort passes from their smallest shape (V 8193) over a bf16-prefiltered table whose slab is exact_cosine_rows'
    ('fused_smallest') to the tie-heavy 'prefix'; Q = 1 in both sorts."""
    E, P = _problem(case)
    V, Q = E.shape[0], P.shape[0]
    sc = C.Scorer(E)
    assert K.rank_path(V, None)[0] == path
    full, added = _counted(sc, lambda: sc.rank(P, None))
    assert added[CALLS] == 1 and added[CHUNKS] == 1 and added[PATH_COUNTER[path]] == Q and sum(added[2:]) == Q, added
    _same(full, sc.rank(P, None, on_device=False), (case, None))
    cos = sc.cosines(P)
    for q in range(Q):
        assert np.array_equal(full[0][q], O.rank_order(cos[q])), (case, q)
    for k in (V, V - 1, 1025, 1500, 2000):
        got, added = _counted(sc, lambda: tuple(a.copy() for a in sc.rank(P, k)))
        kpath, kk = K.rank_path(V, k)
        if k <= min(V, 1024):
            assert added[CALLS] == 0                # (Scorer.rank hands these to topk())
        else:
            assert added[CALLS] == 1 and added[PATH_COUNTER[kpath]] == Q and sum(added[2:]) == Q, (k, added)
        assert got[0].shape == (Q, kk)
        _same(got, sc.rank(P, k, on_device=False), (case, k))
        _same(got, (full[0][:, :kk], full[1][:, :kk]), (case, k, 'head of rank(None)'))
    sc.close()


# ---- 2. special values -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', K.SPECIAL_V)
def test_kernels_on_special_values(hip_lib, V):
    """+0 / -0 interleaved, NaNs of both signs, infinities, denormals, duplicates and an all-NaN row, fed to the LDS sort
    (V 300) and the counting-sort passes (V 8200) themselves."""
    rows = K.special_rows(V)
    for k in (None, 1500, 100, V - 1):
        got = C.debug_scorer_rank_select(rows, k)
        want = K.expected(rows, k)
        _same(got, want, (V, k))
        kk = got[0].shape[1]
        assert np.array_equal(got[0][1], np.arange(kk)) and np.isnan(got[1][1]).all()      # the all-NaN row
    one = C.debug_scorer_rank_select(rows[:1], None)                                        # (Q = 1: one query bit)
    _same(one, K.expected(rows[:1], None), (V, 'one row'))


@pytest.mark.parametrize('V', [1100, 8300])
def test_directionless_rows_through_the_scorer(hip_lib, V):
    """Three all-zero entity rows (0/0: NaN against every query), one zero query and one NaN query (NaN against every
    entity): NaNs last by index, an all-NaN query is 0, 1, 2, ... -- as the host ordering has it."""
    E, P = U.gaussian_score_problem(V, 16, 5, seed=7)
    E[[3, V // 2, V - 1]] = 0
    P[1] = 0
    P[3, 2] = np.nan
    sc = C.Scorer(E)
    for k in (None, 1500):
        got = sc.rank(P, k)
        _same(got, sc.rank(P, k, on_device=False), (V, k))
        kk = got[0].shape[1]
        for q in (1, 3):
            assert np.array_equal(got[0][q], np.arange(kk)) and np.isnan(got[1][q]).all()
    full = sc.rank(P, None)
    assert full[0][0][-3:].tolist() == [3, V // 2, V - 1] and np.isnan(full[1][0][-3:]).all()
    assert not np.isnan(full[1][0][:-3]).any()
    sc.close()


# ---- 3. chunking changes nothing -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', [8193, 300, 1025])
def test_two_queries_per_chunk(hip_lib, monkeypatch, V):
    """SERT_SCORE_RANK_BUDGET (read at every call) set so that two queries fit a chunk: Q = 7 runs in 4 chunks and answers as
    under the default budget.  V 8193: the counting-sort passes; V 1025: the LDS sort; V 300 has kk = 300 <= 1024, which
    include/sert_hip.h gives to the top-k path -- chunked by the same budget -- so that is the path asserted there."""
    E, P = U.gaussian_score_problem(V, 16, 7, seed=11)
    path = K.rank_path(V, None)[0]
    sc = C.Scorer(E)
    want, added = _counted(sc, lambda: sc.rank(P, None))
    assert added[CHUNKS] == 1 and added[PATH_COUNTER[path]] == 7
    monkeypatch.setenv('SERT_SCORE_RANK_BUDGET', str(K.chunk_bytes(V, None, 2)))
    got, added = _counted(sc, lambda: sc.rank(P, None))
    assert added[CALLS] == 1 and added[CHUNKS] == 4 and added[PATH_COUNTER[path]] == 7, added
    _same(got, want, (V, 'two per chunk'))
    monkeypatch.setenv('SERT_SCORE_RANK_BUDGET', '1')
    got, added = _counted(sc, lambda: sc.rank(P, None))
    assert added[CHUNKS] == 7, added                # at least one query always goes through
    _same(got, want, (V, 'one per chunk'))
    monkeypatch.delenv('SERT_SCORE_RANK_BUDGET')
    fresh = C.Scorer(E)
    _same(fresh.rank(P[4:5], None), (want[0][4:5], want[1][4:5]), (V, 'a query alone'))
    fresh.close()
    sc.close()


def test_the_2048_query_cap(hip_lib):
    """Q = 2049 at V = 8193 under the default budget: the cap of a sorted chunk makes two chunks, the second of one query
    (one query bit)."""
    V, Q = 8193, 2049
    E, P = U.gaussian_score_problem(V, 16, Q, seed=13)
    assert K.chunk_bytes(V, None, 2048) < (2 << 30)
    sc = C.Scorer(E)
    (idx, val), added = _counted(sc, lambda: sc.rank(P, None))
    assert added[CHUNKS] == 2 and added[CSORT_ROWS] == Q, added
    rows = [0, 2047, 2048]
    _same((idx[rows], val[rows]), sc.rank(P[rows], None, on_device=False), 'rows 0, 2047, 2048')
    cos = sc.cosines(P)
    sc.close()
    for q in range(Q):
        assert np.array_equal(idx[q], O.rank_order(cos[q])), q
    assert U.same_bits(val, (np.take_along_axis(cos, idx.astype(np.int64), axis=1) + np.float32(1)) / np.float32(2))


# ---- 4. prefix -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['prefix', (40000, 8)], ids=str)
def test_a_deeper_k_is_the_head_of_the_full_ranking(hip_lib, case):
    E, P = _problem(case)
    sc = C.Scorer(E)
    full = sc.rank(P, None)
    for k in (1500, 2000):
        _same(sc.rank(P, k), (full[0][:, :k], full[1][:, :k]), (case, k))
    sc.close()


def test_topk_is_the_head_below_the_prefilter(hip_lib):
    E, P = U.gaussian_score_problem(20000, 16, 8, seed=17)
    sc = C.Scorer(E)
    full = sc.rank(P, None)
    for k in (1, 100, 1024):
        _same(tuple(a.copy() for a in sc.rank(P, k)), (full[0][:, :k], full[1][:, :k]), k)
    sc.close()


# ---- 5. reuse --------------------------------------------------------------------------------------------------------------

def test_a_reused_scorer_answers_as_a_fresh_one(hip_lib):
    V = 40000
    E, P = U.gaussian_score_problem(V, 16, 40, seed=19)
    steps = [('topk', 4, 10), ('rank', 6, None), ('scores', 9, None), ('rank', 14, 1500), ('topk', 20, 1024), ('rank', 40, None)]

    def do(sc, op, q, k):
        if op == 'scores':
            return (sc.scores(P[:q]),)
        return tuple(a.copy() for a in (sc.topk(P[:q], k) if op == 'topk' else sc.rank(P[:q], k)))

    sc = C.Scorer(E)
    reused = [do(sc, *s) for s in steps]
    sc.close()
    for s, got in zip(steps, reused):
        fresh = C.Scorer(E)
        want = do(fresh, *s)
        fresh.close()
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and (np.array_equal(a, b) if a.dtype == np.int32 else U.same_bits(a, b)), s


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------

def test_arguments(hip_lib):
    E, P = U.gaussian_score_problem(1200, 16, 3, seed=23)
    sc = C.Scorer(E)
    lib = C.load()
    idx = np.empty((3, 1200), dtype=np.int32)
    val = np.empty((3, 1200), dtype=np.float32)
    for k in (0, -2):
        with pytest.raises(C.SertError, match='k must be'):
            sc.rank(P, k)
        assert lib.sert_scorer_rank(sc._h, P.ctypes.data, 3, k, idx.ctypes.data, val.ctypes.data) != 0
        assert b'k must be -1 (every entity) or positive' in lib.sert_last_error()
    got, added = _counted(sc, lambda: sc.rank(P, 5000))
    assert got[0].shape == (3, 1200) and added[LDS_ROWS] == 3
    _same(got, sc.rank(P, None), 'k above V ranks V')
    assert lib.sert_scorer_rank(sc._h, P.ctypes.data, 3, 1024, idx.ctypes.data, val.ctypes.data) == 0     # kk <= 1024 ...
    t_idx, t_val = sc.topk(P, 1024)
    assert np.array_equal(idx.reshape(-1)[:3 * 1024].reshape(3, 1024), t_idx)                               # ... is topk(kk)
    assert U.same_bits(val.reshape(-1)[:3 * 1024].reshape(3, 1024), t_val)
    with pytest.raises(C.SertError, match='k > 1024'):
        sc.topk(P, 1025)
    sc.close()


# ---- 7. the query callback -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', [300, 8193])
@pytest.mark.parametrize('top', [None, 2000])
def test_callback_ranks_on_the_device(hip_lib, V, top):
    """bin/query.py --type vectorspace with --top unset and --top 2000 (above V_e at V = 300: every entity): process_batch
    hands rank_callback what the host ordering gives."""
    E, P = U.gaussian_score_problem(V, 16, 5, seed=29)
    ranked = []
    cb = scoring.VectorSpaceCallback(E.copy(), types.SimpleNamespace(top=top), types.SimpleNamespace(entity_representation_size=16),
                                     {}, None, lambda t, idx, val: ranked.append((t, np.array(idx), np.array(val))))
    before = cb.scorer.debug_rank_counts()
    cb.process_batch([[1]] * 5, P.copy(), [{'topic_id': 'q%d' % i} for i in range(5)])
    added = [a - b for a, b in zip(cb.scorer.debug_rank_counts()[:5], before[:5])]
    path, kk = K.rank_path(V, top)
    assert added[CALLS] == 1 and added[PATH_COUNTER[path]] == 5, added
    widx, wval = cb.scorer.rank(P, cb.n_neighbors, on_device=False)
    assert len(ranked) == 5
    for q, (tid, idx, val) in enumerate(ranked):
        assert tid == 'q%d' % q and idx.dtype == np.int64 and idx.shape == (kk,)
        assert np.array_equal(idx, widx[q]) and U.same_bits(val, wval[q])
