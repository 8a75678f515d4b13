"""-m gpu: one ranking order across every path of the cosine scorer ("One ranking order").

The exact problems of tests/util.py have cosines that are multiples of 1/16 -- exact in fp32 in any summation order and in
bf16 (tests/test_score_contract_cpu.py proves it on every shape used here) -- so indices must EQUAL oracle.rank_order of the
integer cosines and values must be bit-equal: no gap exemption.  The path a shape is there for is asserted through
sert_debug_scorer_counts, not assumed."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import util as U

pytestmark = pytest.mark.gpu

MODES = {'default': {}, 'fp32_filter': {'SERT_SCORE_FP32': '1'}, 'materialise': {'SERT_SCORE_MATERIALISE': '1'}}
FUSED_CALLS, BF16_CALLS, CHUNKS, FLAGGED, DIRECT_ROWS, DEMOTED = range(6)

_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_score_contract import run_jobs
d = np.load(sys.argv[2])
jobs = []
for j in range(int(d['njobs'])):
    jobs.append((d['E%d' % j], [(d['P%d_%d' % (j, c)], int(k)) for c, k in enumerate(d['k%d' % j])]))
out = {}
for j, (results, counts) in enumerate(run_jobs(jobs)):
    out['counts%d' % j] = np.array(counts)          # (calls, 6)
    for c, (idx, val) in enumerate(results):
        out['idx%d_%d' % (j, c)] = idx
        out['val%d_%d' % (j, c)] = val
np.savez(sys.argv[3], **out)
'''


def run_jobs(jobs):
    """jobs: [(E, [(P, k), ...]), ...] -> per job ([(idx, val) per call], [path counts of that call alone per call]): one
    Scorer per job, topk per call."""
    out = []
    for E, calls in jobs:
        sc = C.Scorer(E)
        results, counts, before = [], [], sc.debug_path_counts()
        for P, k in calls:
            idx, val = sc.topk(P, k)
            results.append((idx.copy(), val.copy()))
            after = sc.debug_path_counts()
            counts.append([a - b for a, b in zip(after[:DEMOTED], before[:DEMOTED])] + [after[DEMOTED]])
            before = after
        out.append((results, counts))
        sc.close()
    return out


def run_jobs_under(mode, jobs):
    """run_jobs in this process, or in a fresh one under the mode's environment (the knobs are read once per process)."""
    if not MODES[mode]:
        return run_jobs(jobs)
    arrays = {'njobs': len(jobs)}
    for j, (E, calls) in enumerate(jobs):
        arrays['E%d' % j] = E
        arrays['k%d' % j] = np.array([k for _, k in calls])
        for c, (P, _) in enumerate(calls):
            arrays['P%d_%d' % (j, c)] = P
    with tempfile.TemporaryDirectory() as tmp:
        inp, outp = os.path.join(tmp, 'in.npz'), os.path.join(tmp, 'out.npz')
        np.savez(inp, **arrays)
        subprocess.run([sys.executable, '-c', _CHILD, U.ROOT, inp, outp], check=True, env=dict(os.environ, **MODES[mode]),
                       timeout=600)
        r = np.load(outp)
        return [([(r['idx%d_%d' % (j, c)], r['val%d_%d' % (j, c)]) for c in range(len(calls))], r['counts%d' % j].tolist())
                for j, (_, calls) in enumerate(jobs)]


def assert_equals_contract(got, want, what):
    (idx, val), (widx, wval) = got, want
    assert idx.shape == widx.shape, (what, idx.shape, widx.shape)
    bad = np.nonzero((idx != widx).any(axis=1))[0]
    assert bad.size == 0, (what, 'queries with a wrong index', bad[:8].tolist(), 'first', idx[bad[0]][:12].tolist(),
                           'want', widx[bad[0]][:12].tolist(), val[bad[0]][:12].tolist())
    assert U.same_bits(val, wval), (what, 'values differ in their bits')


# ---- 1. every selection path ---------------------------------------------------------------------------------------------

MATERIALISED_CASES = [('tiny', (1, 10, 50)), ('k_is_v', (300,)), ('unaligned_rows', (100,)), ('mid', (100, 1024)),
                      ('radix_fallback', (400, 1024))]
FUSED_CASES = [('fused_smallest', (10, 400, 1)), ('fused_ragged', (10, 1024)), ('fused_dense', (1024,))]


def _exact_case(name, ks):
    p = U.exact_score_problem(name)
    c16 = U.exact_cos16(p['Pi'], p['Ei'])
    return p, [U.exact_expected(c16, k) for k in ks]


@pytest.mark.parametrize('name,ks', MATERIALISED_CASES)
def test_selection_of_a_materialised_table_equals_the_contract(hip_lib, name, ks):
    """V < 32768: one GEMM + topk_rows -- the two-pass histogram selection ('tiny', 'k_is_v', 'mid'; 'unaligned_rows':
    V % 4 = 3, scalar loads of rows that start off 16 bytes) and its radix fallback ('radix_fallback': more than 2048
    entities in the threshold bin, tests/test_score_contract_cpu.py)."""
    p, want = _exact_case(name, ks)
    (results, counts), = run_jobs([(p['E'], [(p['P'], k) for k in ks])])
    for k, got, w in zip(ks, results, want):
        assert_equals_contract(got, w, (name, k))
    for c in counts:
        assert c[FUSED_CALLS] == 0 and c[DIRECT_ROWS] == p['P'].shape[0], counts


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name,ks', FUSED_CASES)
def test_selection_of_a_fused_table_equals_the_contract(hip_lib, name, ks, mode):
    """V >= 32768: sampled threshold (k = 10: approx_kth_rows, rs <= 64; k = 400 / 1024: kth_largest_rows) + filtering GEMM +
    selection from the lists, in bf16 with exact re-scoring (default) or in fp32 (SERT_SCORE_FP32=1); queries whose ties
    defeat the threshold are flagged and redone by the materialising path, which SERT_SCORE_MATERIALISE=1 takes for all."""
    p, want = _exact_case(name, ks)
    Q = p['P'].shape[0]
    (results, counts), = run_jobs_under(mode, [(p['E'], [(p['P'], k) for k in ks])])
    print(name, ks, mode, 'path counts', counts)
    for k, got, w in zip(ks, results, want):
        assert_equals_contract(got, w, (name, k, mode))
    for k, c in zip(ks, counts):
        if mode == 'materialise':
            assert c[FUSED_CALLS] == 0 and c[DIRECT_ROWS] == Q, (k, counts)
            continue
        assert c[FUSED_CALLS] == 1 and c[DIRECT_ROWS] == 0 and c[BF16_CALLS] == (1 if mode == 'default' else 0), (k, counts)
        if (name, k) == ('fused_ragged', 1024):
            # every nnz-16 query has ~15 000 entities at or above the sampled threshold: more than the 4096 the lists may
            # hold ('fused_dense' is the k = 1024 shape that keeps fused rows)
            assert c[FLAGGED] > 0, (k, counts)
        else:
            # both ends of the fused path ran in THIS call: rows that kept the fused result, and rows it flagged (mass ties)
            assert 0 < c[FLAGGED] < Q, (k, counts)


def test_k_beyond_the_table_or_the_device_limit_is_refused(hip_lib):
    p = U.exact_score_problem('tiny')
    sc = C.Scorer(p['E'])
    with pytest.raises(C.SertError, match='k exceeds the number of entities'):
        sc.topk(p['P'], 51)
    sc.close()
    p = U.exact_score_problem('mid')
    sc = C.Scorer(p['E'])
    with pytest.raises(C.SertError, match='k > 1024 is not supported'):
        sc.topk(p['P'], 1025)
    sc.close()


# ---- 2. special values ---------------------------------------------------------------------------------------------------

ZERO_ROWS = (0, 16, 4096, 5, 21)        # three the stride-16 sample of the fused path sees, two it does not
NAN_BITS = {7: 0x7fc00000, 9: 0xffc00000, 11: 0x7f800000}     # entity row -> one entry of it: +NaN, -NaN, +inf


def _special_problem(name):
    p = U.exact_score_problem(name)
    E, P = p['E'].copy(), p['P'].copy()
    E[list(ZERO_ROWS)] = 0
    for row, bits in NAN_BITS.items():
        E[row, 3] = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    P[4] = 0                                   # a zero query
    P[5, 2] = np.nan                           # a NaN query, ordinary ones around them
    c16 = U.exact_cos16(p['Pi'], p['Ei'])
    bad_e = list(ZERO_ROWS) + list(NAN_BITS)
    # a table with fewer than k entities that have a direction: the first 7 rows of a block of 300, the rest zero
    Es = p['E'].copy()
    Es[307:] = 0
    Es[:300] = 0
    bad_s = [e for e in range(Es.shape[0]) if not 300 <= e < 307]
    return (E, P, c16, bad_e), (Es, p['P'], c16, bad_s)


@pytest.mark.parametrize('name,ks', [('mid', (10, 400)), ('fused_smallest', (10, 400))])
def test_directionless_rows_rank_last_on_every_path(hip_lib, name, ks):
    """Zero, NaN and infinite entity rows (0/0 and inf/inf in the normalisation) and zero / NaN queries score NaN: after
    every number, by lowest index, k results always -- under the default, SERT_SCORE_FP32=1 and SERT_SCORE_MATERIALISE=1
    alike.  On the fused shape some rows with NaN entities in their table keep the fused result (a NaN never enters a
    candidate list) and some are flagged; the table with 7 numbers is flagged throughout (fewer than k candidates).
    A cosine of -0 is NOT in these problems, nor in any the scorer can be given: orthogonal supports give zero products of
    either sign, but every dot product of the library starts from a +0 accumulator and +0 + -0 = +0, so the device computes
    +0.  The -0 clause is tested on the selection kernels directly, test_negative_zero_ties_with_positive_zero."""
    (E, P, c16, bad_e), (Es, Ps, _, bad_s) = _special_problem(name)
    want = [U.exact_expected(c16, k, nan_entities=bad_e, nan_queries=(4, 5)) for k in ks]
    want_s = [U.exact_expected(c16, k, nan_entities=bad_s) for k in ks]
    for w in want_s:          # 7 numbers, then the NaN entities from index 0 on
        assert sorted(w[0][0][:7].tolist()) == list(range(300, 307)) and w[0][0][7:10].tolist() == [0, 1, 2]
    for w in want:
        assert w[0][4].tolist() == list(range(w[0].shape[1])) and np.isnan(w[1][5]).all()
    first = None
    for mode in sorted(MODES):
        (res, counts), (res_s, counts_s) = run_jobs_under(mode, [(E, [(P, k) for k in ks]), (Es, [(Ps, k) for k in ks])])
        print(name, mode, 'path counts', counts, counts_s)
        if name == 'fused_smallest' and mode != 'materialise':
            for k, c, cs in zip(ks, counts, counts_s):
                assert c[FUSED_CALLS] == 1 and 2 <= c[FLAGGED] < P.shape[0], (k, counts)      # (the zero and the NaN query at least)
                assert cs[FUSED_CALLS] == 1 and cs[FLAGGED] == Ps.shape[0], (k, counts_s)
        for k, got, w, got_s, ws in zip(ks, res, want, res_s, want_s):
            assert_equals_contract(got, w, (name, k, mode, 'special rows'))
            assert_equals_contract(got_s, ws, (name, k, mode, 'fewer than k numbers'))
        if first is None:
            first = (res, res_s)
        for a, b in zip(first[0] + first[1], res + res_s):          # the three modes agree with each other
            assert np.array_equal(a[0], b[0]) and U.same_bits(a[1], b[1]), mode


def _signed_zero_rows(V, seed):
    """(4, V) float32 'cosines': mostly negative multiples of 1/16, per 64 entities about four zeros of either sign, four
    positive multiples of 1/16 and now and then a NaN; row 0 begins -0, +0, row 1 +0, -0."""
    rng = np.random.RandomState(seed)
    S = -(rng.randint(1, 17, size=(4, V)) / 16.0).astype(np.float32)
    kind = rng.randint(0, 64, size=(4, V))
    S[kind < 2] = 0.0
    S[(kind >= 2) & (kind < 4)] = -0.0
    pos = (kind >= 4) & (kind < 8)
    S[pos] = (rng.randint(1, 17, size=(4, V)) / 16.0).astype(np.float32)[pos]
    S[kind == 8] = np.nan
    S[0, :2] = (-0.0, 0.0)
    S[1, :2] = (0.0, -0.0)
    assert np.signbit(S[S == 0]).any() and not np.signbit(S[S == 0]).all()
    return S


@pytest.mark.parametrize('kernel,V,k', [('topk_rows', 512, 512), ('topk_rows', 4099, 300), ('topk_rows', 6000, 400),
                                        ('topk_from_groups', 2048, 200)])
def test_negative_zero_ties_with_positive_zero(hip_lib, kernel, V, k):
    """No dot product of the library yields -0 (see above), so the clause '+0 and -0 are equal, lowest index first' is put to
    the scorer's selection kernels on rows that hold both zeros (sert_debug_scorer_select): topk_rows<false> -- histogram
    selection, and at V = 6000, where the zeros are most of the row's top and share one key bin, its radix fallback -- and
    topk_from_groups on the lists the fp32 filter would leave for the threshold -0 (desc_key keys, canonicalised in the
    gather).  Plain desc_key ranks every +0 before every -0.  The bf16 path's rescore_sort_emit makes its keys from
    exact_dot32, which cannot return -0: score_key's -0 branch is unreachable there and not tested."""
    S = _signed_zero_rows(V, 77 + V)
    if V == 6000:
        S[:, 500:] = np.where(np.arange(V - 500) % 3 == 0, np.float32(0.0), np.float32(-0.0))     # thousands of zeros
    want_idx = np.stack([O.rank_order(row, k) for row in S]).astype(np.int32)
    want_val = (np.take_along_axis(S, want_idx.astype(np.int64), axis=1) + np.float32(1)) / np.float32(2)
    zeros = np.take_along_axis(S, want_idx.astype(np.int64), axis=1) == 0
    assert zeros.sum() > 8 and np.isnan(want_val).any() == (kernel == 'topk_rows' and k == V)
    if kernel == 'topk_from_groups':       # what that kernel needs to keep a row: k .. 1024 candidates, 16 at most per group
        passing = S >= np.float32(-0.0)
        assert passing.reshape(4, -1, 64).sum(axis=2).max() <= 16 and k <= passing.sum(axis=1).min() <= 1024
    got = C.debug_scorer_select(S, k, 0 if kernel == 'topk_rows' else 1, thr=-0.0)
    assert_equals_contract(got, (want_idx, want_val), (kernel, V, k))
    # the expectation itself interleaves the two zeros by index (it is not 'all +0, then all -0')
    z = np.signbit(np.take_along_axis(S, want_idx.astype(np.int64), axis=1)[0][zeros[0]])
    assert z.any() and not z.all() and np.any(z[:-1] & ~z[1:])


@pytest.mark.parametrize('name', ['mid', 'fused_smallest'])
def test_full_ranking_with_directionless_rows(hip_lib, name):
    """The host ordering behind Scorer.rank(q, None) on the tables of the test above: NaN after every number, by lowest
    index, equal to the contract on the integer cosines -- and the device's top-k is its head."""
    (E, P, c16, bad_e), (Es, Ps, _, bad_s) = _special_problem(name)
    for tab, qs, bad_ent, bad_q in ((E, P, bad_e, (4, 5)), (Es, Ps, bad_s, ())):
        want_idx, want_val = U.exact_expected(c16, None, nan_entities=bad_ent, nan_queries=bad_q)
        sc = C.Scorer(tab)
        full = sc.rank(qs, None)
        assert_equals_contract(full, (want_idx, want_val), (name, 'rank(None)'))
        assert np.isnan(full[1][:, -1]).all() and np.all(np.diff(full[0][0][-len(bad_ent):]) > 0)
        for k in (10, 400, 1024):
            idx, val = sc.rank(qs, k)
            assert_equals_contract((idx, val), (full[0][:, :k], full[1][:, :k]), (name, k))
        sc.close()


# ---- 3. prefix consistency -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table', ['gaussian', 'exact'])
@pytest.mark.parametrize('V', [300, 5000, 40000])
def test_topk_is_the_head_of_the_full_ranking(hip_lib, V, table):
    """Scorer.rank(q, k) on the device (k <= min(V, 1024)) against the host-ordered rank(q, None) and rank(q, 1500): one
    order, so the first is the head of the others, indices equal and values bit-equal."""
    if table == 'exact':
        p = U.exact_score_problem({300: 'k_is_v', 5000: 'mid', 40000: 'prefix'}[V])
        E, P = p['E'], p['P']
    else:
        E, P = U.gaussian_score_problem(V, 16, 100 if V == 40000 else 8)
    sc = C.Scorer(E)
    full_idx, full_val = sc.rank(P, None)
    assert full_idx.shape == (P.shape[0], V)
    for q in range(P.shape[0]):
        assert np.array_equal(np.sort(full_idx[q]), np.arange(V))
    big_idx, big_val = sc.rank(P, 1500)
    keep = min(V, 1500)
    assert np.array_equal(big_idx, full_idx[:, :keep]) and U.same_bits(big_val, full_val[:, :keep])
    cos = sc.cosines(P)
    for q in range(P.shape[0]):           # the full ranking is the contract's order of the device's own cosines
        assert np.array_equal(full_idx[q], O.rank_order(cos[q]))
    if table == 'gaussian' and V == 40000:
        # not vacuous: somewhere in the first 1024, two entities share an emitted score and differ in cosine
        assert U.count_score_collisions(cos, 1024) > 0
    for k in (1, 100, 1024):
        idx, val = sc.rank(P, k)
        kk = min(k, V)
        assert idx.shape == (P.shape[0], kk)
        assert_equals_contract((idx, val), (full_idx[:, :kk], full_val[:, :kk]), (V, table, k))
    sc.close()


# ---- 4. chunking ---------------------------------------------------------------------------------------------------------

CHUNK_V, CHUNK_D, CHUNK_K = 32768, 16, 10
CHUNK_QS = {1024: 1024, 1025: 640, 1300: 768}          # Q -> rows of the first chunk (QT: half of Q rounded up to 128)


def _chunk_problem(Q):
    """Gaussian table with the adversarial rows of test_score_topk_fused_path_adversarial_rows (a block of exact duplicates;
    the best entities off the sample stride), the queries aimed at them at both ends of every chunk and inside."""
    rng = np.random.RandomState(12)
    E = rng.randn(CHUNK_V, CHUNK_D).astype(np.float32)
    hot = rng.randn(CHUNK_D).astype(np.float32)
    E[5000:15000] = hot
    spike = rng.randn(CHUNK_D).astype(np.float32)
    off_sample = np.arange(20001, 20001 + 16 * 60, 16)
    E[off_sample] = spike + 0.01 * rng.randn(len(off_sample), CHUNK_D).astype(np.float32)
    P = np.tanh(rng.randn(1300, CHUNK_D)).astype(np.float32)[:Q]
    qt = CHUNK_QS[Q]
    # the duplicate block overflows the candidate lists: these rows are flagged for certain -- first and last row of every chunk
    flagged = sorted(set(x for x in (0, 300, qt - 1, qt, qt + 200, Q - 1) if 0 <= x < Q))
    P[flagged] = hot
    for q in (1, qt - 2, qt + 1, Q - 2):
        if 0 <= q < Q and q not in flagged:
            P[q] = spike
    return E, P, flagged


@pytest.fixture(scope='module')
def chunk_reference():
    """The materialising path's answer for every chunked shape, from one child process."""
    jobs = []
    for Q in sorted(CHUNK_QS):
        E, P, _ = _chunk_problem(Q)
        jobs.append((E, [(P, CHUNK_K)]))
    return {Q: r for Q, r in zip(sorted(CHUNK_QS), run_jobs_under('materialise', jobs))}


@pytest.mark.parametrize('Q', sorted(CHUNK_QS))
def test_two_stream_chunks_equal_the_materialised_path(hip_lib, chunk_reference, Q):
    """Q > 1024 runs in two chunks on two streams (640 + 385, 768 + 532; 1024: one), each chunk's results copied out under
    the next; rows flagged in either chunk are gathered, recomputed and scattered back as one block."""
    E, P, flagged = _chunk_problem(Q)
    (((idx, val),), (counts,)), = run_jobs([(E, [(P, CHUNK_K)])])
    print(Q, 'path counts', counts, 'aimed', flagged)
    assert counts[FUSED_CALLS] == 1 and counts[CHUNKS] == (1 if Q <= 1024 else 2), counts
    assert counts[FLAGGED] >= len(flagged), counts
    ((ridx, rval),), (rcounts,) = chunk_reference[Q]
    assert rcounts[FUSED_CALLS] == 0
    assert np.array_equal(idx, ridx) and U.same_bits(val, rval)
    assert np.array_equal(idx[0], np.arange(5000, 5000 + CHUNK_K))
    U.check_topk_against_oracle(E, P, idx, val, CHUNK_K)


# ---- 5. demotion ---------------------------------------------------------------------------------------------------------

def test_a_demoted_prefilter_changes_no_bit(hip_lib):
    """The no-gap table of test_score_topk_bf16_prefilter_no_gap_falls_back at Q = 128: more than a quarter of the rows are
    flagged, the scorer drops the bf16 prefilter for this table.  What it answers afterwards is what a fresh scorer answers."""
    rng = np.random.RandomState(29)
    V, d, k = 36000, 32, 50
    u = rng.randn(d).astype(np.float32)
    E = (u + 5e-3 * rng.randn(V, d)).astype(np.float32)
    Pn = (u + 0.05 * rng.randn(128, d)).astype(np.float32)
    Pg = np.tanh(rng.randn(40, d)).astype(np.float32)
    sc = C.Scorer(E)
    assert sc.debug_path_counts()[DEMOTED] == 0
    idx1, val1 = [a.copy() for a in sc.topk(Pn, k)]
    counts = sc.debug_path_counts()
    print('after the no-gap block', counts)
    assert counts[DEMOTED] == 1 and counts[BF16_CALLS] == 1 and counts[FLAGGED] * 4 > 128, counts
    U.check_topk_against_oracle(E, Pn[:16], idx1[:16], val1[:16], k)
    got = [[a.copy() for a in sc.topk(P, k)] for P in (Pg, Pn)]
    counts = sc.debug_path_counts()
    print('after two more blocks', counts)
    assert counts[FUSED_CALLS] == 3 and counts[BF16_CALLS] == 1, counts          # the later calls filtered in fp32
    sc.close()
    for P, (idx, val) in zip((Pg, Pn), got):
        fresh = C.Scorer(E)
        fidx, fval = fresh.topk(P, k)
        assert np.array_equal(idx, fidx) and U.same_bits(val, fval)
        fresh.close()


# ---- 6. reuse ------------------------------------------------------------------------------------------------------------

def test_a_reused_scorer_equals_fresh_ones(hip_lib):
    """Growing Q and k on one Scorer, scores() in between (it frees and re-derives the query capacity on its own): every
    answer is a fresh scorer's, bit for bit."""
    E, P = U.gaussian_score_problem(40000, 16, 700, seed=43)
    steps = [('topk', P[:5], 10), ('scores', P[:3], None), ('topk', P, 300), ('topk', P[:2], 1024), ('rank', P[:4], None)]

    def do(sc, op, p, k):
        if op == 'scores':
            return (sc.scores(p),)
        return tuple(a.copy() for a in (sc.topk(p, k) if op == 'topk' else sc.rank(p, None)))

    sc = C.Scorer(E)
    reused = [do(sc, *s) for s in steps]
    sc.close()
    for s, got in zip(steps, reused):
        fresh = C.Scorer(E)
        want = do(fresh, *s)
        fresh.close()
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.shape == b.shape and a.dtype == b.dtype, s[0]
            assert np.array_equal(a, b) if a.dtype != np.float32 else U.same_bits(a, b), (s[0], s[2])
