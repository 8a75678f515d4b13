"""The input conditions of tests/test_gpu_score_bf16_bound.py, proven without a GPU: a NumPy model of the scorer's
round-to-nearest-even bf16 (the one of tests/test_golden_host.py) and float64 products of the fp32-normalised rows
(tests/score_bf16_cases.py `model`) show, for every case and every query, that the tables sit where the device-side
margins of csrc/kernels_score_bf16.h decide: the reversed entities between 1.08 delta and 2 delta below s^_(k), the sampled
threshold among the decoys, and nothing else -- candidate count, group overflow, a missing gap on a `cut` row -- that
could send a row to the fallback instead.  delta is bf16_delta(d), read from the header."""
import os
import re

import numpy as np
import pytest

from tests import score_bf16_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTINGS = [(name, i) for name, (_, pl) in B.CASES.items() for i in range(len(pl))]
CUT = [(n, i) for n, i in PLANTINGS if B.CASES[n][1][i][0] == 'cut']
FLAG = [(n, i) for n, i in PLANTINGS if B.CASES[n][1][i][0] == 'flag']


def test_delta_is_the_formula_of_the_header():
    src = open(os.path.join(ROOT, 'sert_amd', 'csrc', 'kernels_score_bf16.h')).read()
    m = re.search(r'float bf16_delta\(int d\) \{ return ([0-9.e-]+)f \+ ([0-9.e-]+)f \* \(float\)d; \}', src)
    assert m, 'bf16_delta has another form: restate it in tests/score_bf16_cases.py'
    assert (float(m.group(1)), float(m.group(2))) == (B.DELTA_CONST, B.DELTA_PER_DIM)
    assert B.delta(64) == float(np.float32(0.00785) + np.float32(1.2e-7) * np.float32(64))
    # the host's other constants the cases restate
    score = open(os.path.join(ROOT, 'sert_amd', 'csrc', 'kernels_score.h')).read()
    assert 'constexpr int kScoreStride = %d;' % B.STRIDE in score
    assert (B.sample_rank(10), B.sample_rank(100), B.cand_cap(10), B.cand_cap(100)) == (27, 38, 1024, 2048)


def _plants(name, planting):
    case = B.build(name)
    return case, case['plant'][B.NUM_ADV * planting:B.NUM_ADV * (planting + 1)]


def _kth(a, n):
    """n-th largest (1-based) of a 1-d array."""
    return float(np.partition(a, len(a) - n)[len(a) - n])


def _sampled_threshold(sh_row, rs):
    """approx_kth_rows on the model's approximate scores: the rs-th largest of the 256 per-thread maxima; a thread reads
    float4 pieces tid, tid + 256, ... of the 2048 sampled scores."""
    samp = sh_row[::B.STRIDE]
    assert samp.size == 2048
    return _kth(samp.reshape(-1, 256, 4).max(axis=(0, 2)), rs)


def _unflagged_facts(name, row, k, own=()):
    """What keeps row `row` of the case's model on the fused path for reasons OTHER than the margins under test: with T
    anywhere between the (rs - 7)-th and the (rs + 13)-th largest sampled score (k = 10: the 20th and the 40th; the model's
    approx_kth_rows lies between them), between k and ccap candidates, no list beyond its capacity, and the 2 delta gap
    between s^_(k) and T with 1e-3 to spare.  Returns (s^_(k), T of the model)."""
    s, sh = B.model(name)
    d = B.CASES[name][0]
    rs = B.sample_rank(k)
    samp = sh[row, ::B.STRIDE]
    t_hi, t_lo = _kth(samp, rs - 7), _kth(samp, rs + 13)
    t = _sampled_threshold(sh[row], rs)
    assert t_lo <= t <= t_hi, (name, row, t_lo, t, t_hi)
    n_hi, n_lo = int((sh[row] >= t_hi).sum()), int((sh[row] >= t_lo).sum())
    assert k <= n_hi <= n_lo <= B.cand_cap(k), (name, row, n_hi, n_lo)
    per_group = (sh[row] >= t_lo).reshape(-1, B.GROUP).sum(axis=1)
    assert per_group.max() <= B.group_cap(k), (name, row, per_group.max())
    sk = _kth(sh[row], k)
    assert sk - t_hi >= 2 * B.delta(d) + 1e-3, (name, row, sk, t_hi)
    return sk, t


@pytest.mark.parametrize('name', list(B.CASES))
def test_rounding_stays_put(name):
    """After fp32 normalisation every component of an adversarial query, and every component of a planted row that meets a
    non-zero of its query (F_e meets a zero), is at least 2^-14 (relative) from a bf16 rounding midpoint, and the bf16
    image is the same 4 fp32 ulp either way -- whatever order l2_normalize_rows sums in."""
    case = B.build(name)
    sup = case['layout'].support
    En, Pn = B.normalize32(case['E']), B.normalize32(case['P_adv'])
    for pl in case['plant']:
        for X in (Pn[pl['query']][None, sup], En[pl['index']][:, sup]):
            assert np.all((X != 0).sum(axis=1) >= len(B.PATTERN))
            assert B.midpoint_distance(X).min() >= 2.0 ** -14
            bits = np.ascontiguousarray(X).view(np.int32)
            for off in (-4, 4):       # (a zero stays a zero)
                assert np.array_equal(B.bf16(np.where(X != 0, bits + off, bits).view(np.float32)), B.bf16(X))
        # the pattern rounds the way it is meant to: down on A, up on B
        lay = case['layout']
        q = Pn[pl['query']]
        assert np.all(np.abs(B.bf16(q[lay.A])) < np.abs(q[lay.A])) and np.all(np.abs(B.bf16(q[lay.B])) > np.abs(q[lay.B]))


@pytest.mark.parametrize('name', list(B.CASES))
def test_error_within_the_bound_and_close_to_it(name):
    """No |s^ - s| of the table exceeds delta, for any query; every planted entity is beyond 0.6 delta (a Gaussian table:
    0.05 delta), a down entity and an up decoy together 1.2 delta apart."""
    case = B.build(name)
    s, sh = B.model(name)
    dlt = B.delta(case['d'])
    assert np.isfinite(s).all() and np.isfinite(sh).all()
    assert np.abs(sh - s).max() <= dlt
    for pl in case['plant']:
        q, k = pl['query'], pl['k']
        err = (sh - s)[q]
        assert err[pl['top']].max() <= -0.6 * dlt and err[pl['decoys'][:k]].min() >= 0.6 * dlt
        assert err[pl['decoys']].min() >= 0.59 * dlt          # (the short decoys of `flag` lack one dimension)
    print(name, 'max |err| / delta %.4f' % (np.abs(sh - s).max() / dlt))


@pytest.mark.parametrize('name,planting', CUT)
def test_cut_rows_decide_at_the_two_delta_cut(name, planting):
    case, plants = _plants(name, planting)
    s, sh = B.model(name)
    dlt = B.delta(case['d'])
    every = np.concatenate([pl['index'] for pl in case['plant'] if pl['kind'] == 'cut'])
    assert np.all(every % B.STRIDE == 1)            # the sample of a `cut` planting holds background rows only
    for pl in plants:
        q, k = pl['query'], pl['k']
        assert len(pl['top']) == k and len(pl['decoys']) == 2 * k
        sk, t = _unflagged_facts(name, q, k)
        # deficits: every down entity between 1.08 delta and 2 delta - 1e-4 below the k-th largest approximate score
        deficit = sk - sh[q, pl['top']]
        assert B.FLOOR * dlt <= deficit.min() and deficit.max() <= 2 * dlt - 1e-4, (deficit.min() / dlt, deficit.max() / dlt)
        # the two top-k sets: disjoint; the exact one is the planted set in its order, neighbours (the k+1-th included)
        # at least STEP_FLOOR apart; the approximate one holds decoys only
        exact = np.argsort(-s[q], kind='stable')[:k + 1]
        assert np.array_equal(exact[:k], pl['top'])
        assert np.diff(-s[q, exact]).min() >= B.STEP_FLOOR[k]
        approx = np.argsort(-sh[q], kind='stable')[:k]
        assert set(approx.tolist()) <= set(pl['decoys'].tolist()) and not set(approx.tolist()) & set(exact[:k].tolist())
        assert sh[q, pl['decoys']].min() > sh[q, pl['top']].max()
        # background (every row not planted for this query, other queries' planted rows included): at least 0.1 below
        # the cut, so it is the planted rows alone that the cut decides about
        other = np.ones(B.V, dtype=bool)
        other[pl['index']] = False
        assert sh[q, other].max() <= sk - 2 * dlt - 0.1, (sh[q, other].max(), sk)
        # at most 2 planted entities of one query share a 64-entity group (here: none do)
        assert np.bincount(pl['index'] // B.GROUP).max() <= 2
        print(name, 'query', q, 'k', k, 'deficits %.3f .. %.3f delta' % (deficit.min() / dlt, deficit.max() / dlt),
              'T %.3f s^_(k) %.4f' % (t, sk))


@pytest.mark.parametrize('name,planting', FLAG)
def test_flag_rows_decide_at_the_gap_flag(name, planting):
    case, plants = _plants(name, planting)
    s, sh = B.model(name)
    dlt = B.delta(case['d'])
    for pl in plants:
        q, k = pl['query'], pl['k']
        rs = B.sample_rank(k)
        sampled, hidden, decoys = pl['sampled'], pl['top'], pl['decoys']
        assert len(sampled) >= 2 * rs and np.all(sampled % B.STRIDE == 0) and np.all(hidden % B.STRIDE == 1)
        pos = sampled // B.STRIDE
        # different threads of approx_kth_rows, sample positions distinct mod 256, different 64-entity groups
        assert len(set(((pos >> 2) & 255).tolist())) == len(pos) == len(set((pos % 256).tolist()))
        assert np.bincount(pl['index'] // B.GROUP).max() == 1
        # every hidden entity is below every decoy in bf16 and above every decoy exactly, in a known order
        assert sh[q, hidden].max() <= sh[q, decoys].min() - 0.9 * B.FLAG_MARGIN
        exact = np.argsort(-s[q], kind='stable')[:k + 1]
        assert np.array_equal(exact[:k], hidden) and np.diff(-s[q, exact]).min() >= B.STEP_FLOOR[k]
        # the sampled threshold is a sampled decoy's score: the (rs + 8)-th largest sampled score still is one
        samp = sh[q, ::B.STRIDE]
        lo, hi = sh[q, sampled].min(), sh[q, sampled].max()
        assert _kth(samp, rs + 8) >= lo and _kth(samp, 1) == hi
        t = _sampled_threshold(sh[q], rs)
        assert lo <= t <= hi
        # the row must be flagged: no 2 delta between s^_(k) and any possible threshold ...
        sk = _kth(sh[q], k)
        assert sk - lo < 2 * dlt - 1e-4
        # ... and only the second delta says so: s^_(k) - delta is above every possible threshold
        assert sk - dlt >= hi + 0.9 * B.FLAG_MARGIN
        # nothing else flags it: between k and ccap candidates, no group beyond its list
        n = int((sh[q] >= lo).sum())
        assert k <= n == len(decoys) <= B.cand_cap(k)
        # the approximate top k: the unsampled decoys; background at least 0.1 below every planted score
        assert set(np.argsort(-sh[q], kind='stable')[:k].tolist()) == set(decoys[:k].tolist())
        other = np.ones(B.V, dtype=bool)
        other[pl['index']] = False
        assert sh[q, other].max() <= sh[q, pl['index']].min() - 0.1
        print(name, 'query', q, '(s^_(k) - T) / delta in [%.3f, %.3f]' % ((sk - hi) / dlt, (sk - lo) / dlt),
              'hidden below T by %.1e' % (lo - sh[q, hidden].max()))


@pytest.mark.parametrize('name', list(B.CASES))
def test_ordinary_rows_stay_fused_and_meet_the_oracle_check(name):
    """The tanh(randn) queries of every call: finite scores, k distinct entities to report, and on the fused path for every
    k their call uses -- so counts[3] of a `cut` call counts adversarial rows only."""
    case = B.build(name)
    s, sh = B.model(name)
    n_adv = len(case['plant'])
    assert s.shape == (n_adv + B.NUM_ORDINARY, B.V)
    for k in sorted(set(pl['k'] for pl in case['plant'])):
        for row in range(n_adv, n_adv + B.NUM_ORDINARY):
            _unflagged_facts(name, row, k)
            assert np.isfinite(s[row]).all() and len(np.unique(s[row])) > k
