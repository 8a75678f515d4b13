"""No GPU: the inputs of test_gpu_big_offsets.py do what that test needs of them (tests/big_offset_cases.py).

1. every shape takes the route its row names, `under` below its guard and `at` at or above it;
2. the pool construction separates the lines a wrong offset would confuse;
3. a kernel with either failure mode -- lines past a mark read as zero, lines read at their offset modulo the mark -- would
   miss the case's bound a hundredfold;
4. the tiling identity of the loglinear cases holds on the oracle."""
import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import big_offset_cases as G

FORMS = {'plain': C.GEMM_FORM_PLAIN, 'splitk': C.GEMM_FORM_SPLITK, 'longk': C.GEMM_FORM_LONGK}


def test_every_shape_is_on_its_side_of_the_guard_and_takes_its_route(hip_lib, monkeypatch):
    monkeypatch.delenv('SERT_GEMM_FP32', raising=False)
    wrong = {}
    for name, row in G.GEMM_ROWS.items():
        under, lim = G.guarded_extent(row, 'under')
        at, _ = G.guarded_extent(row, 'at')
        assert under < lim <= at, (name, under, at, lim)
        for side, want in zip(G.SIDES, row['routes']):
            M, N, K = row[side]
            got = C.debug_gemm_route(FORMS[row['hook']], M, N, K, tb=row['tb'], splits=row['splits'])
            if got != want:
                wrong[(name, side)] = (got, want)
    assert not wrong, wrong
    # every x3 kernel form has a case under its guard; the loaders of the fp32 kernels change at LD_GUARD, not their route
    assert {r['routes'][0] for r in G.GEMM_ROWS.values()} >= set(C.GEMM_ROUTES) - {'f32_tile64', 'f32_tile128x160'}
    # the logits GEMM of the loglinear cases (G (U, d) . W (d, V_e)): gemm_x3.h, whose guards see A and B but not the output
    for name, case in G.LL_TRAIN.items():
        U = case['P'] * case['c'] * case['n']
        assert C.debug_gemm_route(C.GEMM_FORM_PLAIN, U, case['Ve'], G.D) == 'x3_256', name


@pytest.mark.parametrize('name', [n for n, r in G.GEMM_ROWS.items() if r['build'] != 'k_plain'])
def test_pool_separates_the_lines_a_wrong_offset_would_confuse(name):
    """A condition on the inputs: at most 1 % of the lines have the (h, e) of the line a mark or a tile away."""
    row = G.GEMM_ROWS[name]
    count = G.lines_of(row, 'at')
    h, e = G.hash_lines(count, along_k=row['build'] == 'k_rows')
    assert h.min() == 0 and h.max() == G.POOL - 1 and e.min() == -4 and e.max() == (0 if row['build'] == 'k_rows' else 4)
    key = h * 16 + e
    for dist in G.line_distances(row):
        assert 0 < dist < count, (name, dist)
        same = float(np.mean(key[dist:] == key[:-dist]))
        assert same <= 0.01, (name, dist, same)


def test_tile_period_does_not_divide_the_distance_of_a_mark():
    """Loglinear cases: the table rows 2^31 and 2^32 bytes apart are different rows of the small problem (or the mark falls
    inside a row: V_e 4 bytes do not divide it), and every case's table lies between the marks it names."""
    for name, case in list(G.LL_TRAIN.items()) + list(G.LL_EVAL.items()):
        period, row_bytes = case['P'] * case['n'], case['Ve'] * 4
        assert case['P'] % 2 == 1 or name in G.LL_EVAL
        for mark in (G.MARK31, G.MARK32):
            assert mark % row_bytes != 0 or (mark // row_bytes) % period != 0, (name, mark)
        assert G.table_bytes(case) >= case['above'] and (case['below'] is None or G.table_bytes(case) < case['below']), name
    assert (G.MARK31 // (G.VE * 4)) % 2520 == 64 and (G.MARK32 // (G.VE * 4)) % 4032 == 128
    # the form a batch takes (ll_forward, host/step_softmax_loglinear.inc), restated: the distinct-word row kernels while
    # the row's slab would fit the fused kernel's LDS, ll_row_wave while the table is below 2^32 bytes
    for name, case in G.LL_TRAIN.items():
        fused = (case['n'] + 1) * case['Ve'] * 4 <= 150 * 1024
        wave = fused and case['Ve'] % 4 == 0 and case['Ve'] <= 2048 and G.table_bytes(case) < G.MARK32
        want = ('wave', 8) if wave else ('table', 128) if fused else ('stream', 1)
        assert case['form'] == want, (name, want)


def _line_maxima(diff, axis):
    return np.abs(diff).max(axis=axis)


@pytest.mark.parametrize('name', [n for n, r in G.GEMM_ROWS.items() if r['build'] != 'k_plain'])
def test_a_wrong_kernel_would_fail(name):
    """Both failure modes in NumPy, on the pool's float64 product (the reference of every line, at no cost: nothing of
    2 GiB is built).  The mark: half the axis -- where it would lie were a guard off by a factor of two -- and 2^31 bytes
    where that falls inside the operand (in most rows it is the operand's very end: they are the smallest shapes AT the
    guard).  Lines past the mark read as zero, or read the line that far back: at least 99 % of them then differ from the
    true product by 100 times the bound (all that a hash into 256 lines can promise; test 2), in the unscaled values the
    GPU test compares.  Pool along k: the sums over k themselves differ that much."""
    row = G.GEMM_ROWS[name]
    ops = G.GemmOperands(name, small_only=True)
    tol = 100 * G.bound(row, 'at')
    count = G.lines_of(row, 'at')
    marks = {count // 2} | {d for d in G.line_distances(row) if d > 320}
    for mark in marks:
        if row['build'] == 'k_rows':
            true, cs = ops.k_rows_reference('at')
            zero, zero_b = ops.scale.copy(), ops.scale_b.copy()
            zero[mark:] = zero_b[mark:] = 0
            wrap = lambda a: np.concatenate([a[:mark], a[:count - mark]])
            for bad, bad_cs in (ops.k_rows_reference('at', scale=zero, scale_b=zero_b),
                                ops.k_rows_reference('at', h=wrap(ops.h), scale=wrap(ops.scale), scale_b=wrap(ops.scale_b))):
                assert np.abs(bad - true).max() >= tol and np.abs(bad_cs - cs).max() >= tol, (name, mark)
            continue
        axis = 1 if row['build'] == 'a_rows' else 0
        pp = ops.pool_product if axis == 1 else ops.pool_product.T          # (POOL, other axis)
        past = np.arange(mark, count)
        past = past[::max(1, len(past) // 16384)]                           # (an even sample: 16 384 lines or more)
        true = pp[ops.h[past]]
        assert np.mean(_line_maxima(true, 1) >= tol) >= 0.99, (name, mark, 'zero')
        back = past - mark
        ratio = (ops.scale[back].astype(np.float64) / ops.scale[past])[:, None]
        assert np.mean(_line_maxima(pp[ops.h[back]] * ratio - true, 1) >= tol) >= 0.99, (name, mark, 'wrap')


@pytest.mark.parametrize('name', list(G.LL_TRAIN))
def test_tiling_identity_of_a_training_step(name):
    """On the oracle alone, V_e = 64, c = 4: loss, dW, db of the tiled problem are the small problem's and
    dR_w[u] = (P / B) dR_small[u mod P n], to 1e-6 (float64)."""
    small = G.ll_small_problem(name, Ve=64)
    big = G.ll_tiled(small, 4)
    P, n, B = small['P'], small['n'], big['B']
    assert B == 4 * P and big['X'].max() == B * n - 1 and len(np.unique(big['X'])) == B * n
    lo, go, _ = O.LogLinearOracle(P, n, small['Rw'], small['W'], small['b'], 0.0, dtype=np.float64).loss_and_grads(
        small['X'], small['y'], small['w'])
    lb, gb, _ = O.LogLinearOracle(B, n, big['Rw'], big['W'], big['b'], 0.0, dtype=np.float64).loss_and_grads(
        big['X'], big['y'], big['w'])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    assert abs(lb - lo) <= 1e-6 * abs(lo)
    assert rel(gb[1], go[1]) < 1e-6 and rel(gb[2], go[2]) < 1e-6
    assert rel(gb[0], np.tile(go[0], (4, 1)) * (P / float(B))) < 1e-6
    assert np.abs(go[0]).max() > 0


@pytest.mark.parametrize('name', list(G.LL_EVAL))
def test_tiling_identity_of_an_evaluation(name):
    small = G.ll_small_problem(name, Ve=64)
    big = G.ll_tiled(small, 4, distinct=False)
    P, n = small['P'], small['n']
    fo = O.LogLinearOracle(P, n, small['Rw'], small['W'], small['b'], 0.0, dtype=np.float64)
    fb = O.LogLinearOracle(4 * P, n, big['Rw'], big['W'], big['b'], 0.0, dtype=np.float64)
    assert abs(fb.eval_loss(big['X'], big['y']) - fo.eval_loss(small['X'], small['y'])) <= 1e-6 * abs(fo.eval_loss(small['X'], small['y']))
    assert np.allclose(fb.forward(big['X'], big['y'])['loss'], np.tile(fo.forward(small['X'], small['y'])['loss'], 4), rtol=1e-12)


@pytest.mark.parametrize('name', list(G.LL_TRAIN) + list(G.LL_EVAL))
def test_no_probability_near_a_clip_bound(name):
    """Engine and oracle must not differ by an fp32 mask decision: every P and Q of the small problem at its full V_e is
    an order of magnitude inside (1e-7, 1 - 1e-7), and two rows' losses differ by far more than the loss tolerance."""
    _, ref = G.ll_reference(name)
    r = ref['float64']
    assert r['P3min'] > 1e-6 and r['P3max'] < 0.9 and r['Q'].min() > 1e-6 and r['Q'].max() < 0.9
    loss = np.sort(r['rowloss'])
    assert np.median(np.diff(loss)) > 1e-4 * loss.mean()
