"""No GPU: the problems of tests/wgrad_cases.py are what they claim.  For every case and both of its steps: the tokens are the
stated counts; the index the engine would upload (sert_debug_word_index_sum walks the real build_word_index output on the host)
has the levels, level-0 items, partial rows, dense words and fused upper levels the stated plan implies, and the stated plan is
what the dispatch of csrc/host/lazy_segsum.inc, restated in K.plan_from_dispatch, makes of the counts; between them the cases
produce every event of K.EVENTS; the float32 oracle's word gradient sits within U.ROW_TOL64 of the float64 oracle's row by row
over the touched rows (the condition that makes the GPU bound meaningful: the reference alone meets it), and no touched row's
norm is below the floor of U.row_err, which would otherwise hide it."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import util as U
from tests import wgrad_cases as K

NAMES = list(K.CASES)
ROW_FLOOR = 1e-3        # util.row_err: floor, relative to the median row norm


@pytest.mark.parametrize('name', NAMES)
def test_tokens_are_the_stated_counts(name):
    c, p = K.case_problem(name)
    B, n, Vw = c['B'], c['n'], c['Vw']
    assert p['X'].shape == (K.STEPS * B, n) and p['X'].dtype == U.id_dtype(Vw) and p['Rw'].shape[0] == Vw
    counts = [K.step_counts(name, s) for s in range(K.STEPS)]
    for s in range(K.STEPS):
        assert int(counts[s].sum()) == B * n
        assert np.array_equal(counts[s], K.stated_counts(c, s)), (name, s)
        for count, k in c['counts'][s][0]:
            assert int((counts[s] == count).sum()) >= k, (name, s, count, k)
        # step 2 is another plan: a word of more than one item in this step is absent or a singleton in the other
        multi = np.nonzero(counts[s] > K.SEG)[0]
        assert len(multi) > 0 or counts[1 - s].max() > K.SEG, (name, s)
        assert counts[1 - s][multi].max(initial=0) <= 1, (name, s, multi[:5], counts[1 - s][multi][:5])
    assert c['plan'][0] != c['plan'][1], name
    # word 0 and the last word: each present in one step and absent in the other
    assert (counts[0][0] > 0) != (counts[1][0] > 0) and (counts[0][-1] > 0) != (counts[1][-1] > 0), name
    if c.get('full_row'):
        X = K.step_tokens(name, 0)
        assert np.all(X[0] == X[0, 0]) and counts[0][X[0, 0]] > K.HEAVY_MIN and n >= 2


@pytest.mark.parametrize('name', NAMES)
def test_index_and_dispatch_give_the_stated_plan(name):
    c, _ = K.case_problem(name)
    B, n, Vw = c['B'], c['n'], c['Vw']
    for s in range(K.STEPS):
        plan = c['plan'][s]
        counts = K.step_counts(name, s)
        assert K.plan_from_dispatch(c, counts) == plan, (name, s, K.plan_from_dispatch(c, counts), plan)
        ids = np.ascontiguousarray(K.step_tokens(name, s)).reshape(1, B, n)
        src = np.ones((B, 1), dtype=np.float32)
        if K.is_ll(name):
            # (the loglinear index keeps its dense words in the tree, flagged: the tree of all the words)
            got, st = C.debug_word_index_sum(ids, Vw, src, dense_heavy=False)
            dense, tree = K.dense_words(counts, B * n, c['Ve'] % 4 == 0), counts
        else:
            got, st = C.debug_word_index_sum(ids, Vw, src, dense_heavy=K.dense_enabled(c), sort_level0=True)
            dense = K.dense_words(counts, B * n, K.dense_enabled(c))
            tree = counts.copy()
            tree[dense] = 0
            assert st['dense_words'] == plan['dense_cnt'], (name, s, st)
        levels, items, most = K.tree_shape(tree)
        assert len(dense) == plan['dense_cnt'] and levels == plan['levels'], (name, s, dense, levels)
        assert st['levels'] == plan['levels'] and st['level0_items'] == items[0] and st['items'] == sum(items), (name, s, st, items)
        assert st['partial_rows'] == sum(items[l] - int((np.asarray(_lens(tree, l)) <= K.SEG).sum()) for l in range(levels)), (name, s, st)
        assert st['level1_items'] == (items[1] if levels > 1 else 0), (name, s, st)
        assert st['distinct_words'] == int((counts > 0).sum())
        # levels 1 and 2 as one launch: three levels and no word above 32 level-1 chunk items
        assert bool(st['fused_upper_ok']) == (levels == 3 and most <= K.FUSED_MAX), (name, s, st, most)
        forms = [f for f, _ in plan['launches']]
        if not K.is_ll(name) and c['dw'] % 4 == 0:
            assert ('upper_fused' in forms) == bool(st['fused_upper_ok']), (name, s, forms, st)
        if levels == 3:
            assert st['heavy_cnt'] == int((tree > K.SEG * K.SEG).sum()), (name, s, st)
        # with src = 1 the walked index returns every word's count (vectorspace entries are batch rows: any row is 1)
        assert np.array_equal(got[:, 0], counts.astype(np.float32)), (name, s)


def _lens(tree, level):
    """entry counts of the items' words at `level` (a word's level-l input length)."""
    lens = [int(k) for k in tree if k > 0]
    for _ in range(level):
        lens = [-(-k // K.SEG) for k in lens if k > K.SEG]
    return lens


def test_tree_shape_and_dense_words_by_eye():
    """K.tree_shape / K.dense_words / K.heavy_rows on counts small enough to check by eye."""
    assert K.tree_shape([1, 64, 0, 3]) == (1, [3], 0)
    assert K.tree_shape([65, 1]) == (2, [3, 1], 0)                       # chunks of 64 and 1, then one item of 2
    assert K.tree_shape([4096]) == (2, [64, 1], 0)
    assert K.tree_shape([4097, 2]) == (3, [66, 2, 1], 2)                 # 65 chunks; 65 entries: 2 chunk items; one of 2
    assert K.tree_shape([131072]) == (3, [2048, 32, 1], 32)
    assert K.tree_shape([131073]) == (3, [2049, 33, 1], 33)
    assert K.tree_shape([262144]) == (3, [4096, 64, 1], 64)
    assert K.tree_shape([262145])[0] == 4
    assert K.dense_words([4096, 10], 4106) == [] and K.dense_words([4097, 10], 4107) == [0]
    assert K.dense_words([4097, 10], 8 * 4097 + 1) == [] and K.dense_words([10, 4097, 4097], 8 * 8194) == [1, 2]
    c = np.full(20, 5000)
    c[3] = 4097
    assert 3 not in K.dense_words(c, 100000) and len(K.dense_words(c, 100000)) == 16 and K.dense_words(c, 100000)[0] == 0
    assert [K.heavy_rows(B) for B in (64, 32767, 32768, 32808, 65535, 65536, 1 << 20)] == [64, 64, 128, 128, 128, 256, 256]


def test_every_event_is_produced_by_some_case():
    """The union over all cases and both steps covers K.EVENTS; each kind of case produces only events of its own list."""
    produced = {}
    for name in NAMES:
        own = K.LL_EVENTS if K.is_ll(name) else K.VS_EVENTS
        for s in range(K.STEPS):
            ev = K.events_of(name, s)
            assert ev <= set(own), (name, s, sorted(ev - set(own)))
            for e in ev:
                produced.setdefault(e, []).append((name, s))
    missing = [e for e in K.EVENTS if e not in produced]
    assert not missing, 'tests/wgrad_cases.py: EVENTS that no case produces: %s' % ', '.join(missing)
    # the forms no other test launches, each in the case that is there for it
    assert ('four_levels_d132', 0) in produced['tree_4_levels'] and ('upper_bounds_d8', 1) in produced['level2_launch_33_chunk_items']
    assert ('upper_bounds_d8', 0) in produced['upper_fused_32_chunk_items'] and ('rows128_d4', 0) in produced['heavy_rows128']
    assert ('w_d200_dense', 0) in produced['dw200_two_launches'] and ('lens_d256_dense', 1) in produced['dw256_two_launches']
    assert ('w_d70', 0) in produced['dw70_scalar_upper_levels'] and ('rows256_d8', 1) in produced['heavy17_lightest_in_tree_combine_alone']
    assert ('rows256_d8', 0) in produced['row_of_one_dense_word'] and ('ll_v75', 1) in produced['ll_scalar_count4097']


@pytest.mark.parametrize('name', NAMES)
def test_reference_alone_meets_the_row_bound(name):
    """float32 oracle against float64 oracle, dR_w of both steps: U.row_err over the touched rows below U.ROW_TOL64, and every
    touched row's norm above the floor of U.row_err as the GPU test applies it.

    Measured (float32 against float64 oracle, worst touched row over both steps; the bound is 5e-5): four_levels_d132 2.1e-5,
    upper_bounds_d8 1.7e-5 -- the float32 oracle adds a word's occurrences one after the other -- and at most 2.3e-6 for every
    other case; the smallest touched row is 29 (rows128_d4, step 1) to 360 times above the floor."""
    g32, _ = K.case_reference(name, np.float32)
    g64, _ = K.case_reference(name, np.float64)
    for s in range(K.STEPS):
        a32, a64 = K.word_grad(name, g32[s]), K.word_grad(name, g64[s])
        counts = K.step_counts(name, s)
        touched = np.nonzero(counts > 0)[0]
        err, row = U.row_err(a32, a64, rows=touched)
        norms = np.sqrt((np.asarray(a64, np.float64) ** 2).sum(axis=1))
        floor = ROW_FLOOR * float(np.median(norms[touched]))
        low = touched[norms[touched] <= floor]
        print('%s step %d: float32 vs float64 oracle row_err %.2e (word %d, %d occurrences), smallest touched row norm %.2e, floor %.2e'
              % (name, s, err, row, counts[row], norms[touched].min(), floor))
        assert err < U.ROW_TOL64, (name, s, err, 'word', row, 'occurrences', int(counts[row]))
        assert len(low) == 0, (name, s, 'rows the floor of row_err would hide', low[:10], norms[low[:10]])
        assert np.isfinite(a32).all() and np.isfinite(a64).all()


@pytest.mark.parametrize('name', NAMES)
def test_reference_state_alone_meets_the_bounds(name):
    """The float32 oracle's parameters and moments after both steps against the float64 oracle's, through U.check_state -- the
    bounds the keep_grads = 0 GPU test applies to the engine (worst row against float64: four_levels_d132 4.6e-5 of 1e-4 on a
    second moment, upper_bounds_d8 3.4e-5, every other case at most 1.6e-5)."""
    _, o32 = K.case_reference(name, np.float32)
    _, o64 = K.case_reference(name, np.float64)
    s32 = U.oracle_state(o32)
    print('%s: %s' % (name, '; '.join(U.check_state(s32, s32, U.oracle_state(o64)))))
