"""No GPU: the problems of tests/egrad_key_cases.py are what they claim.  For every case and both of its steps: the keys fill
the B (z + 1) slots and are the stated plan; the events the case produces are found from its keys, the constant 16 and the
stated plan alone, and between them the cases produce every event of K.EVENTS; the float32 oracle's dR_e sits within
U.ROW_TOL64 of the float64 oracle's row by row (the condition that makes the GPU bound meaningful: the reference alone meets
it), and no present row's norm is below the floor of U.row_err, which would otherwise hide it."""
import numpy as np
import pytest

from tests import egrad_key_cases as K
from tests import util as U

NAMES = list(K.CASES)
ROW_FLOOR = 1e-3        # util.row_err: floor, relative to the median row norm


@pytest.mark.parametrize('name', NAMES)
def test_keys_are_the_stated_plan(name):
    c, p = K.case_problem(name)
    B, z, Ve = c['B'], c['z'], c['Ve']
    assert p['y'].shape == (K.STEPS * B,) and p['X'].shape == (K.STEPS * B, K.N) and p['Re'].shape == (Ve, c['de'])
    moved = []
    for s in range(K.STEPS):
        cand = K.step_keys(name, s)
        assert cand.shape == (B, z + 1) and p['neg'][s].shape == (B, z) and p['neg'][s].dtype == np.int64
        assert cand.min() >= 0 and cand.max() < Ve
        counts = K.step_counts(name, s)
        assert int(counts.sum()) == B * (z + 1)
        if K.is_bucket(name):
            g = c['plan']
            assert g['num_sub'] == -(-B // g['sub_rows']) and g['groups'] == -(-g['num_sub'] // g['subs_per_group'])
            assert g['ranges'] == -(-Ve // K.RANGE) and g['sub_rows'] * (z + 1) <= 4096
            ln = K.bucket_list_lengths(cand, g['sub_rows'], g['ranges'])
            assert ln.shape == (g['num_sub'], g['ranges']) and int(ln.sum()) == B * (z + 1)
            for sg, lists in K.bucket_step_lists(c, s).items():
                for r, k in lists.items():
                    assert ln[sg, r] == k, (name, s, sg, r, int(ln[sg, r]), k)
            moved.append(ln)
        else:
            assert np.array_equal(counts, K.sorted_step_counts(c, s)), (name, s)
            moved.append(counts)
    # step 2 is another plan: runs, lists and absent entities moved
    assert not np.array_equal(K.step_keys(name, 0), K.step_keys(name, 1)), name
    assert c['Ve'] <= K.RANGE or not np.array_equal(moved[0], moved[1]), name      # (one range: its lists cannot move)
    if not K.is_bucket(name):
        assert not np.array_equal(moved[0] == 0, moved[1] == 0), (name, 'the absent entities did not move')


def test_sorted_events_come_from_the_counts_alone():
    """sorted_events on plans small enough to check by eye: chunk = 16."""
    plan = dict(path='sorted', sort_bits=5, passes=1, vec=4, nch=1, fixup='wave')
    ev = K.sorted_events([1, 15, 16, 0, 0, 0, 0, 0, 17, 0], 10, 16, plan)
    # runs [0, 1) [1, 16) [16, 32) [32, 49): 1 in the first slot, 16 aligned, 17 over two chunks; 49 pairs; 5 absent
    assert {'run1_first_slot', 'run15', 'run16_aligned', 'run17', 'absent_stretch_5', 'last_entity_absent', 'total_mod16_nonzero',
            'total_below_tile', 'reduce_4_1', 'fixup_wave_vec4'} == ev
    ev = K.sorted_events([0, 15, 17, 16, 16], 5, 70, dict(plan, vec=1, nch=4, fixup='workgroup'))
    # runs [0, 15) [15, 32) [32, 48) [48, 64): 17 from the last slot, ending at a chunk's end from the chunk before
    assert {'entity0_absent', 'run15', 'run17', 'run17_from_last_slot', 'run_ends_at_chunk_end_from_earlier_chunk', 'run16_aligned',
            'last_entity_present', 'total_mod16_zero', 'total_below_tile', 'reduce_1_4_second_column_pass', 'fixup_wg_vec1'} == ev
    ev = K.sorted_events([0, 0, 15 + 16 * 70, 1, 0], 5, 512, dict(plan, nch=8, fixup='workgroup'))
    # runs [0, 1135) [1135, 1136): 71 chunks, the last of them shared with a run of 1 in its last slot
    assert {'fixup_wg_18_chunks', 'fixup_wg_70_chunks', 'run_over_3_chunks', 'run1_last_slot', 'reduce_4_8_de512', 'fixup_wg_vec4_de512'} <= ev
    assert not ev & {'one_entity_takes_all', 'fixup_wave_70_chunks', 'run_ends_at_chunk_end_from_earlier_chunk'}
    assert 'one_entity_takes_all' in K.sorted_events([0, 0, 40, 0, 0], 5, 16, plan)


def test_every_event_is_produced_by_some_case():
    """The union over all cases and both steps covers K.EVENTS; each kind of case produces only events of its own list."""
    produced = {}
    for name in NAMES:
        own = K.BUCKET_EVENTS if K.is_bucket(name) else K.SORTED_EVENTS
        for s in range(K.STEPS):
            ev = K.events_of(name, s)
            assert ev <= set(own), (name, s, sorted(ev - set(own)))
            for e in ev:
                produced.setdefault(e, []).append((name, s))
    missing = [e for e in K.EVENTS if e not in produced]
    assert not missing, 'events of tests/egrad_key_cases.py: EVENTS that no case produces: %s' % ', '.join(missing)
    # the four plans the dispatch could reach and no test launched: each in a case of its own
    assert ('one_entity_d384', 0) in produced['reduce_4_8_de384'] and ('runs_wg_v4_d512', 0) in produced['reduce_4_8_de512']
    assert ('runs_wave_v1', 0) in produced['fixup_wave_vec1'] and ('runs_wg_v4_d512', 0) in produced['fixup_wg_vec4_de512']
    assert ('deep_groups_d4', 0) in produced['subs_per_group_gt_32']


@pytest.mark.parametrize('name', NAMES)
def test_reference_alone_meets_the_row_bound(name):
    """float32 oracle against float64 oracle, dR_e of both steps: U.row_err over the present entities below U.ROW_TOL64, and
    every present row's norm above the floor of U.row_err as the GPU test applies it (over ALL rows: the median there is the
    median of all V_e row norms)."""
    c, _ = K.case_problem(name)
    g32, _ = K.case_reference(name, np.float32)
    g64, _ = K.case_reference(name, np.float64)
    for s in range(K.STEPS):
        present = np.nonzero(K.step_counts(name, s) > 0)[0]
        err, row = U.row_err(g32[s], g64[s], rows=present)
        norms = np.sqrt((np.asarray(g64[s], np.float64) ** 2).sum(axis=1))
        floor_present = ROW_FLOOR * float(np.median(norms[present]))
        floor_all = ROW_FLOOR * float(np.median(norms))
        low = present[norms[present] <= max(floor_present, floor_all)]
        print('%s step %d: float32 vs float64 oracle row_err %.2e (entity %d), smallest present row norm %.2e, floor %.2e'
              % (name, s, err, row, norms[present].min(), max(floor_present, floor_all)))
        assert err < U.ROW_TOL64, (name, s, err, row)
        assert len(low) == 0, (name, s, 'rows the floor of row_err would hide', low[:10], norms[low[:10]])
        # nothing of either oracle is a NaN or an overflow
        assert np.isfinite(g32[s]).all() and np.isfinite(g64[s]).all()


def test_bucket_geometry_is_what_api_model_derives():
    """The stated geometry of every bucket case is what csrc/host/api_model.inc derives for its shape (restated here: the GPU
    test asserts the reported one), and every bucket case is a shape the bucket path takes; the sorted cases whose shape the
    bucket path would take are the ones the GPU test has to force onto the sort."""
    for name, c in K.BUCKET_CASES.items():
        B, c1, Ve, de = c['B'], c['z'] + 1, c['Ve'], c['de']
        assert Ve <= 2048 and de % 4 == 0 and de <= 128 and c1 <= 4096
        sub_rows = min(256, 4096 // c1)
        while sub_rows > 32 and B < 64 * sub_rows:
            sub_rows //= 2
        num_sub = -(-B // sub_rows)
        spg = max(1, ((2 << 20) // (de * 4)) // sub_rows)
        spg = max(1, min(spg, num_sub // 16))
        want = dict(path='bucket', sub_rows=sub_rows, num_sub=num_sub, subs_per_group=spg, groups=-(-num_sub // spg),
                    ranges=-(-Ve // 16), group_sum=False)
        assert c['plan'] == want, (name, c['plan'], want)
    for name, c in K.CASES.items():
        plan = c['sorted_plan'] if K.is_bucket(name) else c['plan']
        Ve, de = c['Ve'], c['de']
        bits = max(1, int(np.ceil(np.log2(Ve))))
        passes = -(-bits // 11)
        vec = 4 if de % 4 == 0 else 1
        nch = 4 if vec == 1 else next(k for k in (1, 2, 5, 8) if -(-(de // 4) // 16) <= k)
        want = dict(path='sorted', sort_bits=bits, passes=passes, vec=vec, nch=nch,
                    fixup='workgroup' if Ve < 256 and de <= 512 else 'wave')
        assert plan == want, (name, plan, want)
