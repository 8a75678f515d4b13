"""No GPU: the problems of tests/foldin_key_cases.py are what they claim, and the bounds of tests/test_gpu_foldin_keys.py can
tell a wrong fold-in step from a right one.

  1. Inputs: the built y and negatives give exactly the stated counts, every positive is on a new row, sorted the sentinel run
     is the end of the order, step 2 is another plan than step 1; the union of events_of over the cases is K.EVENTS; every
     case's stated plan follows from its shape by the dispatch rules of csrc/host/api_foldin.inc, restated here.
  2. Numerics: the float32 twin alone is within U.ROW_TOL64 (twice that for v) of the float64 twin on every tensor the GPU test
     checks, no present row is small enough for the floor of U.row_err to hide it, and no score or unit is near a clip bound.
  3. Teeth: K.ChunkedGradient, a chunk-by-chunk restatement of the reduce and the fix-up, reproduces the oracle's gradient;
     made wrong on purpose -- one head carry, one tail carry, the second column pass, the last live pair, the sentinel run added
     into row 0, stale run bounds, the second upload slab shifted by a row -- it misses the GPU test's bound by a factor of 10
     or more on the case that exists for it."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import foldin_key_cases as K
from tests import util as U

NAMES = list(K.CASES)
ROW_FLOOR = 1e-3        # util.row_err: floor, relative to the median row norm
# the checks of one step of the GPU test: (tensor, multiple of the row bounds)
CHECKED = {0: (('m', 1), ('v', 2)), 1: (('E', 1), ('m', 1), ('v', 2))}


def _counts(name, s):
    c = K.case_problem(name)
    counts = np.bincount(K.step_keys(name, s), minlength=c['N'] + 1)
    return counts[:c['N']], int(counts[c['N']])


@pytest.mark.parametrize('name', NAMES)
def test_keys_are_the_stated_counts(name):
    c = K.case_problem(name)
    B, z, N = c['B'], c['z'], c['N']
    total = B * (z + 1)
    assert c['X'].shape == (c['M'], K.NWIN) and c['y'].shape == (c['M'],) and c['E0'].shape == (N, c['de'])
    assert 0 <= c['y'].min() and c['y'].max() < N and c['M'] % B != 0 and len(c['batches']) == K.STEPS
    seen = []
    for s, b in enumerate(c['batches']):
        assert (b + 1) * B <= c['M']
        neg = c['neg'][s]
        assert neg.shape == (B, z) and neg.dtype == np.int64 and neg.min() >= 0 and neg.max() < K.VE + N
        want, want_sent = K.step_counts(c, s)
        live, sent = _counts(name, s)
        assert np.array_equal(live, want) and sent == want_sent, (name, s)
        L = int(live.sum())
        assert L + sent == total and B <= L <= total
        # a row's count is at least its number of positives
        assert np.all(live >= np.bincount(c['y'][b * B:(b + 1) * B], minlength=N))
        # sorted (the sort is stable), the sentinel run is the end of the order
        sk = np.sort(K.step_keys(name, s), kind='stable')
        assert np.all(sk[:L] < N) and np.all(sk[L:] == N)
        seen.append((live, sent))
    # step 2 is another plan: the runs moved and the sentinel run starts elsewhere
    assert seen[0][1] != seen[1][1] and (N == 1 or not np.array_equal(seen[0][0], seen[1][0])), name
    if N > 5 and (seen[0][0] == 0).any():
        assert not np.array_equal(seen[0][0] == 0, seen[1][0] == 0), (name, 'the absent rows did not move')


def test_events_come_from_the_counts_alone():
    """key_events on plans small enough to check by eye: chunk = 16."""
    plan = K.plan_of('vector', 1, 4, 1, 4, 1, 1, 'workgroup', 1)
    ev = K.key_events([1, 15, 16, 0, 0, 0, 0, 0, 17, 0], 15, 10, 16, plan)
    # runs [0, 1) [1, 16) [16, 32) [32, 49): 1 in the first slot, 16 aligned, 17 over two chunks; the sentinel [49, 64) from
    # slot 1 behind an absent last row
    assert {'run1_first_slot', 'run15', 'run16_aligned', 'run17', 'absent_stretch_5', 'last_row_absent', 'sentinel_in_slot1',
            'last_row_absent_before_sentinel', 'reduce_4_1', 'fixup_wg_vec4', 'N_mod4_nonzero'} == ev
    ev = K.key_events([0, 15, 17, 16, 16 + 32], 1, 5, 70, K.plan_of('scalar', 2, 3, 1, 1, 4, 2, 'workgroup', 1))
    # runs [0, 15) [15, 32) [32, 48) [48, 96): 17 from the last slot, ending at a chunk's end; the last run three chunks to a
    # chunk's end, the sentinel one pair at a chunk start (97 pairs: not the last slot)
    assert {'row0_absent', 'run15', 'run17', 'run17_from_last_slot', 'run_ends_at_chunk_end_from_earlier_chunk', 'run16_aligned',
            'run_over_3_chunks', 'last_row_present', 'sentinel_at_chunk_start', 'reduce_1_4_two_column_passes', 'fixup_wg_vec1',
            'N_mod4_nonzero'} == ev
    ev = K.key_events([0, 0, 15 + 16 * 70, 0, 0], 1, 5, 512, K.plan_of('vector', 8, 3, 1, 4, 8, 1, 'workgroup', 1))
    assert {'fixup_wg_70_chunks', 'run_over_3_chunks', 'sentinel_in_last_slot', 'sentinel_run1_is_last_pair',
            'last_live_run_3_chunks_ends_in_sentinel_chunk', 'reduce_4_8_de512', 'fixup_wg_vec4_de512'} <= ev
    assert not ev & {'one_row_takes_all', 'fixup_wave_70_chunks', 'fixup_wg_6_chunks', 'no_sentinel_total_mod16_zero'}
    ev = K.key_events([0, 0, 40, 0, 0], 0, 5, 16, plan)
    assert {'one_row_takes_all', 'no_sentinel_total_mod16_nonzero'} <= ev


def test_every_event_is_produced_by_some_case():
    produced = {}
    for name in NAMES:
        ev = K.events_of(name)
        assert ev <= set(K.EVENTS), (name, sorted(ev - set(K.EVENTS)))
        for e in ev:
            produced.setdefault(e, []).append(name)
    missing = [e for e in K.EVENTS if e not in produced]
    assert not missing, 'events of tests/foldin_key_cases.py: EVENTS that no case produces: %s' % ', '.join(missing)
    assert len(K.EVENTS) == len(set(K.EVENTS))
    # the cases that exist for one event have it
    for event, name in (('reduce_4_5_de300', 'n256_d300'), ('reduce_4_5_de320', 'runs_wave_d320'), ('reduce_4_8_de384', 'one_row_d384'),
                        ('reduce_4_8_de512', 'runs_wg_v4_d512'), ('reduce_1_4_two_column_passes', 'runs_wave_v1'),
                        ('reduce_1_4_eight_column_passes', 'runs_wg_v1_d510'), ('fixup_wave_vec1', 'runs_wave_v1'),
                        ('fixup_wg_vec1', 'runs_wg_v1_d510'), ('fixup_wg_vec4_de512', 'runs_wg_v4_d512'),
                        ('sentinel_run1_is_last_pair', 'runs_wg_v1_d510'), ('sentinel_longer_than_tile', 'n2048_d8'),
                        ('last_live_run_3_chunks_ends_in_sentinel_chunk', 'runs_wave_d320'), ('sentinel_in_slot1', 'n256_d300'),
                        ('N2048_12bits_2passes', 'n2048_d8'), ('N4_3bits', 'n4_d8'), ('N_17bits_unequal_passes', 'n70000_d8'),
                        ('upload_batch_straddles_slab', 'upload_two_slabs'), ('upload_batch_behind_slab', 'upload_two_slabs')):
        assert name in produced[event], (event, produced[event])
    # every loss-kernel instance of both forms: the vector form with a full last chunk group and with a single float4 in it, the
    # scalar form with one column and with all but one column in its last slice
    des = {}
    for name in K.LOSS_INSTANCE_CASES:
        p = K.CASES[name]['plan']
        des.setdefault((p['loss'], p['k']), set()).add(K.CASES[name]['de'])
    assert sorted(des) == [(f, k) for f in ('scalar', 'vector') for k in range(1, 9)]
    assert {64, 68, 132, 256, 260, 300, 384, 448, 512} == set().union(*(v for (f, _), v in des.items() if f == 'vector'))
    assert {63, 65, 130, 250, 301, 382, 446, 510} == set().union(*(v for (f, _), v in des.items() if f == 'scalar'))
    assert all(K.CASES[n]['B'] == 24 and K.CASES[n]['z'] == 4 for n in K.LOSS_CASES)
    assert K.CASES[K.REPRO_CASE]['plan']['passes'] == 2 and K.CASES[K.REPRO_CASE]['plan']['tiles'] >= 2


@pytest.mark.parametrize('name', NAMES)
def test_stated_plan_is_what_the_dispatch_derives(name):
    """csrc/host/api_foldin.inc (foldin_create, foldin_loss, foldin_grad), restated; the GPU test asserts the reported plan."""
    c = K.case_problem(name)
    B, z, N, de = c['B'], c['z'], c['N'], c['de']
    cdiv = lambda a, b: -(-a // b)
    bits = 1
    while (1 << bits) <= N:           # keys lie in [0, N]: the sentinel is N itself
        bits += 1
    passes = cdiv(bits, K.SORT_MAX_BITS)
    if de % 4 == 0:
        loss, k = 'vector', cdiv(de // 4, 16)
        vec, nch = 4, next(n for n in (1, 2, 5, 8) if k <= n)
    else:
        loss, k = 'scalar', cdiv(de, 64)
        vec, nch = 1, 4
    want = K.plan_of(loss, k, bits, passes, vec, nch, cdiv(de // vec, 16 * nch), 'workgroup' if N < 256 else 'wave',
                     cdiv(B * (z + 1), K.SORT_TILE))
    assert 1 <= k <= 8 and de <= 512 and c['plan'] == want, (name, c['plan'], want)
    if bits == 17:
        width = cdiv(bits, passes)
        assert (width, bits - width) == (9, 8)
    if bits == 12:
        assert cdiv(bits, passes) == 6


def test_upload_cases_take_the_routes_they_claim(hip_lib):
    """The first slab of upload_two_slabs goes to the bf16-pipe GEMM, its second slab and every other case's projection to an
    fp32 kernel -- asked of the launchers' own predicates (sert_debug_gemm_route: host only)."""
    c = K.case_problem('upload_two_slabs')
    assert c['M'] == K.SLAB + 70 and K.SLAB % c['B'] != 0 and c['de'] <= 128
    assert C.debug_gemm_route(C.GEMM_FORM_PLAIN, K.SLAB, c['de'], c['dw']).startswith('x3_')
    assert C.debug_gemm_route(C.GEMM_FORM_PLAIN, c['M'] - K.SLAB, c['de'], c['dw']).startswith('f32_')
    for name in NAMES:
        d = K.case_problem(name)
        if d['M'] < K.SLAB:
            assert C.debug_gemm_route(C.GEMM_FORM_PLAIN, d['M'], d['de'], d['dw']).startswith('f32_'), name
    assert K.case_problem('upload_dw10')['dw'] % 4 != 0 and K.case_problem('upload_w_none')['w_upload'] is None
    assert np.all(K.case_problem('upload_w_none')['w'] == 1)


def test_plan_hook_refuses_bad_arguments(hip_lib):
    """sert_debug_foldin_plan (include/sert_hip_debug.h) touches no device: without a handle it fails with a message, and the
    binding knows the values of its enum by name."""
    import ctypes
    import os
    import re
    v = (ctypes.c_int32 * 10)()
    hip_lib.sert_debug_foldin_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    assert hip_lib.sert_debug_foldin_plan(None, v, 10) != 0
    assert b'bad argument' in hip_lib.sert_last_error()
    src = open(os.path.join(U.ROOT, 'include', 'sert_hip_debug.h')).read()
    assert C.FOLDIN_LOSS_FORMS == ('none', 'vector', 'scalar')
    for k, form in enumerate(C.FOLDIN_LOSS_FORMS):
        assert re.search(r'\bSERT_FOLDIN_LOSS_%s = %d\b' % (form.upper(), k), src), form


def _present(name, s):
    """rows a pair of step 0 .. s hit"""
    c = K.case_problem(name)
    hit = np.zeros(c['N'], bool)
    for k in range(s + 1):
        hit |= _counts(name, k)[0] > 0
    return np.nonzero(hit)[0]


@pytest.mark.parametrize('name,lam', [(n, None) for n in NAMES] + [(K.EXACT_CASE, 0.0)])
def test_reference_alone_meets_the_row_bounds(name, lam):
    r32, _ = K.case_reference(name, np.float32, lam=lam)
    r64, _ = K.case_reference(name, np.float64, lam=lam)
    for s in range(K.STEPS):
        assert abs(float(r32[s]['loss']) - float(r64[s]['loss'])) <= 1e-6 * abs(float(r64[s]['loss']))
        present = _present(name, s)
        for key, mult in CHECKED[s]:
            a32, a64 = r32[s][key], r64[s][key]
            assert np.isfinite(a32).all() and np.isfinite(a64).all()
            err, row = U.row_err(a32, a64)
            norms = np.sqrt((np.asarray(a64, np.float64) ** 2).sum(axis=1))
            floor = ROW_FLOOR * float(np.median(norms))
            low = present[norms[present] <= floor]
            print('%s step %d %s: float32 vs float64 twin row_err %.2e (row %d), smallest present row norm %.2e, floor %.2e'
                  % (name, s, key, err, row, norms[present].min(), floor))
            assert err < mult * U.ROW_TOL64, (name, s, key, err, row)
            assert len(low) == 0, (name, s, key, 'rows the floor of row_err would hide', low[:10], norms[low[:10]])


@pytest.mark.parametrize('name', NAMES)
def test_no_mask_is_near(name):
    """Every sigmoid(u) lies inside (1e-3, 1 - 1e-3) and every |t| below 0.999: far from the clip bounds 1e-7 and 1 - 2^-23, so
    an fp32 mask decision cannot differ between the device and the twin."""
    c = K.case_problem(name)
    r64, _ = K.case_reference(name, np.float64)
    E = np.asarray(c['E0'], np.float64)
    for s in range(K.STEPS):
        f = K.pair_terms(c, E, s)[4]
        assert 1e-3 < f['sig'].min() and f['sig'].max() < 1 - 1e-3 and np.abs(f['t']).max() < 0.999, (name, s)
        E = r64[s]['E']


# --------------------------------------------------------------------------------------------------------------------- #
# teeth
# --------------------------------------------------------------------------------------------------------------------- #

def _miss(name, s, wrong_run):
    """By how many times the state a wrong run leaves after step s misses the GPU test's float64 bounds (the largest over the
    tensors checked there)."""
    r64, _ = K.case_reference(name, np.float64)
    return max(U.row_err(wrong_run[s][key], r64[s][key])[0] / (mult * U.ROW_TOL64) for key, mult in CHECKED[s])


@pytest.mark.parametrize('name', list(K.STRUCTURE_CASES) + ['loss_scalar_d130', 'upload_two_slabs'])
def test_chunked_restatement_is_the_oracle(name):
    """Right, K.ChunkedGradient gives the oracle's gradient in both steps and K.chunked_run the float64 twin's state."""
    c = K.case_problem(name)
    r64, _ = K.case_reference(name, np.float64)
    run = K.chunked_run(name)
    E = np.asarray(c['E0'], np.float64)
    for s in range(K.STEPS):
        want = K.pair_terms(c, E, s)[3]
        assert U.row_err(run[s]['g'], want)[0] < 1e-9, (name, s)
        assert np.array_equal(run[s]['g'][_counts(name, s)[0] == 0], np.zeros((int((_counts(name, s)[0] == 0).sum()), c['de'])))
        E = r64[s]['E']
        assert _miss(name, s, run) < 1e-3, (name, s)


def _run_rows(name, s):
    """(rows whose run of step s crosses a chunk boundary, their first and last chunks)"""
    live, _ = _counts(name, s)
    end = np.cumsum(live)
    start = end - live
    rows = np.nonzero((live > 0) & (start // K.CHUNK != (np.maximum(end, 1) - 1) // K.CHUNK))[0]
    return rows, start[rows] // K.CHUNK, (end[rows] - 1) // K.CHUNK


@pytest.mark.parametrize('name', ['runs_wave_v1', 'runs_wg_v1_d510', 'runs_wg_v4_d512', 'one_row_d384', 'runs_wave_d320'])
def test_a_dropped_carry_misses_the_bound(name):
    """One head carry, or one tail carry, left out of the fix-up of the LONGEST run of step 1 (the run a single carry is the
    smallest part of): the first moment after step 1 misses its bound at least ten times."""
    rows, cs, cl = _run_rows(name, 0)
    row = int(rows[np.argmax(cl - cs)])
    for what in ('drop_head', 'drop_tail'):
        miss = _miss(name, 0, K.chunked_run(name, (what, row)))
        print('%s, %s of row %d (%d chunks): misses the bound %.0f times' % (name, what, row, int((cl - cs).max()) + 1, miss))
        assert miss >= 10, (name, what, row, miss)


def test_other_mutants_miss_the_bound():
    out = {}
    # the columns of the second column pass of foldin_chunk_reduce<1, 4>
    out['second column pass, runs_wave_v1'] = _miss('runs_wave_v1', 0, K.chunked_run('runs_wave_v1', ('second_column_pass',)))
    # the last live pair in front of the sentinel: where it is the chunk's only live pair, where the sentinel starts in the last
    # slot behind a run of four chunks, and where it starts a chunk
    for name in ('n256_d300', 'runs_wave_d320', 'runs_wave_v1'):
        out['last live pair, ' + name] = _miss(name, 0, K.chunked_run(name, ('drop_last_live_pair',)))
    # the sentinel run added into row 0: N a power of two (an off-by-one in sort_bits), present and absent row 0
    for name in ('n2048_d8', 'n4_d8', 'runs_wg_v1_d510'):
        out['sentinel into row 0, ' + name] = _miss(name, 0, K.chunked_run(name, ('sentinel_into_row0',)))
    # step 1's run bounds kept in step 2: the state after step 2
    for name in ('runs_wave_v1', 'n2048_d8', 'n255_d128'):
        out['stale run bounds, ' + name] = _miss(name, 1, K.chunked_run(name, ('stale_bounds',)))
    # the second upload slab shifted by one row: the batch that straddles the boundary
    c = K.case_problem('upload_two_slabs')
    X = c['X'].copy()
    X[K.SLAB:-1] = c['X'][K.SLAB + 1:]
    out['second slab shifted, upload_two_slabs'] = _miss('upload_two_slabs', 0, K.chunked_run('upload_two_slabs', X=X))
    for what, miss in out.items():
        print('%s: misses the bound %.0f times' % (what, miss))
    weak = {k: v for k, v in out.items() if v < 10}
    assert not weak, weak
