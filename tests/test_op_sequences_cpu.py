"""CPU: what the inputs and the sequences of tests/op_sequence_cases.py are, and that the reference alone stays inside the bounds
the GPU test (test_gpu_op_sequences.py) holds the engines to."""
import ctypes
import re

import numpy as np
import pytest

from sert_amd import _capi
from tests import op_sequence_cases as S
from tests import util as U
from tests.test_capi_cpu import ROOT, _declared_functions

CASES = sorted(S.CASES)


def test_the_cases_are_the_shapes_their_mechanisms_need():
    """Lazy word table: 2^22 elements and more, rows of 16-byte pieces.  Sorted entity chain: more than 2048 entities or rows
    that are no multiple of four floats.  Big entity table: more than 2^22 elements."""
    for name, c in S.CASES.items():
        assert (c['Vw'] * c['dw'] >= S.LAZY_MIN_ELEMENTS and c['dw'] % 4 == 0) == c['lazy'], name
    c = S.CASES
    assert c['vs_sorted']['Ve'] > S.SORT_FREE_MAX_ENTITIES and c['vs_sorted']['Ve'] * c['vs_sorted']['de'] <= 1 << 22
    assert c['vs_lazy_big_re']['Ve'] * c['vs_lazy_big_re']['de'] > 1 << 22
    assert c['vs_scalar']['dw'] % 4 and c['vs_scalar']['de'] % 4
    assert c['vs_b32768']['B'] >= 32768 and c['vs_b32768']['Ve'] <= S.SORT_FREE_MAX_ENTITIES and c['vs_b32768']['de'] % 4 == 0
    # the streaming loss form: the (n + 1, V_e) slab of a row does not fit the 150 KB of the fused kernels; three 4096-wide segments
    assert (c['ll_stream']['n'] + 1) * c['ll_stream']['Ve'] * 4 > 150 * 1024 and -(-c['ll_stream']['Ve'] // 4096) == 3
    assert c['ll_stream']['Ve'] % 4


@pytest.mark.parametrize('name', [n for n in CASES if S.CASES[n]['lazy']])
def test_lazy_cases_touch_few_rows(name):
    """Every batch, in either row order, touches under 35 % of the word table: announced or not, the product engine takes
    dense_update_skip, whose row sums do not depend on which rows were skipped (csrc/kernels_opt.h)."""
    fr = S.touched_fractions(name)
    print(name, 'touched fraction: max %.4f' % max(fr))
    assert len(fr) == 2 * S.NB and max(fr) < S.LAZY_MAX_TOUCHED


@pytest.mark.parametrize('name', CASES)
def test_sequences_are_built_by_construction(name):
    ops = S.build_ops(name)
    assert ops == S.build_ops(name)                      # same seed, same list
    kinds = S.other_kinds(name)
    assert {op['op'] for op in ops} == set(kinds) | set(S.TRAIN_OPS)
    pos = S.op_positions(ops)
    for k in kinds:
        assert pos[k] == {'behind_live', 'before_announced', 'between_unhinted'}, (k, pos[k])
    # two calls between an announcing step and the announced one: somewhere the two positions are two different ops
    assert any(not S.is_training(ops[i]) and not S.is_training(ops[i + 1]) for i in range(len(ops) - 1))
    assert {op['hint'] for op in ops if op['op'] == 'train'} == set(S.HINTS)
    assert {op['which'] for op in ops if op['op'] == 'get'} == set(S.tensor_names(name))
    assert {op['form'] for op in ops if op['op'] == 'set'} == set(S.set_forms(name))
    assert {op['split'] for op in ops if op['op'] in ('eval', 'eval_many')} == {'train', 'valid'}
    # set_step and set_eval_draws move their counter
    assert all(op['delta'] != 0 for op in ops if op['op'] in ('set_step', 'set_eval_draws'))
    # announcements: a right one names the next training step's first batch, a wrong one another batch
    for i, op in enumerate(ops):
        if op['op'] != 'train':
            continue
        j = S.next_training(ops, i)
        h = S.hinted_batch(ops, i)
        if op['hint'] == 'right' and j is not None:
            assert h == S.first_batch(ops[j])
        if op['hint'] == 'wrong' and j is not None:
            assert 0 <= h < S.NB and h != S.first_batch(ops[j])
        if op['hint'] in ('none', 'cleared'):
            assert h == (None if op['hint'] == 'none' else -1)
    # a run of kLazyK + 2 announced steps stands at the head: full pass, sparse passes, full pass
    assert all(op['op'] == 'train' and op['hint'] == 'right' for op in ops[:6])
    # the un-hinted engine's early keys: some step has its negatives from the step before, some step behind an invalidating
    # call has not
    ahead = [S.negatives_drawn_ahead(ops, i) for i, op in enumerate(ops) if op['op'] == 'train']
    assert any(ahead) and not all(ahead[1:])
    n_train = sum(len(op['bs']) if op['op'] == 'train_many' else 1 for op in ops if S.is_training(op))
    print(name, '%d ops, %d training steps, %d other calls' % (len(ops), n_train, sum(not S.is_training(op) for op in ops)))


def _distances(a32, a64, name):
    """(global distance as a fraction of TENSOR_TOL, row-wise distance as a fraction of the entry's row bound) of two (rows, cols)
    entries of U.oracle_state."""
    row64 = (2 if name.rpartition('.')[0] in U.SECOND_MOMENTS else 1) * U.ROW_TOL64      # (check_state's float64 row bound)
    return U.rel_err(a32, a64) / U.TENSOR_TOL, U.row_err(a32, a64)[0] / min(U.state_row_tol32(name), row64)


@pytest.mark.parametrize('name', CASES)
def test_the_float32_replay_stays_inside_half_of_every_bound(name):
    """The float32 replay against the float64 one, at every op: losses and predictions within half of 1e-5, every tensor read
    in the sequence and the final state within half of TENSOR_TOL globally and half of its row bound against the float32
    oracle.  Loglinear: no probability the loss clips within a factor of two of a clip bound, anywhere in the sequence."""
    ref = S.case_reference(name)
    worst = dict(loss=0.0, predict=0.0, rel=0.0, row=0.0)
    for i, rec in enumerate(ref['records']):
        pairs = [rec['loss']] if 'loss' in rec else rec.get('losses', [])
        for a, b in pairs:
            assert np.isfinite(a) and np.isfinite(b), i
            worst['loss'] = max(worst['loss'], abs(float(a) - float(b)) / abs(float(b)))
        if rec['op'] == 'predict':
            for key in ('value', 'tokens'):
                if key in rec:
                    worst['predict'] = max(worst['predict'], U.rel_err(rec[key][0], rec[key][1]))
            for r32, r64 in zip(*rec.get('ranks', ([], []))):
                worst['predict'] = max(worst['predict'], U.rel_err(r32, r64))
        if rec['op'] == 'get':
            g, r = _distances(rec['value'][0], rec['value'][1], ref['ops'][i]['which'])
            assert g < 0.5 and r < 0.5, (i, ref['ops'][i], g, r)
            worst['rel'], worst['row'] = max(worst['rel'], g), max(worst['row'], r)
    for k in ref['final'][0]:
        g, r = _distances(ref['final'][0][k], ref['final'][1][k], k)
        assert g < 0.5 and r < 0.5, ('final', k, g, r)
        worst['rel'], worst['row'] = max(worst['rel'], g), max(worst['row'], r)
    print('%-15s losses %.1e  predict %.1e  tensors %.2f of TENSOR_TOL  rows %.2f of their bound  clip margin %.3g  replay %.1f s'
          % (name, worst['loss'], worst['predict'], worst['rel'], worst['row'], ref['clip_margin'], ref['seconds']))
    assert worst['loss'] < 0.5 * S.LOSS_TOL and worst['predict'] < 0.5 * S.LOSS_TOL
    if S.CASES[name]['kind'] == 'll':
        assert ref['clip_margin'] > 2.0
    # the host model of the counters: the step counter never goes below zero and moves at every set_step
    steps = [r['step'] for r in ref['records']]
    for i, op in enumerate(ref['ops']):
        if op['op'] == 'set_step':
            assert steps[i] != steps[i - 1] and steps[i] >= 0


def test_the_state_counts_hook_is_bound(hip_lib):
    """sert_debug_state_counts: declared in the debug header, exported, named position by position in the binding, and -- no
    device is touched -- it fails with a message without a model."""
    assert 'sert_debug_state_counts' in _declared_functions('sert_hip_debug.h')
    assert 'sert_debug_state_counts' in _capi.EXPORTS and hasattr(hip_lib, 'sert_debug_state_counts')
    header = open(ROOT + '/include/sert_hip_debug.h').read()
    doc = header[:header.index('int sert_debug_state_counts')].rsplit('/*', 1)[1]
    assert sorted(int(x) for x in re.findall(r'out\[(\d)\]', doc)) == list(range(len(_capi.STATE_COUNTS)))
    assert 'n <= %d' % len(_capi.STATE_COUNTS) in doc
    v = (ctypes.c_int64 * len(_capi.STATE_COUNTS))()
    hip_lib.sert_debug_state_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    assert hip_lib.sert_debug_state_counts(None, v, len(_capi.STATE_COUNTS)) != 0
    assert b'bad argument' in hip_lib.sert_last_error()
