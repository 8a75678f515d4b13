"""CPU: the schedule of the vectorspace training step as csrc/step_plan.h decides it (vs_plan_step, through the test hook
sert_debug_vs_plan_for -- no device): the pinned plan of every schedule (tests/step_plan_cases.py), and two invariants over
the cross product of the facts."""
import ctypes
import itertools
import os
import re

import pytest

from sert_amd import _capi as C
from tests import step_plan_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_plan_of_case(hip_lib, name):
    facts, expected = S.CASES[name]
    got = C.vs_plan_for(**facts)
    assert got == expected, {k: (got[k], expected[k]) for k in expected if got[k] != expected[k]}


def test_binding_names_follow_the_header(hip_lib):
    """sert_amd._capi names the facts and the plan's entries in the order of SERT_VS_FACT_* / SERT_VS_PLAN_*, and the enums by
    value; the knob defaults of the binding are those of VsKnobs (a plan from no knob facts at all equals the defaults' plan)."""
    src = open(os.path.join(ROOT, 'include', 'sert_hip_debug.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    fact_names = re.findall(r'\bSERT_VS_FACT_([A-Z_0-9]+)\b', src.split('SERT_VS_FACT_COUNT')[0])
    assert tuple(n.lower() for n in fact_names) == C.VS_FACTS
    plan_names = re.findall(r'\bSERT_VS_PLAN_([A-Z_0-9]+)\b(?! \+)', src.split('SERT_VS_FACT_COUNT')[1].split('SERT_VS_PLAN_COUNT')[0])
    expanded = []
    for n in plan_names:
        expanded += ['order'] * 4 if n == 'ORDER' else [n.lower()]       # (SERT_VS_PLAN_ORDER: four entries)
    assert tuple(expanded) == C.VS_PLAN
    for prefix, names in (('FORK', C.VS_FORKS), ('PIECE', C.VS_PIECES), ('QUEUE', C.VS_QUEUES), ('EVENT', C.VS_EVENTS)):
        for k, name in enumerate(names):
            assert re.search(r'\bSERT_VS_%s_%s = %d\b' % (prefix, name.upper().replace('EV_', ''), k), src), (prefix, name)
    # facts cut off in front of the knobs: the defaults of VsKnobs
    n = C.VS_FACTS.index('k_ext_events')
    vals = dict({name: 0 for name in C.VS_FACTS}, **S.facts())
    f = (ctypes.c_int32 * n)(*[vals[name] for name in C.VS_FACTS[:n]])
    v = (ctypes.c_int32 * len(C.VS_PLAN))()
    hip_lib.sert_debug_vs_plan_for.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    assert hip_lib.sert_debug_vs_plan_for(f, n, v, len(C.VS_PLAN)) == 0
    assert C._vs_plan_dict(v) == S.A


def test_plan_hooks_refuse_bad_arguments(hip_lib):
    v = (ctypes.c_int32 * len(C.VS_PLAN))()
    f = (ctypes.c_int32 * len(C.VS_FACTS))()
    hip_lib.sert_debug_vs_plan_for.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    hip_lib.sert_debug_vs_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    for args in ((None, 1, v, 1), (f, 0, v, 1), (f, len(C.VS_FACTS) + 1, v, 1), (f, 1, None, 1), (f, 1, v, 0), (f, 1, v, len(C.VS_PLAN) + 1)):
        assert hip_lib.sert_debug_vs_plan_for(*args) != 0, args
        assert b'bad argument' in hip_lib.sert_last_error()
    assert hip_lib.sert_debug_vs_plan(None, v, 1) != 0
    hip_lib.sert_debug_vs_facts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    assert hip_lib.sert_debug_vs_facts(None, f, 1) != 0


def test_invariants_over_the_cross_product_of_the_facts(hip_lib):
    """Whatever the facts:
      * a plan that puts anything on a side queue has nstreams >= 2 and timing off;
      * a plan without lazy_join and without dp_late_join whose backward used the side queue joins it at the end of the backward
        (and one whose dense gradients went to the third queue waits for their event there -- Engine-side: dense_event ev_join3);
      * only a kernel the plan launches through a completion signal carries an event, and the order is a permutation."""
    flags = ('host_ar', 'comm', 'timing', 'big_re', 'big_w', 'keep_grads', 'sort_free', 'neg_side_ready', 'next_neg_drawn', 'dh_strip')
    count = 0
    for bits in itertools.product((0, 1), repeat=len(flags)):
        f = dict(zip(flags, bits))
        f['n_re'] = 40000 * 128 if f['big_re'] else 1000 * 128
        for nstreams, kind, side_heavy in itertools.product((1, 2, 3), (S.KIND_VECTORSPACE, S.KIND_SOFTMAX), (1, 2)):
            p = C.vs_plan_for(**S.facts(nstreams=nstreams, kind=kind, k_side_heavy=side_heavy, **f))
            count += 1
            backward_side = (p['entity_queue'] != 'main' or p['dense_queue'] != 'main' or p['bucket_early'] or p['sort_early'] or
                             p['draw_next_neg'] or p['side_meets_fork'])
            update_side = p['side_small'] or p['re_on_side'] or p['defer_re'] or p['defer_small'] or p['split_small']
            if backward_side or update_side or p['fork_carried'] or p['dh_carried'] or p['lazy_join'] or p['dp_late_join']:
                assert nstreams >= 2 and not f['timing'], (f, nstreams, p)
            if p['dense_queue'] == 'third':
                assert nstreams == 3 and p['dense_event'] == 'ev_join3', (f, p)
            if backward_side and not p['lazy_join'] and not p['dp_late_join']:
                assert p['end_join'], (f, nstreams, p)
            if p['end_join']:
                assert backward_side
            assert sorted(p['order']) == sorted(C.VS_PIECES)
            assert not (p['fork_carried'] and p['fork_recorded'])
            if p['dh_carried']:
                assert p['dh_event'] != 'none' and not f['dh_strip']
            if kind != S.KIND_VECTORSPACE:
                assert not backward_side and p['fork_at'] == 'none' and not p['combine_in_tail']
    assert count == 12 * 1024
