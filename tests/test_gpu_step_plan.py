"""-m gpu: which schedule the vectorspace training step RAN.

tests/test_gpu_parity.py::test_schedule_variants_do_not_change_a_bit proves that every schedule gives the same bits; nothing
there says which one a step took.  Here three steps at the smallest shapes that reach each schedule, each in a fresh process
(the knobs are read once per process), and after every step
  * Engine.vs_plan() -- the plan the step issued from (csrc/step_plan.h, sert_model::plan) -- equals vs_plan_for(the facts of
    that engine and step, Engine.vs_facts()) and the plan pinned for the case in tests/step_plan_cases.py, and those facts
    are what the configuration and the step number say they must be;
  * the entity chain's record (Engine.egrad_plan) and the tail counters agree with it;
  * the loss is finite.
A change that moves a shape off its schedule fails here instead of showing up as a slower benchmark line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import _capi as C
from tests import step_plan_cases as S
from tests import util as U

pytestmark = pytest.mark.gpu

WORKER = r'''
import sys, json
sys.path.insert(0, %(root)r)
import numpy as np
from tests import util as U
from sert_amd import _capi as C
d = %(dims)r
p = U.make_vs_problem(17, 3 * d['B'], d['n'], d['z'], d['Vw'], d['Ve'], d['dw'], d['de'], zipf=True)
eng = U.vs_engine(p, d['B'], d['n'], d['z'], 0.01, keep_grads=0, seed=5)
eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
out = {'before': eng.vs_plan(), 'steps': []}
if %(timing)d:
    eng.timing_enable(%(timing)d)
for s in range(3):
    loss = float(eng.train_batch(s))
    out['steps'].append(dict(loss=loss, plan=eng.vs_plan(), facts=eng.vs_facts(), egrad=eng.egrad_plan(), tails=eng.tail_counts()))
eng.close()
print('RESULT ' + json.dumps(out))
'''

A_DIMS = dict(B=2048, n=3, z=10, Vw=2000, Ve=1000, dw=128, de=128)
# (the sort-free entity chain: V_e <= 2048, d_e <= 128 and a multiple of four -- csrc/host/api_model.inc)
SORT_FREE_MAX_ENTITIES = 2048
RUNS = {
    # name: (dims, environment, timing mode, case of step 0, case of the later steps)
    'A': (A_DIMS, {}, 0, 'A', 'A'),
    'B_side_heavy_2': (A_DIMS, {'SERT_SIDE_HEAVY': '2'}, 0, 'B_side_heavy_2', 'B_side_heavy_2'),
    'C_one_queue': (A_DIMS, {'SERT_STREAMS': '1'}, 0, 'C_one_queue', 'C_one_queue'),
    'E_timing': (A_DIMS, {}, 1, 'E_timing', 'E_timing'),
    'D_big_entity_table': (dict(B=1024, n=3, z=10, Vw=2000, Ve=40000, dw=32, de=128), {}, 0, 'D_first_step', 'D_big_entity_table'),
    'F_sorted_chain_late_fork': (dict(B=1024, n=3, z=10, Vw=2000, Ve=SORT_FREE_MAX_ENTITIES + 1, dw=32, de=64), {}, 0,
                                 'F_first_step', 'F_product_search'),
}


def engine_facts(d, env, timing, step):
    """What Engine.vs_facts() must report for step `step` of the worker's engine, from its configuration: the negatives of every
    step but the first were drawn during the step before where there is a side queue."""
    n_re = d['Ve'] * d['de']
    nstreams = int(env.get('SERT_STREAMS', 2))
    return S.facts(nstreams=nstreams, timing=int(timing == 1), n_re=n_re, big_re=int(n_re > 1 << 22), big_w=int(d['dw'] * d['de'] > 1 << 22),
                   batch=d['B'], word_dim=d['dw'], entity_dim=d['de'], num_negatives=d['z'],
                   sort_free=int(d['Ve'] <= SORT_FREE_MAX_ENTITIES and d['de'] <= 128 and d['de'] % 4 == 0),
                   neg_side_ready=int(step > 0 and nstreams >= 2 and timing != 1), next_neg_drawn=0,
                   k_side_heavy=int(env.get('SERT_SIDE_HEAVY', 1)))


@pytest.mark.parametrize('name', sorted(RUNS))
def test_steps_issue_the_pinned_plan(hip_lib, name):
    dims, env, timing, first_case, later_case = RUNS[name]
    code = WORKER % dict(root=U.ROOT, dims=dims, timing=timing)
    r = subprocess.run([sys.executable, '-c', code], check=True, env=dict(os.environ, **env), cwd=U.ROOT, stdout=subprocess.PIPE,
                       timeout=300)
    out = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])

    def as_plan(p):
        return dict(p, order=tuple(p['order']))

    assert as_plan(out['before']) == S.DEFAULT
    tails = 0
    for step, rec in enumerate(out['steps']):
        case = first_case if step == 0 else later_case
        facts = engine_facts(dims, env, timing, step)
        # the shape of the run differs from the shape of the pinned case only in what the plan does not depend on here
        pinned_facts, pinned = S.CASES[case]
        got = as_plan(rec['plan'])
        print(name, step, got)
        expected_facts = {k: 0 for k in C.VS_FACTS}
        expected_facts.update(C.VS_KNOB_DEFAULTS)
        expected_facts.update(facts)
        # (the shape predicates of a variants build's kernels are that build's: without their knobs they move nothing, which the
        #  pinned plan below asserts)
        for k in ('dh_strip', 'bwd_fused_shape'):
            expected_facts[k] = rec['facts'][k]
        assert rec['facts'] == expected_facts, (step, 'the facts the engine decided from',
                                                {k: (rec['facts'][k], expected_facts[k]) for k in expected_facts if rec['facts'][k] != expected_facts[k]})
        assert got == C.vs_plan_for(**rec['facts']), (step, 'the plan of the facts of this engine and step')
        assert got == pinned, (step, case, {k: (got[k], pinned[k]) for k in pinned if got[k] != pinned[k]})
        for k in ('nstreams', 'timing', 'big_re', 'sort_free', 'k_side_heavy'):
            assert facts[k] == pinned_facts.get(k, 0 if k != 'k_side_heavy' else 1), (k, 'the run is not the pinned case')
        # what the launches recorded agrees with the plan
        assert rec['egrad']['path'] == ('bucket' if facts['sort_free'] else 'sorted')
        if facts['sort_free']:
            assert rec['egrad']['group_sum'] == (not got['re_in_parts'])
        tails += int(got['combine_in_tail'])
        assert rec['tails'] == {'alone': tails, 'in_gather': 0}
        assert np.isfinite(rec['loss'])
