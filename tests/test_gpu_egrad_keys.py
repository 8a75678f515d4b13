"""-m gpu: dR_e, the entity-table gradient of the vectorspace step, at every run and list structure of both of its paths
(tests/egrad_key_cases.py), row by row against the float64 oracle.  What every step launched is asked of the engine
(Engine.egrad_plan, sert_debug_egrad_plan): a case that a moved dispatch threshold takes off its kernels fails here instead
of passing for the wrong reason.  tests/test_egrad_keys_inputs_cpu.py proves the inputs: the keys are the stated plans, the
cases produce every event of K.EVENTS between them, the float32 oracle alone is within U.ROW_TOL64 of the float64 one and no
present row is small enough for the floor of U.row_err to hide it."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import egrad_key_cases as K
from tests import util as U

pytestmark = pytest.mark.gpu

RE_STATE = ('R_e', 'm.R_e', 'v.R_e')


def _engine(name, keep, monkeypatch, sort):
    """An engine of the case with its dataset uploaded; `sort`: SERT_EGRAD_SORT=1 (read at sert_create)."""
    c, p = K.case_problem(name)
    if sort:
        monkeypatch.setenv('SERT_EGRAD_SORT', '1')
    else:
        monkeypatch.delenv('SERT_EGRAD_SORT', raising=False)
    eng = U.vs_engine(p, c['B'], K.N, c['z'], K.LAM, keep_grads=keep)
    assert eng.egrad_plan() == {'path': 'none'}, (name, 'before the first backward')
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    return eng


def _train(eng, name, step):
    _, p = K.case_problem(name)
    eng.train_batch(step, p['neg'][step] if p['neg'][step].shape[1] else None)
    return eng.egrad_plan()


def _check_plan(name, step, got, want):
    assert got == want, (name, 'step', step, 'the backward launched', got, 'the case is there for', want)
    if got['path'] == 'bucket':
        # the list structure the case claims, from the REPORTED geometry and the keys
        c, _ = K.case_problem(name)
        claimed = K.events_of(name, step)
        reached = K.bucket_events(K.step_keys(name, step), c['Ve'], c['de'], got)
        assert claimed <= reached, (name, step, sorted(claimed - reached))


def _gradient_steps(name, monkeypatch, sort, want):
    """Both steps of a case on a fresh engine with keep_grads = 1: [dR_e (V_e, d_e) of step 0, of step 1], each checked row by
    row against the float64 oracle; the plan of each step asserted."""
    c, p = K.case_problem(name)
    g64, _ = K.case_reference(name, np.float64)
    Ve, de = c['Ve'], c['de']
    l2k = np.float32(K.LAM) / np.float32(c['B'])       # csrc/host/optimizer_and_loss.inc: lambda / B, in float
    eng = _engine(name, 1, monkeypatch, sort)
    out = []
    for s in range(K.STEPS):
        Re = eng.get_tensor(C.T_RE, (Ve, de)).copy()    # the table this step reads (step 1: after the engine's own update)
        plan = _train(eng, name, s)
        _check_plan(name, s, plan, want)
        got = eng.get_tensor(C.T_GRAD_RE, (Ve, de)).copy()
        err, row = U.row_err(got, g64[s])
        counts = K.step_counts(name, s)
        print('%s step %d%s: plan %s; dR_e worst row error against float64 %.2e (entity %d, %d pairs)'
              % (name, s, ' SERT_EGRAD_SORT=1' if sort and K.is_bucket(name) else '', plan, err, row, counts[row]))
        assert err < U.ROW_TOL64, (name, 'step', s, 'row_err against the float64 oracle', err, 'entity', row, 'pairs', int(counts[row]))
        # An absent entity's row is EXACTLY zero.  T_GRAD_RE is read behind the optimiser, which adds the L2 term
        # (lambda / B) R_e to the stored gradient in float with contraction off (kernels_opt.h: adam_elem), so a row the
        # batch does not touch holds exactly fl(l2k * R_e) -- 0.0 + x = x -- and anything left of an earlier step, or of
        # another entity's carry, shows as a difference in the last bit.
        absent = np.nonzero(counts == 0)[0]
        data = got[absent] - l2k * Re[absent]
        bad = np.nonzero(np.any(data != 0.0, axis=1))[0]
        assert len(bad) == 0, (name, 'step', s, 'rows of absent entities that are not exactly zero', absent[bad][:10], data[bad][:3])
        out.append(got)
    eng.close()
    return out


@pytest.mark.parametrize('name', list(K.CASES))
def test_entity_gradient_row_by_row(hip_lib, monkeypatch, name):
    """keep_grads = 1.  Two steps with different plans on one engine, each dR_e within U.ROW_TOL64 of the float64 oracle row by
    row and exactly zero where the entity is absent, the plan of each step as the case states it; a second engine bit for
    bit; the bucket cases also through the sort, the two paths within 2 ROW_TOL64 of each other row by row (each is within
    ROW_TOL64 of float64).

    Measured on the MI355X, worst row error against float64 over both steps (the bound is 5e-5): runs_wave_v1 7.2e-7,
    runs_wg_v1 4.5e-7, runs_wg_v4_d512 3.5e-7, one_entity_d384 1.1e-7, runs_wave_d320 8.3e-7, v2048_d64 3.2e-7, v2049_d128 2.7e-7,
    v70000_d8 1.1e-6 (a row of an absent entity in step 2: the L2 term of a table the engine updated itself), lists_v100_d128
    6.4e-7, z0_v16_d4 2.2e-7, z20_v2048_d32 2.0e-7, deep_groups_d4 5.4e-7; the bucket cases through the sort 1.3e-7 ... 6.3e-7, the
    two paths at most 5.0e-7 apart.  As a check of this test (not kept): with the final flush of egrad_chunk_reduce treating
    touches_end as false, every one of the eight sorted cases fails in step 0 with a row error of 0.8 ... 2.3 and names the
    entity -- runs_wave_v1: entity 263, a run of 16 pairs that crosses a chunk boundary."""
    c, _ = K.case_problem(name)
    bucket = K.is_bucket(name)
    first = _gradient_steps(name, monkeypatch, not bucket, c['plan'])
    again = _gradient_steps(name, monkeypatch, not bucket, c['plan'])
    for s in range(K.STEPS):
        assert U.same_bits(first[s], again[s]), (name, 'step', s, 'a second engine differs', U.row_err(again[s], first[s]))
    if bucket:
        through_sort = _gradient_steps(name, monkeypatch, True, c['sorted_plan'])
        for s in range(K.STEPS):
            err, row = U.row_err(first[s], through_sort[s])
            print('%s step %d: bucket against sorted, worst row %.2e (entity %d)' % (name, s, err, row))
            assert err < 2 * U.ROW_TOL64, (name, 'step', s, 'bucket against sorted', err, 'entity', row)


@pytest.mark.parametrize('name', list(K.CASES))
def test_entity_table_after_the_product_steps(hip_lib, monkeypatch, name):
    """keep_grads = 0, the product path: the entity table's update may be deferred behind the tail and the optimiser adds the
    bucket path's group tables itself.  Nothing is read between the two steps (the plan hook touches no device); then R_e and
    both of its Adam moments against the float32 and the float64 oracle's train_step, globally and row by row."""
    c, _ = K.case_problem(name)
    _, o32 = K.case_reference(name, np.float32)
    _, o64 = K.case_reference(name, np.float64)
    eng = _engine(name, 0, monkeypatch, not K.is_bucket(name))
    for s in range(K.STEPS):
        _check_plan(name, s, _train(eng, name, s), c['plan'])
    log = U.check_state(U.engine_state(eng), U.oracle_state(o32), U.oracle_state(o64), names=RE_STATE)
    eng.close()
    print('%s keep_grads=0: %s' % (name, '; '.join(log)))
