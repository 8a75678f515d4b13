"""-m gpu: sequences of API calls in which every step-schedule mechanism is live (tests/op_sequence_cases.py), call by call
against the NumPy oracle and bit for bit against an engine that is never told anything.

Three engines run the sequence of a case: the product engine with the announcements the sequence states (sert_hint_next_batch),
the product engine never told anything, and -- vectorspace kinds -- keep_grads = 1, never told anything (dense launches, no
run-ahead, no deferral).
  1. announced against unannounced: every returned number, every tensor read, the step and the draw counter after every call and
     the final state, bit for bit;
  2. keep_grads = 1 against the product engine: every tensor read, every prediction and the final state bit for bit, losses
     within 2e-6 (the relations of tests/test_gpu_lazy_dense.py);
  3. against the oracle at every call: losses and predictions within 1e-5, every tensor read in the sequence and the final state
     under util.check_tensor / check_state's bounds against the float32 and the float64 replay, the counters against the host
     model of the replay;
  4. liveness: the hooks show that every mechanism the case is there for ran -- and was off where it has to be off;
  5. the transitions without a launch of their own (sert_debug_state_counts): a run-ahead is consumed or discarded exactly where
     the sequence says, flushes of the lazy table and settled entity updates happen where a call has to make them.
Every failure names the index of the op."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import op_sequence_cases as S
from tests import util as U

pytestmark = pytest.mark.gpu


def run_sequence(name, ops, hinted, keep_grads):
    """(what every op returned, the hooks' records behind every op, the final state)."""
    eng = S.make_engine(name, keep_grads)
    state = dict(train_rows=np.arange(S.CASES[name]['B'] * S.NB))
    kind = S.CASES[name]['kind']
    outs, hooks = [], []
    for i, op in enumerate(ops):
        outs.append(S.apply_op(eng, name, ops, i, hinted, state))
        h = dict(state=eng.state_counts(), upd=eng.update_counts(), tails=eng.tail_counts())
        if S.is_training(op) and kind != 'll':
            h.update(plan=eng.vs_plan(), facts=eng.vs_facts())
        if S.is_training(op) and kind == 'vs':
            h.update(egrad=eng.egrad_plan(), nce=eng.nce_form())
        if kind == 'll' and (S.is_training(op) or op['op'] in ('eval', 'eval_many')):
            h.update(ll=eng.ll_loss_form())
        hooks.append(h)
    final = U.engine_state(eng)
    eng.close()
    return outs, hooks, final


def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return U.same_bits(a, b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


def check_equal_runs(ops, a, b, what, loss_tol=None):
    """Two engines' runs: everything bit for bit, or -- loss_tol -- the losses within it."""
    (outs_a, _, final_a), (outs_b, _, final_b) = a, b
    for i, (x, y) in enumerate(zip(outs_a, outs_b)):
        assert sorted(x) == sorted(y), (what, i, ops[i])
        for k in x:
            if loss_tol is not None and k in ('loss', 'losses'):
                assert close(x[k], y[k], loss_tol), (what, 'op', i, ops[i], k, x[k], y[k])
            else:
                assert same(x[k], y[k]), (what, 'op', i, ops[i], k, 'differs')
    for k in final_a:
        assert same(final_a[k], final_b[k]), (what, 'final state', k)


def check_against_oracle(name, ref, run, tensors):
    """Every call of a run against the replay; tensors: also the tensors read in the sequence and the final state."""
    ops, kind = ref['ops'], S.CASES[name]['kind']
    outs, _, final = run
    log = []
    for i, (op, rec, out) in enumerate(zip(ops, ref['records'], outs)):
        at = ('op', i, op)
        assert (out['step'], out['draws']) == (rec['step'], rec['draws']), (at, 'step and eval draws', out['step'], out['draws'], rec['step'], rec['draws'])
        got = [out['loss']] if 'loss' in out else list(out.get('losses', []))
        want = [rec['loss']] if 'loss' in rec else rec.get('losses', [])
        assert len(got) == len(want), at
        for g, (r32, r64) in zip(got, want):
            print('op %3d %-14s loss %.7g  float32 replay %.7g (%.1e)  float64 %.7g (%.1e)' % (
                i, op['op'], g, r32, abs(g - r32) / abs(r32), r64, abs(g - r64) / abs(r64)))
            assert abs(g - r32) <= S.LOSS_TOL * abs(r32) and abs(g - r64) <= S.LOSS_TOL * abs(r64), (at, 'loss', g, r32, r64)
        if op['op'] == 'train_explicit' and kind == 'vs':
            assert np.array_equal(out['negatives'], S.explicit_negatives(name, rec['step'] - 1)), (at, 'negatives_of_step(get_step())')
        if op['op'] == 'negatives_of_step':
            assert np.array_equal(out['value'], rec['value']), at
        if op['op'] == 'predict' and kind != 'll':
            e32, e64 = U.rel_err(out['value'], rec['value'][0]), U.rel_err(out['value'], rec['value'][1])
            print('op %3d predict_project %.1e %.1e' % (i, e32, e64))
            assert e32 < S.LOSS_TOL and e64 < S.LOSS_TOL, (at, e32, e64)
        if op['op'] == 'predict' and kind == 'll':
            e32, e64 = U.rel_err(out['tokens'], rec['tokens'][0]), U.rel_err(out['tokens'], rec['tokens'][1])
            print('op %3d predict_tokens %.1e %.1e' % (i, e32, e64))
            assert e32 < S.LOSS_TOL and e64 < S.LOSS_TOL, (at, e32, e64)
            idx, score, status = out['ranks']
            assert np.all(status == C.LL_STATUS_DEVICE), at
            Ve = S.CASES[name]['Ve']
            for q in range(idx.shape[0]):
                assert np.array_equal(np.sort(idx[q]), np.arange(Ve)), (at, 'query', q, 'not a permutation of the entities')
                for r in (rec['ranks'][0][q], rec['ranks'][1][q]):
                    at_dev = r[idx[q].astype(np.int64)]
                    e = U.rel_err(score[q], at_dev)
                    assert e < S.LOSS_TOL, (at, 'query', q, 'scores', e)
                    # ... and the device's order is the reference's wherever two reference scores are further apart than that
                    assert np.all(at_dev[1:] - at_dev[:-1] <= S.LOSS_TOL * r.max()), (at, 'query', q, 'order')
        if op['op'] == 'get' and tensors:
            k = op['which']
            square = k.rpartition('.')[0] in U.SECOND_MOMENTS
            try:
                log.append('op %3d ' % i + U.check_tensor(k, out['value'], rec['value'][0], rec['value'][1], row_tol32=U.state_row_tol32(k),
                                                          row_tol64=(2 if square else 1) * U.ROW_TOL64))
            except AssertionError as e:
                raise AssertionError((at, e.args))
    if tensors:
        log += U.check_state(final, ref['final'][0], ref['final'][1], prefix='final ')
    print('\n'.join(log))


def model_run_ahead(name, ops):
    """(discarded, consumed) behind every op for an engine that announces what the sequence says: the host model of
    spec_fb_batch (csrc/host/api_data_train.inc, optimizer_and_loss.inc)."""
    speculates = S.CASES[name]['dw'] % 4 == 0 or S.CASES[name]['kind'] != 'vs'      # (the vectorspace run-ahead needs the touched-row path)
    live, discarded, consumed, out = None, 0, 0, []
    for i, op in enumerate(ops):
        if S.is_training(op):
            if live is not None:
                # (explicit negatives exist for the NCE model only: elsewhere train_explicit is a plain step)
                if (op['op'] != 'train_explicit' or S.CASES[name]['kind'] != 'vs') and S.first_batch(op) == live:
                    consumed += 1
                else:
                    discarded += 1
                live = None
            if op['op'] == 'train' and speculates:
                h = S.hinted_batch(ops, i)
                live = h if h is not None and h >= 0 else None
        elif op['op'] in S.INVALIDATING and live is not None:
            discarded += 1
            live = None
        out.append((discarded, consumed))
    return out


def delta(hooks, i, group, key):
    return hooks[i][group][key] - (hooks[i - 1][group][key] if i > 0 else 0)


def check_liveness(name, ops, plain, hinted, keep):
    c = S.CASES[name]
    kind = c['kind']
    steps = sum(len(op['bs']) if op['op'] == 'train_many' else 1 for op in ops if S.is_training(op))
    hp, hh = plain[1], hinted[1]
    trains = [i for i, op in enumerate(ops) if op['op'] == 'train']

    # ---- 5. transitions that launch nothing of their own
    model = model_run_ahead(name, ops)
    for i, op in enumerate(ops):
        got = (hh[i]['state']['run_ahead_discarded'], hh[i]['state']['run_ahead_consumed'])
        assert got == model[i], ('op', i, op, 'run-aheads (discarded, consumed)', got, 'expected', model[i])
        assert (hp[i]['state']['run_ahead_discarded'], hp[i]['state']['run_ahead_consumed']) == (0, 0), ('op', i, op)
    if c['dw'] % 4 == 0 or kind != 'vs':
        assert model[-1][0] > 0 and model[-1][1] > 0, model[-1]
        wrong = [i for i in trains if ops[i]['hint'] == 'wrong']
        assert wrong and all(model[S.next_training(ops, i)][0] == model[S.next_training(ops, i) - 1][0] + 1 for i in wrong)
    else:
        assert model[-1] == (0, 0)
    # the lazy table: an engine that is never told anything leaves no row behind; the announcing one does, and the reads and
    # the invalidating calls behind an announcing step flush them
    assert hp[-1]['state']['lazy_flushes'] == 0
    if c['lazy']:
        flushed_by = {ops[i]['op'] for i in range(len(ops)) if delta(hh, i, 'state', 'lazy_flushes') > 0}
        assert {'get', 'eval', 'set_step', 'set', 'predict' if kind == 'll' else 'get'} <= flushed_by, flushed_by
        for i, op in enumerate(ops):
            if op['op'] in ('synchronize', 'set_eval_draws', 'negatives_of_step'):
                assert delta(hh, i, 'state', 'lazy_flushes') == 0, ('op', i, op)
    else:
        assert hh[-1]['state']['lazy_flushes'] == 0
    # the word-table update by form
    for h, lazy in ((hp, c['lazy']), (hh, c['lazy'])) + (((keep[1], False),) if keep else ()):
        u = h[-1]['upd']
        assert u['dense'] == (0 if lazy else steps) and u['skip_32_1'] == (steps if lazy else 0), u
        assert u['skip_full'] + u['skip_sparse'] == (steps if lazy else 0) and u['lazy'] == 0, u
    if c['lazy']:
        assert hh[-1]['upd']['skip_sparse'] > 0 and hh[-1]['upd']['skip_full'] > 0 and hp[-1]['upd']['skip_full'] > 0
        # the announced run at the head: a full pass, kLazyK - 1 sparse ones, a full one
        assert [delta(hh, i, 'upd', 'skip_sparse') for i in range(6)] == [0, 1, 1, 1, 0, 1]

    if kind == 'll':
        for h in (hp, hh):
            for i, op in enumerate(ops):
                if 'll' not in h[i]:
                    continue
                f = h[i]['ll']
                assert f['train'] == S.is_training(op), ('op', i, op, f)
                if name == 'll_stream':
                    assert (f['form'], f['param'], f['segments']) == ('stream', 0, 3), ('op', i, op, f)
                if S.is_training(op) or op['split'] == 'train':
                    assert f['slots'], ('op', i, op, f)          # the distinct-word table
                else:
                    assert not f['slots'], ('op', i, op, f)
        return

    # ---- the schedule of every step is the plan of its facts
    for what, h in (('plain', hp), ('hinted', hh), ('keep_grads', keep[1])):
        for i, op in enumerate(ops):
            if 'plan' in h[i]:
                assert h[i]['plan'] == C.vs_plan_for(**h[i]['facts']), (what, 'op', i, op)
    if kind == 'fs':
        assert all(hp[i]['plan']['side_small'] for i in trains)
        return

    # ---- vectorspace: tails, early keys, the deferred entity update (named ops: on the engine that is never told anything, whose
    # plan behind a train op is that op's)
    touched_path = c['dw'] % 4 == 0
    assert all(h[i]['plan']['combine_in_tail'] for h in (hp, hh) for i in trains)
    assert hp[-1]['tails'] == {'alone': steps, 'in_gather': 0}
    t = hh[-1]['tails']
    assert t['alone'] + t['in_gather'] == steps and (t['in_gather'] > 0) == touched_path and t['alone'] > 0, t
    path = 'bucket' if c['Ve'] <= S.SORT_FREE_MAX_ENTITIES and c['de'] % 4 == 0 else 'sorted'
    assert all(h[i]['egrad']['path'] == path for h in (hp, hh) for i in trains)
    assert all(h[i]['nce']['train'] and (h[i]['nce']['form'] == 'scalar') == (c['de'] % 4 != 0) for h in (hp, hh) for i in trains)
    big_re = c['Ve'] * c['de'] > 1 << 22
    for i in trains:
        ready = touched_path and S.negatives_drawn_ahead(ops, i)
        f, p = hp[i]['facts'], hp[i]['plan']
        at = ('op', i, ops[i])
        assert f['neg_side_ready'] == int(ready) and f['big_re'] == int(big_re), (at, f)
        assert p['sort_early'] == (ready and path == 'sorted'), (at, 'sort_early', p['sort_early'])
        assert p['bucket_early'] == (ready and path == 'bucket' and c['B'] >= 32768), (at, 'bucket_early', p['bucket_early'])
        assert p['defer_re'] == big_re and p['re_on_side'] == big_re and p['defer_small'] == (not big_re), (at, p)
        if name == 'vs_b32768':
            assert p['order'][:2] == ('dh', 'dense') and p['dense_queue'] == 'side', (at, p)
        # the sums of squares of R_e: handed over by the step before, or read again behind whatever invalidated them
        handed = S.negatives_drawn_ahead(ops, i)
        got = tuple(delta(hp, i, 'state', k) for k in ('re_sq_handed', 're_sq_small', 're_sq_adam'))
        assert got == ((1, 0, 0) if handed else (0, 0, 1) if big_re else (0, 1, 0)), (at, 'sums of squares of R_e', got)
    ready = [S.negatives_drawn_ahead(ops, i) for i in trains]
    assert any(ready) and not all(ready[1:])
    if path == 'bucket':
        assert any(hp[i]['plan']['draw_next_neg'] for i in trains)
    # a deferred update is settled by the call that reads R_e next: an evaluation behind a training step waits for it
    for i, op in enumerate(ops):
        if op['op'] in ('eval', 'eval_many') and i > 0 and S.is_training(ops[i - 1]):
            assert delta(hp, i, 'state', 're_settled') == 1, ('op', i, op, 'the evaluation did not settle the deferred update')
    assert hh[-1]['state']['re_settled'] > 0 and hh[-1]['state']['re_sq_handed'] > 0
    s = keep[1][-1]['state']
    assert all(v == 0 for v in s.values()), s


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_api_call_sequences(hip_lib, name):
    ref = S.case_reference(name)
    ops = ref['ops']
    plain = run_sequence(name, ops, hinted=False, keep_grads=0)
    hinted = run_sequence(name, ops, hinted=True, keep_grads=0)
    check_equal_runs(ops, hinted, plain, 'announced against unannounced')
    keep = None
    if S.CASES[name]['kind'] != 'll':
        keep = run_sequence(name, ops, hinted=False, keep_grads=1)
        check_equal_runs(ops, keep, plain, 'keep_grads = 1 against the product engine', loss_tol=S.KEEP_LOSS_TOL)
        check_against_oracle(name, ref, keep, tensors=False)
    check_against_oracle(name, ref, plain, tensors=False)
    check_against_oracle(name, ref, hinted, tensors=True)
    check_liveness(name, ops, plain, hinted, keep)
