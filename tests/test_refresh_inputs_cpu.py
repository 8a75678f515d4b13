"""CPU: the inputs of the refresh tests have the structure they exist for (tests/refresh_cases.py), the twin does what the
contract of sert_foldin_create_refresh says, the row bound of the GPU test tells slot order from id order, and the host
side of ``bin/fold_in.py --refresh`` (foldin.merge_meta, foldin.refresh_dump, the parser) does what it states.  No device."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi, foldin
from tests import refresh_cases as RC
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', list(RC.CASES))
def test_case_has_its_structure(name):
    c = RC.make_case(name)
    B, Ve, z, Nt, R, num_new = c['B'], c['Ve'], c['z'], c['Nt'], c['num_refresh'], c['num_new']
    refresh = c['refresh']
    assert Ve <= 320 and B <= 48 and z <= 3 and RC.STEPS == 2
    assert len(set(refresh.tolist())) == R and refresh.min() >= 0 and refresh.max() < Ve and Nt == R + num_new >= 1
    assert c['y'].min() >= 0 and c['y'].max() < Nt and c['X'].max() < c['Vw']
    assert c['M'] // B == RC.STEPS and c['M'] % B != 0
    assert not np.array_equal(c['neg'][0], c['neg'][1])
    refreshed = set(refresh.tolist())
    for s in range(RC.STEPS):
        neg, y = c['neg'][s], c['y'][s * B:(s + 1) * B]
        assert neg.shape == (B, z) and neg.min() >= 0 and neg.max() < Ve + num_new
        own = c['ext_of_slot'][y]
        is_refreshed = np.isin(neg, refresh)
        is_new = neg >= Ve
        is_frozen = ~is_refreshed & ~is_new
        keys = RC.slot_keys(c, s)
        counts = np.bincount(keys, minlength=Nt + 1)
        assert counts[:Nt].sum() >= B and counts[Nt] == is_frozen.sum()
        if name == 'order_and_edges':
            assert refresh.tolist() != sorted(refresh.tolist()) and {0, Ve - 1} <= refreshed and num_new == 0
            assert is_refreshed.any() and is_frozen.any() and (neg == own[:, None]).any(axis=1).sum() >= B // 3 - 1
            assert max(np.count_nonzero((neg == e).any(axis=1)) for e in refreshed) >= 5
        elif name == 'mixed':
            assert (y < R).any() and (y >= R).any() and is_new.any() and is_refreshed.any() and is_frozen.any()
        elif name == 'all_rows':
            assert sorted(refresh.tolist()) == list(range(Ve)) and refresh.tolist() != list(range(Ve)) and counts[Nt] == 0
        elif name == 'ragged':
            assert B == 20 and B % 16 == 4 and c['w_upload'] is None and np.all(c['w'] == 1)
        elif name == 'wave_fixup':
            assert Ve == 320 and R == 256 and c['de'] == 4 and c['plan']['fixup'] == 'wave' and counts[Nt] > 0
            assert (counts[:Nt] == 0).sum() > Nt // 2
        elif name == 'sparse':
            assert (counts[:Nt] == 0).sum() >= 6 and counts[Nt] > 0
        if name != 'ragged':
            assert c['w_upload'] is not None and c['w_upload'].min() >= 0.5 and c['w_upload'].max() <= 2.0


def test_every_loss_kernel_instance_has_its_case():
    seen = set()
    for name in RC.INSTANCE_CASES:
        c = RC.make_case(name)
        assert c['B'] == 16 and c['Ve'] == 8
        seen.add((c['plan']['loss'], c['plan']['k']))
        form, k = name.split('_k')
        assert c['plan']['loss'] == form and c['plan']['k'] == int(k)
        assert (c['de'] % 4 == 0) == (form == 'vector')
    assert seen == {(f, k) for f in ('vector', 'scalar') for k in range(1, 9)}


@pytest.mark.parametrize('name', ['order_and_edges', 'mixed', 'all_rows'])
def test_twin_is_the_oracle_with_ext_as_the_parameter(name):
    """The twin against a direct evaluation: Ext is the oracle's parameter, Adam runs over ALL of Ext, and only the slot rows
    are taken.  Adam is elementwise, so the slot rows of that run are the twin's E bit for bit; the loss is the oracle's data
    term plus lambda / (2B) sum(E E) over the slots; nothing frozen is written."""
    c = RC.make_case(name)
    B = c['B']
    before = [c[k].copy() for k in ('Rw', 'Re', 'W', 'b', 'New0')]
    tw = RC.RefreshTwin(c)
    ext = np.concatenate([c['Re'], np.zeros((c['num_new'], c['de']), np.float32)])
    ext[c['ext_of_slot']] = c['E0']
    assert np.array_equal(ext, np.concatenate([c['Re'], c['New0']]))
    opt = O.Adam([ext], lr=c['lr'])
    for s in range(RC.STEPS):
        sl = slice(s * B, (s + 1) * B)
        ora = O.VectorSpaceOracle(B, c['n'], c['z'], c['Rw'], ext, c['W'], c['b'], c['lam'])
        _, grads, _ = ora.loss_and_grads(c['X'][sl], c['ext_of_slot'][c['y'][sl]], c['w'][sl], c['neg'][s])
        data, _, _ = O.VectorSpaceOracle(B, c['n'], c['z'], c['Rw'], ext, c['W'], c['b'], 0.0).loss_and_grads(
            c['X'][sl], c['ext_of_slot'][c['y'][sl]], c['w'][sl], c['neg'][s])
        E = ext[c['ext_of_slot']].astype(np.float64)
        loss = tw.train_step(s, c['neg'][s])
        assert abs(float(loss) - (float(data) + c['lam'] / (2.0 * B) * float((E * E).sum()))) <= 1e-6 * abs(float(loss))
        # the frozen rows move in this direct run (dense Adam over Ext); put them back: the contract freezes them
        moved = ext.copy()
        opt.update([moved], [grads[0]])
        ext[c['ext_of_slot']] = moved[c['ext_of_slot']]
        assert np.array_equal(tw.E, ext[c['ext_of_slot']]) and np.array_equal(tw.m, opt.m[0][c['ext_of_slot']])
        assert np.array_equal(tw.ext(), ext)
    assert tw.opt.t == RC.STEPS and not np.array_equal(tw.E, c['E0'])
    for k, b in zip(('Rw', 'Re', 'W', 'b', 'New0'), before):
        assert np.array_equal(c[k], b), k
    # ... and it is the shared reference
    ref = RC.case_reference(name, np.float32)
    assert np.array_equal(ref[1]['E'], tw.E) and np.array_equal(ref[1]['v'], tw.v)


def test_row_bound_tells_slot_order_from_id_order():
    """order_and_edges with the slots in id order ([0, 3, 7]) in place of the order given ([7, 0, 3]): the same rows in another
    order.  The row-wise bound of the GPU test (tests.util.check_tensor, the bounds of tests/test_gpu_foldin_keys.py) refuses
    it, for the gradient after step 1 and for E after step 2; the right order passes against itself."""
    c = RC.make_case('order_and_edges')
    r32, r64 = RC.case_reference('order_and_edges', np.float32), RC.case_reference('order_and_edges', np.float64)
    wrong = RC.RefreshTwin(c, ext_of_slot=np.sort(c['ext_of_slot']))
    # (y names a slot: with another slot order the same y would name other entities -- keep the ENTITIES, as a handle that
    #  stored its rows in id order would)
    perm = np.argsort(c['ext_of_slot'], kind='stable')              # wrong slot -> right slot
    right_to_wrong = np.argsort(perm)
    wrong.c = dict(c, y=right_to_wrong[c['y']].astype(np.int32))
    states = []
    for s in range(RC.STEPS):
        wrong.train_step(s, c['neg'][s])
        states.append(dict(E=wrong.E.copy(), m=wrong.m.copy()))
    assert np.array_equal(states[1]['E'][right_to_wrong], r32[1]['E'])    # the same rows ...
    for s, key in ((0, 'm'), (1, 'E')):
        U.check_tensor('right', r32[s][key], r32[s][key], r64[s][key])
        # ... in an order the row bounds refuse, against either twin (check_tensor stops at its first bound, so ask row_err)
        assert U.row_err(states[s][key], r32[s][key])[0] > 100 * U.ROW_TOL32
        assert U.row_err(states[s][key], r64[s][key])[0] > 100 * U.ROW_TOL64
        with pytest.raises(AssertionError):
            U.check_tensor('id order', states[s][key], r32[s][key], r64[s][key])


# ---- the host side of bin/fold_in.py --refresh --------------------------------------------------------------------------

def _meta(Ve=4):
    words = {'w%d' % i: types.SimpleNamespace(id=i) for i in range(9)}
    tokens = {i: 'w%d' % i for i in range(9)}
    return [types.SimpleNamespace(window_size=4), words, tokens, {i: 'E%d' % i for i in range(Ve)},
            {'E%d' % i: ['D%d' % i] for i in range(Ve)}]


def test_merge_meta_on_real_pickles(tmp_path):
    foldin.write_meta(str(tmp_path / 'meta'), _meta())
    meta = foldin.read_meta(str(tmp_path / 'meta'))
    ids = ['F0', 'E2', 'F1', 'E0']              # entity k of the new documents' meta: new, known, new, known
    merged, refreshed, new_ids, slots = foldin.merge_meta(meta, ids, {'F0': ['N0'], 'E2': ['N1', 'N2'], 'F1': [], 'E0': ['N3']})
    assert refreshed.tolist() == [2, 0] and refreshed.dtype == np.int32 and new_ids == ['F0', 'F1']
    assert slots.tolist() == [2, 0, 3, 1]                                  # refreshed slots first, in order of appearance
    assert merged[3] == {0: 'E0', 1: 'E1', 2: 'E2', 3: 'E3', 4: 'F0', 5: 'F1'}
    assert merged[4]['E2'] == ['D2', 'N1', 'N2'] and merged[4]['E0'] == ['D0', 'N3'] and merged[4]['E1'] == ['D1']
    assert merged[4]['F0'] == ['N0'] and merged[4]['F1'] == []
    assert len(meta[3]) == 4 and meta[4]['E2'] == ['D2']                    # the input is not changed
    assert merged[1] == meta[1] and merged[2] == meta[2]
    foldin.write_meta(str(tmp_path / 'meta_out'), merged)
    assert foldin.read_meta(str(tmp_path / 'meta_out'))[3] == merged[3]
    # nothing new: V_e is unchanged
    merged, refreshed, new_ids, slots = foldin.merge_meta(meta, ['E3', 'E1'])
    assert merged[3] == meta[3] and refreshed.tolist() == [3, 1] and new_ids == [] and slots.tolist() == [0, 1]
    with pytest.raises(RuntimeError, match='duplicate'):
        foldin.merge_meta(meta, ['E1', 'F0', 'E1'])
    # extend_meta still refuses a known id
    with pytest.raises(RuntimeError, match='already in the trained model'):
        foldin.extend_meta(meta, ['F0', 'E2'])


def test_refresh_dump_replaces_in_place_and_appends():
    rng = np.random.RandomState(2)
    R_e = rng.randn(5, 3).astype(np.float32)
    keep = R_e.copy()
    rows, new = rng.randn(2, 3).astype(np.float32), rng.randn(1, 3).astype(np.float32)
    out = foldin.refresh_dump('args', 'predict', 'R_w', R_e, [4, 1], rows, new)
    assert out[:3] == ['args', 'predict', 'R_w'] and out[3].shape == (6, 3) and np.array_equal(R_e, keep)
    assert np.array_equal(out[3][[4, 1]], rows) and np.array_equal(out[3][[0, 2, 3]], keep[[0, 2, 3]]) and np.array_equal(out[3][5:], new)
    out = foldin.refresh_dump('args', 'predict', 'R_w', R_e, [0], rows[:1], np.zeros((0, 3), np.float32))
    assert out[3].shape == (5, 3)


def test_parser_has_refresh_off_by_default():
    spec = importlib.util.spec_from_file_location('fold_in_cli', os.path.join(ROOT, 'bin', 'fold_in.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    need = ['--meta', __file__, '--model', __file__, '--new_meta', __file__, '--data', __file__, '--iterations', '1',
            '--model_output', os.path.join(ROOT, 'no_such_model'), '--meta_output', os.path.join(ROOT, 'no_such_meta')]
    assert parser.parse_args(need).refresh is False
    assert parser.parse_args(need + ['--refresh']).refresh is True
    assert 'old documents' in parser.format_help() and 'old documents' in mod.__doc__


def test_binding_lists_the_refresh_symbols(hip_lib):
    """The new constructor is declared in include/sert_hip_foldin.h, the new hook in include/sert_hip_debug.h; the binding lists
    both and the library exports them; without a model both refuse with a message (no device)."""
    import ctypes
    src = open(os.path.join(ROOT, 'include', 'sert_hip_foldin.h')).read()
    assert re.search(r'\bint sert_foldin_create_refresh\(', src) and 'sert_foldin_create_refresh' in _capi.EXPORTS_FOLDIN
    assert 'sert_debug_foldin_table' in open(os.path.join(ROOT, 'include', 'sert_hip_debug.h')).read()
    assert 'sert_debug_foldin_table' in _capi.EXPORTS
    cfg = _capi.SertFoldInConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    h = ctypes.c_void_p()
    assert hip_lib.sert_foldin_create_refresh(None, None, 0, 1, None, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'null argument' in hip_lib.sert_last_error()
    v = (ctypes.c_int32 * 4)()
    hip_lib.sert_debug_foldin_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    assert hip_lib.sert_debug_foldin_table(None, v, 4) != 0
    assert b'bad argument' in hip_lib.sert_last_error()
