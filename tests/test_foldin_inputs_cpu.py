"""CPU: the inputs of the fold-in tests have the structure they exist for (tests/foldin_cases.py), the twin does what the
contract says, ``bin/prepare.py --vocabulary_from`` gives the trained model's token ids, and the writers of bin/fold_in.py
extend the dump and the meta consistently.  No device."""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle import sert_oracle as O
from sert_amd import _capi, foldin
from tests import foldin_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16           # kEChunk (csrc/kernels_egrad.h): sorted pairs per chunk of the reduction


def _sorted_keys(c, s):
    return np.sort(FC.keys_of_step(c, s), kind='stable')


@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_case_has_its_structure(name):
    c = FC.make_case(name)
    B, Ve, N, z = c['B'], c['Ve'], c['N'], c['z']
    assert c['neg'].shape == (FC.STEPS, B, z) and c['neg'].min() >= 0 and c['neg'].max() < Ve + N
    assert c['y'].min() >= 0 and c['y'].max() < N and c['X'].max() < c['Vw']
    assert c['M'] % B != 0 and c['M'] // B == c['batches'] >= FC.STEPS      # a tail that is never visited
    for s in range(FC.STEPS):
        keys = FC.keys_of_step(c, s)
        counts = np.bincount(keys, minlength=N + 1)
        live, sentinel = counts[:N], counts[N]
        assert live.sum() >= B                          # every positive hits a new row
        if name == 'base':
            assert sentinel > 0 and live.sum() > B      # negatives on frozen AND on new rows
            assert live.max() >= 2
            if s == 0:
                assert np.bincount(c['y'][:B], minlength=N)[N - 1] == 0
        elif name == 'ragged':
            assert B % 16 != 0
        elif name == 'wide':
            assert c['de'] % 4 == 0 and c['de'] // 4 > 16
        elif name == 'odd_de':
            assert c['de'] % 4 != 0
        elif name == 'many_cands':
            assert z + 1 > 16
        elif name == 'one_entity':
            assert N == 1 and live[0] >= B + 1
            assert live[0] > 3 * CHUNK and live[0] % CHUNK != 0     # many chunks; the sentinel run starts inside a chunk
            assert sentinel > CHUNK
        elif name == 'all_frozen':
            assert live.sum() == B and sentinel == B * z
        elif name == 'all_new':
            assert sentinel == 0 and live.sum() == B * (z + 1)
        elif name == 'two_digits':
            assert N + 1 > 2048 and (live == 0).sum() > N // 2
            assert keys.max() == N                       # the sentinel itself needs the second digit
        elif name == 'target_as_negative':
            yb = Ve + c['y'][s * B:(s + 1) * B]
            assert (c['neg'][s] == yb[:, None]).any(axis=1).sum() >= B // 3
        # sorted, the sentinel run is the END of the order
        sk = _sorted_keys(c, s)
        assert np.all(sk[:live.sum()] < N) and np.all(sk[live.sum():] == N)


def test_twin_follows_the_contract():
    """The twin on the base case, against a direct use of the oracle on the extended table: the gradient of the frozen
    rows is dropped, the new rows' is the oracle's, the loss is the data term plus lambda / (2B) sum(E E), and frozen
    inputs are not written."""
    c = FC.make_case('base')
    tw = FC.FoldInTwin(c)
    before = [c[k].copy() for k in ('Rw', 'Re', 'W', 'b', 'E0')]
    B, Ve = c['B'], c['Ve']
    ext = np.concatenate([c['Re'], c['E0']])
    ora = O.VectorSpaceOracle(B, c['n'], c['z'], c['Rw'], ext, c['W'], c['b'], 0.0)
    data, grads, _ = ora.loss_and_grads(c['X'][:B], Ve + c['y'][:B].astype(np.int64), c['w'][:B], c['neg'][0])
    loss = tw.train_step(0, c['neg'][0])
    reg = c['lam'] / (2.0 * B) * float((c['E0'].astype(np.float64) ** 2).sum())
    assert abs(float(loss) - (float(data) + reg)) <= 1e-6 * abs(float(loss))
    g = grads[0][Ve:] + np.float32(c['lam'] / B) * c['E0']
    assert np.allclose(tw.m, 0.1 * g, rtol=1e-5, atol=1e-9)             # Adam's first moment after one step from zero
    assert tw.opt.t == 1 and not np.array_equal(tw.E, c['E0'])
    for k, b in zip(('Rw', 'Re', 'W', 'b', 'E0'), before):
        assert np.array_equal(c[k], b), k
    ev = tw.eval_loss(1, c['eval_neg'])
    E1 = tw.E.copy()
    assert np.isfinite(ev) and np.array_equal(tw.E, E1)


def test_binding_lists_the_foldin_symbols(hip_lib):
    """include/sert_hip_foldin.h, which sert_hip.h includes, declares exactly _capi.EXPORTS_FOLDIN; the library exports
    them; the config struct of the binding has the header's size."""
    import re
    src = open(os.path.join(ROOT, 'include', 'sert_hip_foldin.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(sert_foldin_[a-z_0-9]+)\s*\(', src)))
    assert declared == sorted(_capi.EXPORTS_FOLDIN)
    assert '#include "sert_hip_foldin.h"' in open(os.path.join(ROOT, 'include', 'sert_hip.h')).read()
    assert not [s for s in _capi.EXPORTS_FOLDIN if not hasattr(hip_lib, s)]
    assert not set(_capi.EXPORTS_FOLDIN) & set(_capi.EXPORTS)
    import ctypes
    assert ctypes.sizeof(_capi.SertFoldInConfig) == 40
    # no device: a null model is refused with a message
    cfg = _capi.SertFoldInConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    h = ctypes.c_void_p()
    assert hip_lib.sert_foldin_create(None, 1, None, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b'null argument' in hip_lib.sert_last_error()


# ---- prepare --vocabulary_from -----------------------------------------------------------------------------------------

def _doc(name, text):
    return '<DOC>\n<DOCNO> %s </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n' % (name, text)


def _prepare(tmp_path, docs, assocs, meta, data, extra=()):
    (tmp_path / (meta + '.trectext')).write_text(''.join(docs))
    (tmp_path / (meta + '.assocs')).write_text('\n'.join(assocs) + '\n')
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'prepare.py'), '--seed', '3', str(tmp_path / (meta + '.trectext')),
           '--assoc_path', str(tmp_path / (meta + '.assocs')), '--window_size', '4', '--vocabulary_min_count', '1',
           '--validation_set_ratio', '0.2', '--meta_output', str(tmp_path / meta), '--data_output', str(tmp_path / data),
           '--loglevel', 'ERROR'] + list(extra)
    subprocess.check_call(cmd)
    return np.load(str(tmp_path / data), allow_pickle=True), foldin.read_meta(str(tmp_path / meta))


def test_prepare_vocabulary_from_gives_the_trained_ids(tmp_path):
    rng = np.random.RandomState(0)
    old_words = 'alpha beta gamma delta kappa lambda sigma omega'.split()
    docs = [_doc('D%02d' % d, ' '.join(rng.choice(old_words, size=20))) for d in range(8)]
    assocs = ['E%d D%02d 1' % (d % 2, d) for d in range(8)]
    _, old_meta = _prepare(tmp_path, docs, assocs, 'meta', 'data.npz')
    words = old_meta[1]
    # new documents: known words in an order that would give them OTHER ids if a vocabulary were extracted, and words the
    # trained model never saw
    new_docs = [_doc('N%02d' % d, ' '.join(['omega'] * 9 + ['zulu', 'yankee'] * 3 + ['alpha'] * 2 + ['sigma'] * 5))
                for d in range(4)]
    new_assocs = ['F%d N%02d 1' % (d % 2, d) for d in range(4)]
    data, new_meta = _prepare(tmp_path, new_docs, new_assocs, 'new_meta', 'new.npz', ['--vocabulary_from', str(tmp_path / 'meta')])
    assert new_meta[1] == words and new_meta[2] == old_meta[2]            # the meta's words: identical
    assert new_meta[0].vocabulary_from == str(tmp_path / 'meta')
    assert not hasattr(old_meta[0], 'vocabulary_from')                     # (the flag is absent unless given)
    assert set(new_meta[3].values()) == {'F0', 'F1'}
    x = np.concatenate([data['x_train'], data['x_validate']])
    seen = set(np.unique(x).tolist())
    assert seen == {words[w].id for w in ('omega', 'alpha', 'sigma')}     # the OLD ids; OOV tokens dropped
    # 16 in-vocabulary tokens per document -> four full windows each: an OOV token leaves no gap and no padding
    assert x.shape == (16, 4)
    # without the flag the same documents get a vocabulary of their own, with other ids
    _, own = _prepare(tmp_path, new_docs, new_assocs, 'own_meta', 'own.npz')
    assert 'zulu' in own[1] and any(own[1][w].id != words[w].id for w in ('omega', 'alpha', 'sigma'))


# ---- the writers of bin/fold_in.py ----------------------------------------------------------------------------------

def test_writers_extend_the_index_and_the_table(tmp_path):
    rng = np.random.RandomState(1)
    Vw, Ve, N, dw, de = 9, 4, 3, 5, 6
    words = {'w%d' % i: types.SimpleNamespace(id=i) for i in range(Vw)}
    tokens = {i: 'w%d' % i for i in range(Vw)}
    meta = [types.SimpleNamespace(window_size=4), words, tokens, {i: 'E%d' % i for i in range(Ve)},
            {'E%d' % i: ['D%d' % i] for i in range(Ve)}]
    R_w, R_e = rng.randn(Vw, dw).astype(np.float32), rng.randn(Ve, de).astype(np.float32)
    new_rows = rng.randn(N, de).astype(np.float32)
    new_ids = ['F0', 'F1', 'F2']
    ext = foldin.extend_meta(meta, new_ids, {'F0': ['N0', 'N1'], 'F2': ['N2']})
    assert ext[1] is words and ext[2] is tokens
    assert ext[3] == {0: 'E0', 1: 'E1', 2: 'E2', 3: 'E3', 4: 'F0', 5: 'F1', 6: 'F2'}
    assert ext[4]['F0'] == ['N0', 'N1'] and ext[4]['E2'] == ['D2'] and len(meta[3]) == Ve       # the input is not changed
    with pytest.raises(RuntimeError, match='already in the trained model'):
        foldin.extend_meta(meta, ['F0', 'E1'])
    with pytest.raises(RuntimeError, match='duplicate'):
        foldin.extend_meta(meta, ['F0', 'F0'])
    args = types.SimpleNamespace(batch_size=8)
    predict = {'W': rng.randn(dw, de).astype(np.float32)}
    objects = foldin.extend_dump(args, predict, R_w, R_e, new_rows)
    foldin.write_dump(str(tmp_path / 'model.bin'), objects)
    foldin.write_meta(str(tmp_path / 'meta'), ext)
    with open(str(tmp_path / 'model.bin'), 'rb') as f:
        back = [pickle.load(f) for _ in range(4)]
    assert back[0].batch_size == 8 and np.array_equal(back[1]['W'], predict['W']) and np.array_equal(back[2], R_w)
    assert back[3].shape == (Ve + N, de) and back[3].dtype == np.float32
    assert np.array_equal(back[3][:Ve], R_e) and np.array_equal(back[3][Ve:], new_rows)
    meta_back = foldin.read_meta(str(tmp_path / 'meta'))
    # row i of the table is the entity the index names i
    assert len(meta_back[3]) == back[3].shape[0] and [meta_back[3][Ve + e] for e in range(N)] == new_ids
