"""GPU: the command-line chain of a loglinear fold-in in which trained entities GAIN documents, on the product-search fixture
as tests/test_gpu_ll_foldin_labels_cli.py builds it: bin/train.py --type loglinear on 300 products; new documents for the
other 38 AND for some of the 300; bin/prepare.py --vocabulary_from, bin/fold_in.py --unfreeze_known with and without
--label_distributions, bin/query.py.  The known ids' columns learn in place, every other trained column keeps its bits."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import foldin, models, training
from sert_amd.utils import trec_utils
from tests.test_gpu_foldin_cli import GOLD, NUM_NEW, ROOT, _corpora

pytestmark = pytest.mark.gpu

NUM_KNOWN = 5               # trained products that gain documents: one of their own each, and a share of some new products'


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_unfreeze_known(hip_lib, tmp_path):
    products, new = _corpora(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    P = lambda name: str(tmp_path / name)

    def run(script, *args, **kw):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', script)] + list(args) + ['--loglevel', 'ERROR'], env=env,
                              check=kw.get('check', True), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)

    # the new corpus: the new products' documents, the first of each co-owned by one of NUM_KNOWN trained products, and one
    # document of its own for each of those; `gain`: the same without any new product
    known = products[:NUM_KNOWN]
    with open(os.path.join(GOLD, 'topics')) as f:
        words = ' '.join(trec_utils.parse_topics(f).values()).split()
    rng = np.random.RandomState(1)
    docs = (tmp_path / 'new.trectext').read_text()
    lines = [line for line in (tmp_path / 'new.assocs').read_text().split('\n') if line]
    own_docs, own_lines, shared = [], [], {}
    for k, e in enumerate(known):
        own_docs.append('<DOC>\n<DOCNO> K%04d </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n' % (k, ' '.join(rng.choice(words, 22).tolist())))
        own_lines.append('%s K%04d 1' % (e, k))
    for k, line in enumerate(line for line in lines if line.split()[1].endswith('_0')):
        shared.setdefault(known[k % NUM_KNOWN], []).append(line.split()[1])
    co_lines = ['%s %s 1' % (e, doc) for e in known for doc in shared[e]]
    (tmp_path / 'mix.trectext').write_text(docs + ''.join(own_docs))
    (tmp_path / 'mix.assocs').write_text('\n'.join(lines + co_lines + own_lines) + '\n')
    (tmp_path / 'gain.trectext').write_text(''.join(own_docs))
    (tmp_path / 'gain.assocs').write_text('\n'.join(own_lines) + '\n')

    prep = ['--window_size', '4', '--overlapping', '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1',
            '--no_instance_weights']
    run('prepare.py', '--seed', '3', P('old.trectext'), '--assoc_path', P('old.assocs'), '--meta_output', P('meta'),
        '--data_output', P('data.npz'), *prep)
    run('train.py', '--data', P('data.npz'), '--meta', P('meta'), '--type', 'loglinear', '--iterations', '2', '--batch_size',
        '64', '--word_representation_size', '16', '--regularization_lambda', '0.01', '--model_output', P('model'), '--seed', '1')
    for name in ('mix', 'gain'):
        run('prepare.py', '--seed', '3', P(name + '.trectext'), '--assoc_path', P(name + '.assocs'), '--vocabulary_from', P('meta'),
            '--meta_output', P(name + '_meta'), '--data_output', P(name + '.npz'), *prep)

    def fold(data, *flags, **kw):
        out = kw.pop('out')
        return run('fold_in.py', '--meta', kw.pop('meta', P('meta')), '--model', kw.pop('model', P('model_2.bin')), '--new_meta',
                   kw.pop('new_meta', P(data + '_meta')), '--data', P(data + '.npz'), '--iterations', '3', '--batch_size', '16',
                   '--seed', '1', '--model_output', P('model_%s.bin' % out), '--meta_output', P('meta_' + out), *flags, **kw)

    meta, mix_meta = foldin.read_meta(P('meta')), foldin.read_meta(P('mix_meta'))
    V_e = len(meta[3])
    assert V_e == len(products) - NUM_NEW and set(mix_meta[3].values()) == new | set(known)
    index_of = dict((e, i) for i, e in meta[3].items())
    refreshed = sorted(index_of[e] for e in known)
    untouched = np.setdiff1d(np.arange(V_e), refreshed)
    old = training.read_checkpoint(P('model_2.bin'))
    W, b = np.asarray(old['predict_fn'].W), np.asarray(old['predict_fn'].b)

    def check(out, new_meta, num_new, query=True):
        """the output dump and meta of a run: untouched columns bit for bit, refreshed ones moved, new ones appended"""
        ext, meta_out = training.read_checkpoint(P('model_%s.bin' % out)), foldin.read_meta(P('meta_' + out))
        assert ext['args'].type is models.LanguageModel and len(ext['tables']) == 1
        assert np.array_equal(_bits(ext['tables'][0]), _bits(old['tables'][0]))                     # R_w
        Wx, bx = np.asarray(ext['predict_fn'].W), np.asarray(ext['predict_fn'].b)
        assert Wx.shape == (16, V_e + num_new) and bx.shape == (V_e + num_new,)
        assert np.array_equal(_bits(Wx[:, untouched]), _bits(W[:, untouched])) and np.array_equal(_bits(bx[untouched]), _bits(b[untouched]))
        assert np.isfinite(Wx).all() and np.isfinite(bx).all()
        for e in refreshed:
            assert not np.array_equal(_bits(Wx[:, e]), _bits(W[:, e])) and bx[e] != b[e], e
        if num_new:
            assert np.abs(bx[V_e:]).max() > 0                      # (the new biases start at zero: they learnt)
        # merge_meta's meta: every trained id keeps its index, the unknown ids follow, the associations gained the documents
        assert len(meta_out[3]) == V_e + num_new and meta_out[1] == meta[1]
        assert all(meta_out[3][i] == meta[3][i] for i in range(V_e))
        assert set(meta_out[3][i] for i in range(V_e, V_e + num_new)) == (new if num_new else set())
        for e in known:
            gained = list(new_meta[4][e])
            assert gained and list(meta_out[4][e]) == list(meta[4][e]) + gained
        assert all(list(meta_out[4][e]) == list(meta[4][e]) for e in meta[3].values() if e not in known)
        if not query:
            return Wx, bx
        run('query.py', '--meta', P('meta_' + out), '--model', P('model_%s.bin' % out), '--topics', os.path.join(GOLD, 'topics'),
            '--run_out', P('run_' + out))
        with open(P('run_%s_ef' % out)) as f:
            ranking = trec_utils.parse_run(f)
        want = set(meta_out[3].values())
        assert ranking and all(set(e for _, e in entries) == want and len(entries) == len(want) for entries in ranking.values())
        return Wx, bx

    # label distributions: a document of a new product and a known one is ONE instance with two labels
    y = training.load_data_sets(P('mix.npz'))[0][1]
    assert (np.diff(y.tocsr().indptr) > 1).any()
    fold('mix', '--unfreeze_known', '--label_distributions', out='rows')
    Wa, _ = check('rows', mix_meta, NUM_NEW)
    # one instance per label
    fold('mix', '--unfreeze_known', out='onehot')
    Wb, _ = check('onehot', mix_meta, NUM_NEW)
    assert not np.array_equal(Wa, Wb)                              # (two different losses)
    # no new id at all: V_e is unchanged
    gain_meta = foldin.read_meta(P('gain_meta'))
    assert set(gain_meta[3].values()) == set(known)
    fold('gain', '--unfreeze_known', out='gain')
    check('gain', gain_meta, 0, query=False)               # (the same V_e entities as the trained dump)

    # ---- the refusals: nothing is written ----
    def refused(result, message, out):
        assert result.returncode != 0 and message in result.stdout, result.stdout[-600:]
        assert not os.path.exists(P('model_%s.bin' % out)) and not os.path.exists(P('meta_' + out))

    # nothing known together with nothing new: a meta that names no entity
    foldin.write_meta(P('empty_meta'), mix_meta[:3] + [{}, {}])
    refused(fold('mix', '--unfreeze_known', new_meta=P('empty_meta'), out='n', check=False), b'nothing to fold in', 'n')
    # --refresh stays the vectorspace flag, and says where to go
    ref = fold('mix', '--refresh', out='r', check=False)
    refused(ref, b'--refresh needs a vectorspace model', 'r')
    assert b'--unfreeze_known' in ref.stdout
    # a vectorspace dump with --unfreeze_known is refused and pointed to --refresh
    rng = np.random.RandomState(5)
    de = 8
    vs_args = argparse.Namespace(type=models.VectorSpaceLanguageModel)
    Wv, bv = rng.uniform(-0.3, 0.3, (16, de)).astype(np.float32), np.zeros(de, np.float32)
    R_e = rng.uniform(-0.3, 0.3, (V_e, de)).astype(np.float32)
    foldin.write_dump(P('vs.bin'), [vs_args, models.VectorSpacePredictFn(W=Wv, b=bv), old['tables'][0], R_e])
    vs = fold('mix', '--unfreeze_known', model=P('vs.bin'), out='vs', check=False)
    refused(vs, b'--unfreeze_known needs a loglinear model', 'vs')
    assert b'--refresh' in vs.stdout
