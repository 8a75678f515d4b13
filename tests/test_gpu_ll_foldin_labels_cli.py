"""GPU: the command-line chain of a loglinear fold-in on label DISTRIBUTIONS, on the product-search fixture as
tests/test_gpu_ll_foldin_cli.py builds it: bin/train.py --type loglinear WITHOUT --one_hot_classes on 300 products; new
documents of which some belong to a new product AND a trained one; bin/prepare.py --vocabulary_from, bin/fold_in.py
--label_distributions, bin/query.py.  The trained co-labels stay frozen and keep their index; only the unknown ids are new."""
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

NUM_CO = 5                  # trained products that co-own new documents


def test_label_distributions_with_trained_co_labels(hip_lib, tmp_path):
    products, new = _corpora(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    P = lambda name: str(tmp_path / name)

    def run(script, *args, **kw):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', script)] + list(args) + ['--loglevel', 'ERROR'], env=env,
                              check=kw.get('check', True), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)

    # the new association file: the first document of every new product also belongs to one of NUM_CO trained products
    co = products[:NUM_CO]
    lines = (tmp_path / 'new.assocs').read_text().split('\n')
    lines = [line for line in lines if line]
    shared = {}
    for k, line in enumerate(line for line in lines if line.split()[1].endswith('_0')):
        shared.setdefault(co[k % NUM_CO], []).append(line.split()[1])
    assert len(shared) == NUM_CO and sum(len(v) for v in shared.values()) == NUM_NEW
    (tmp_path / 'co.assocs').write_text('\n'.join(lines + ['%s %s 1' % (e, doc) for e in co for doc in shared[e]]) + '\n')

    prep = ['--window_size', '4', '--overlapping', '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1',
            '--no_instance_weights']
    run('prepare.py', '--seed', '3', P('old.trectext'), '--assoc_path', P('old.assocs'), '--meta_output', P('meta'),
        '--data_output', P('data.npz'), *prep)
    # (no --one_hot_classes: the model learns from label distributions)
    run('train.py', '--data', P('data.npz'), '--meta', P('meta'), '--type', 'loglinear', '--iterations', '2', '--batch_size',
        '64', '--word_representation_size', '16', '--regularization_lambda', '0.01', '--model_output', P('model'), '--seed', '1')
    run('prepare.py', '--seed', '3', P('new.trectext'), '--assoc_path', P('co.assocs'), '--vocabulary_from', P('meta'),
        '--meta_output', P('new_meta'), '--data_output', P('new.npz'), *prep)
    fold = ['fold_in.py', '--meta', P('meta'), '--model', P('model_2.bin'), '--new_meta', P('new_meta'), '--data', P('new.npz'),
            '--iterations', '3', '--batch_size', '64', '--seed', '1']
    run(*fold, '--label_distributions', '--model_output', P('model_ext.bin'), '--meta_output', P('meta_ext'))
    run('query.py', '--meta', P('meta_ext'), '--model', P('model_ext.bin'), '--topics', os.path.join(GOLD, 'topics'),
        '--run_out', P('run'))

    meta, new_meta, meta_ext = foldin.read_meta(P('meta')), foldin.read_meta(P('new_meta')), foldin.read_meta(P('meta_ext'))
    V_e = len(meta[3])
    assert V_e == len(products) - NUM_NEW
    # the new documents' meta names the co-labels too, and its label rows hold more than one entry
    assert set(new_meta[3].values()) == new | set(co)
    y = training.load_data_sets(P('new.npz'))[0][1]
    assert (np.diff(y.tocsr().indptr) > 1).any() and (np.diff(y.tocsr().indptr) == 1).any()
    # N = the unknown ids only; every trained id keeps its index, the co-labels among them
    assert len(meta_ext[3]) == len(products) and meta_ext[1] == meta[1]
    assert all(meta_ext[3][i] == meta[3][i] for i in range(V_e))
    assert set(meta_ext[3][i] for i in range(V_e, len(products))) == new
    for e in co:
        gained = list(new_meta[4][e])
        assert gained and list(meta_ext[4][e]) == list(meta[4][e]) + gained           # the co-labels gained the new documents
    assert all(meta_ext[4][e] for e in new)
    assert all(list(meta_ext[4][e]) == list(meta[4][e]) for e in meta[3].values() if e not in co)
    # the extended dump: W (d, V_e + N) and b (V_e + N); trained columns and R_w bit for bit
    old, ext = training.read_checkpoint(P('model_2.bin')), training.read_checkpoint(P('model_ext.bin'))
    assert ext['args'].type is models.LanguageModel and len(ext['tables']) == 1
    assert np.array_equal(ext['tables'][0].view(np.uint32), old['tables'][0].view(np.uint32))
    W, b, Wx, bx = old['predict_fn'].W, old['predict_fn'].b, ext['predict_fn'].W, ext['predict_fn'].b
    assert Wx.shape == (16, V_e + NUM_NEW) and bx.shape == (V_e + NUM_NEW,)
    assert np.array_equal(np.ascontiguousarray(Wx[:, :V_e]).view(np.uint32), np.ascontiguousarray(W).view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(bx[:V_e]).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert np.isfinite(Wx).all() and np.abs(bx[V_e:]).max() > 0             # (the new biases start at zero: they learnt)
    with open(P('run_ef')) as f:
        ranking = trec_utils.parse_run(f)
    assert ranking and all(len(entries) == len(products) for entries in ranking.values())     # every entity, old and new
    assert all(set(products) == set(e for _, e in entries) for entries in ranking.values())
    # without the flag nothing changes: the known ids are refused, and nothing is written
    again = run(*fold, '--model_output', P('model_x.bin'), '--meta_output', P('meta_x'), check=False)
    assert again.returncode != 0 and b'entity ids already in the trained model' in again.stdout
    assert not os.path.exists(P('model_x.bin')) and not os.path.exists(P('meta_x'))
    # nothing to fold in: every id of the new meta is known to the EXTENDED meta
    none = run('fold_in.py', '--meta', P('meta_ext'), '--model', P('model_ext.bin'), *fold[5:], '--label_distributions',
               '--model_output', P('model_n.bin'), '--meta_output', P('meta_n'), check=False)
    assert none.returncode != 0 and b'nothing to fold in' in none.stdout
    assert not os.path.exists(P('model_n.bin')) and not os.path.exists(P('meta_n'))
    # --refresh stays refused on a loglinear dump
    ref = run(*fold, '--label_distributions', '--refresh', '--model_output', P('model_r.bin'), '--meta_output', P('meta_r'),
              check=False)
    assert ref.returncode != 0 and b'--refresh needs a vectorspace model' in ref.stdout
    assert not os.path.exists(P('model_r.bin')) and not os.path.exists(P('meta_r'))
    # --label_distributions on a vectorspace dump is refused, and nothing is written
    rng = np.random.RandomState(5)
    de = 8
    vs_args = argparse.Namespace(type=models.VectorSpaceLanguageModel)
    Wv, bv = rng.uniform(-0.3, 0.3, (16, de)).astype(np.float32), np.zeros(de, np.float32)
    R_e = rng.uniform(-0.3, 0.3, (V_e, de)).astype(np.float32)
    foldin.write_dump(P('vs.bin'), [vs_args, models.VectorSpacePredictFn(W=Wv, b=bv), old['tables'][0], R_e])
    vs = run('fold_in.py', '--meta', P('meta'), '--model', P('vs.bin'), *fold[5:], '--label_distributions', '--model_output',
             P('vs_ext.bin'), '--meta_output', P('vs_meta_ext'), check=False)
    assert vs.returncode != 0 and b'--label_distributions needs a loglinear model' in vs.stdout
    assert not os.path.exists(P('vs_ext.bin')) and not os.path.exists(P('vs_meta_ext'))
