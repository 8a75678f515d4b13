"""GPU: the command-line chain of a LOGLINEAR fold-in on the product-search fixture (tests/golden/product_search):
bin/prepare.py and bin/train.py --type loglinear on 300 of its products, bin/prepare.py --vocabulary_from and bin/fold_in.py
for the other 38, bin/query.py on the extended dump and meta; --refresh is refused on that dump; a vectorspace dump still
takes bin/fold_in.py's vectorspace path."""
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


def test_loglinear_fold_in_then_query_ranks_the_new_products(hip_lib, tmp_path):
    products, new = _corpora(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    P = lambda name: str(tmp_path / name)

    def run(script, *args, **kw):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', script)] + list(args) + ['--loglevel', 'ERROR'], env=env,
                              check=kw.get('check', True), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)

    prep = ['--window_size', '4', '--overlapping', '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1',
            '--no_instance_weights']
    run('prepare.py', '--seed', '3', P('old.trectext'), '--assoc_path', P('old.assocs'), '--meta_output', P('meta'),
        '--data_output', P('data.npz'), *prep)
    run('train.py', '--data', P('data.npz'), '--meta', P('meta'), '--type', 'loglinear', '--iterations', '2', '--batch_size',
        '64', '--word_representation_size', '16', '--one_hot_classes', '--regularization_lambda', '0.01', '--model_output',
        P('model'), '--seed', '1')
    run('prepare.py', '--seed', '3', P('new.trectext'), '--assoc_path', P('new.assocs'), '--vocabulary_from', P('meta'),
        '--meta_output', P('new_meta'), '--data_output', P('new.npz'), *prep)
    # (no --num_negative_samples: a loglinear fold-in draws none)
    fold = ['fold_in.py', '--meta', P('meta'), '--model', P('model_2.bin'), '--new_meta', P('new_meta'), '--data', P('new.npz'),
            '--iterations', '3', '--batch_size', '64', '--seed', '1']
    run(*fold, '--model_output', P('model_ext.bin'), '--meta_output', P('meta_ext'))
    run('query.py', '--meta', P('meta_ext'), '--model', P('model_ext.bin'), '--topics', os.path.join(GOLD, 'topics'),
        '--run_out', P('run'))
    meta, meta_ext = foldin.read_meta(P('meta')), foldin.read_meta(P('meta_ext'))
    V_e = len(meta[3])
    assert V_e == len(products) - NUM_NEW and len(meta_ext[3]) == len(products)
    assert set(meta_ext[3][i] for i in range(V_e, len(products))) == new
    assert all(meta_ext[3][i] == meta[3][i] for i in range(V_e)) and meta_ext[1] == meta[1]
    # the extended dump: a loglinear dump whose predict function holds W (d, V_e + N) and b (V_e + N), trained columns untouched
    old, ext = training.read_checkpoint(P('model_2.bin')), training.read_checkpoint(P('model_ext.bin'))
    assert ext['args'].type is models.LanguageModel and len(ext['tables']) == 1
    assert np.array_equal(ext['tables'][0], old['tables'][0])
    W, b, Wx, bx = old['predict_fn'].W, old['predict_fn'].b, ext['predict_fn'].W, ext['predict_fn'].b
    assert Wx.shape == (16, len(products)) and bx.shape == (len(products),)
    assert np.array_equal(Wx[:, :V_e], W) and np.array_equal(bx[:V_e], b)
    assert np.isfinite(Wx).all() and np.abs(bx[V_e:]).max() > 0             # (the new biases start at zero: they learnt)
    with open(P('run_ef')) as f:
        ranking = trec_utils.parse_run(f)
    assert ranking and all(len(entries) == len(products) for entries in ranking.values())     # every entity, old and new
    assert all(new <= set(e for _, e in entries) for entries in ranking.values())
    # --refresh is refused on a loglinear dump, with a message, and nothing is written
    again = run(*fold, '--refresh', '--model_output', P('model_r.bin'), '--meta_output', P('meta_r'), check=False)
    assert again.returncode != 0 and b'--refresh needs a vectorspace model' in again.stdout
    assert not os.path.exists(P('model_r.bin')) and not os.path.exists(P('meta_r'))
    # a vectorspace dump over the same meta still takes the vectorspace path: R_e grows by the new rows, W and b stay
    rng = np.random.RandomState(5)
    Vw, de = old['tables'][0].shape[0], 8
    vs_args = argparse.Namespace(type=models.VectorSpaceLanguageModel)
    Wv, bv = rng.uniform(-0.3, 0.3, (16, de)).astype(np.float32), np.zeros(de, np.float32)
    R_e = rng.uniform(-0.3, 0.3, (V_e, de)).astype(np.float32)
    foldin.write_dump(P('vs.bin'), [vs_args, models.VectorSpacePredictFn(W=Wv, b=bv), old['tables'][0], R_e])
    run('fold_in.py', '--meta', P('meta'), '--model', P('vs.bin'), '--new_meta', P('new_meta'), '--data', P('new.npz'),
        '--iterations', '1', '--batch_size', '64', '--num_negative_samples', '4', '--seed', '1', '--model_output',
        P('vs_ext.bin'), '--meta_output', P('vs_meta_ext'))
    vs_ext = training.read_checkpoint(P('vs_ext.bin'))
    assert vs_ext['args'].type is models.VectorSpaceLanguageModel and len(vs_ext['tables']) == 2
    assert vs_ext['tables'][1].shape == (len(products), de) and np.array_equal(vs_ext['tables'][1][:V_e], R_e)
    assert np.array_equal(vs_ext['predict_fn'].W, Wv) and Vw == vs_ext['tables'][0].shape[0]
