"""GPU: the command-line chain of a WORD fold-in into a LOGLINEAR model on LABEL ROWS, on the product-search fixture
(tests/golden/product_search): bin/prepare.py and bin/train.py --type loglinear WITHOUT --one_hot_classes -- the expert-finding
recipe's loss -- on the products' documents, then new documents of trained products that bring invented words and name two
products each: bin/prepare.py --vocabulary_from META --extend_vocabulary, bin/fold_in.py --ll_new_words --label_rows,
bin/query.py on the extended dump and meta."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import _capi
from sert_amd import foldin, models, training
from sert_amd.utils import trec_utils
from tests.test_gpu_wfold_cli import NEW_WORDS, NUM_GAINING, ROOT, _corpora

pytestmark = pytest.mark.gpu

upload_csr = _capi.LlWordFoldIn.upload_csr      # what --label_rows drives: without it there is no chain to test


def test_loglinear_word_fold_in_on_label_rows_then_query_answers_in_a_new_word(hip_lib, tmp_path):
    products, topics = _corpora(tmp_path)
    # every new document names a second trained product: its label row holds two entries of 0.5
    with open(str(tmp_path / 'words.assocs'), 'a') as f:
        for i in range(NUM_GAINING):
            for d in range(2):
                f.write('%s W%04d_%d 1\n' % (products[(i + 1) % NUM_GAINING], i, d))
    env = dict(os.environ, PYTHONPATH=ROOT)
    P = lambda name: str(tmp_path / name)

    def run(script, *args, **kw):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', script)] + list(args) + ['--loglevel', 'ERROR'], env=env,
                              check=kw.get('check', True), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)

    prep = ['--window_size', '4', '--overlapping', '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1',
            '--no_instance_weights']
    run('prepare.py', '--seed', '3', P('old.trectext'), '--assoc_path', P('old.assocs'), '--meta_output', P('meta'),
        '--data_output', P('data.npz'), *prep)
    train = ['--data', P('data.npz'), '--meta', P('meta'), '--iterations', '2', '--batch_size', '64',
             '--word_representation_size', '16', '--regularization_lambda', '0.01', '--seed', '1']
    run('train.py', *train, '--type', 'loglinear', '--model_output', P('model'))
    run('prepare.py', '--seed', '3', P('words.trectext'), '--assoc_path', P('words.assocs'), '--vocabulary_from', P('meta'),
        '--extend_vocabulary', '--meta_output', P('new_meta'), '--data_output', P('new.npz'), *prep)

    def fold(*flags, **over):
        paths = dict(meta=P('meta'), model=P('model_2.bin'), new_meta=P('new_meta'), data=P('new.npz'))
        paths.update(over)
        return ['fold_in.py'] + list(flags) + ['--meta', paths['meta'], '--model', paths['model'], '--new_meta', paths['new_meta'],
                                              '--data', paths['data'], '--iterations', '3', '--batch_size', '64', '--seed', '1']

    run(*fold('--ll_new_words', '--label_rows'), '--model_output', P('model_w.bin'), '--meta_output', P('meta_w'))

    meta, meta_w, new_meta = foldin.read_meta(P('meta')), foldin.read_meta(P('meta_w')), foldin.read_meta(P('new_meta'))
    V_w = len(meta[1])
    added = [meta_w[2][i] for i in range(V_w, len(meta_w[2]))]
    assert sorted(added) == sorted(NEW_WORDS) and meta_w[3] == meta[3]
    # the dump: the trained rows, W and b are bit-equal to the input dump's
    old, new = training.read_checkpoint(P('model_2.bin')), training.read_checkpoint(P('model_w.bin'))
    assert new['args'].type is models.LanguageModel and len(new['tables']) == 1
    Rw_old, Rw_new = np.asarray(old['tables'][0]), np.asarray(new['tables'][0])
    assert Rw_old.shape == (V_w, 16) and Rw_new.shape == (V_w + len(NEW_WORDS), 16)
    assert Rw_new[:V_w].tobytes() == Rw_old.tobytes()
    assert np.asarray(new['predict_fn'].R_w).tobytes() == Rw_new.tobytes()
    W, b = np.asarray(old['predict_fn'].W), np.asarray(old['predict_fn'].b)
    assert np.asarray(new['predict_fn'].W).tobytes() == W.tobytes() and np.asarray(new['predict_fn'].b).tobytes() == b.tobytes()

    # the new rows are those of LogLinearWordFoldIn driven directly with the same seed and rows: y_train as the sparse matrix
    # it is, columns moved to the trained index, the windows without a new word dropped
    (x, y, w), _ = training.load_data_sets(P('new.npz'))
    index_of = dict((entity_id, index) for index, entity_id in meta[3].items())
    trained = np.array([index_of[new_meta[3][e]] for e in range(len(new_meta[3]))], dtype=np.int32)
    y = foldin.remap_label_columns(y, trained, W.shape[1])
    keep = (np.asarray(x) >= V_w).any(axis=1)
    x, y = np.asarray(x)[keep].astype(np.int32), y[keep]
    w = None if w is None else np.asarray(w)[keep]
    counts = np.diff(y.indptr)
    assert int(keep.sum()) >= 2 * 64 and (counts == 2).all() and np.allclose(y.data, 0.5) and y.shape == (x.shape[0], len(meta[3]))
    state = np.random.get_state()
    np.random.seed(1)
    drawn = foldin.new_word_rows(V_w, len(NEW_WORDS), 16)
    direct = foldin.LogLinearWordFoldIn(Rw_old, W, b, drawn, (x, y, w), batch_size=64, regularization_lambda=0.01,
                                        window_size=meta[0].window_size)
    direct.train_error()
    for _ in range(3):
        direct.train()
        direct.train_error()
    assert direct._foldin.plan()['labels'] == 'rows'
    rows = direct.get_new_word_representations()
    direct.close()
    np.random.set_state(state)
    assert rows.tobytes() == Rw_new[V_w:].tobytes()
    assert np.isfinite(rows).all() and (np.abs(rows - drawn).max(axis=1) > 0).all()          # ... and they LEARNT

    # a topic that consists of a new word ranks every entity on the extended model
    (tmp_path / 'topics').write_text(''.join('%s;%s\n' % kv for kv in list(topics.items())[:5]) + 'new0;%s\n' % NEW_WORDS[7])
    run('query.py', '--meta', P('meta_w'), '--model', P('model_w.bin'), '--topics', P('topics'), '--run_out', P('run_new'))
    with open(P('run_new_ef')) as f:
        ranked = trec_utils.parse_run(f)
    assert len(ranked) == 6
    assert sorted(e for _, e in ranked['new0']) == sorted(products) and np.isfinite([s for s, _ in ranked['new0']]).all()

    # refusals leave no output file
    def refused(command, text):
        bad = run(*command, '--model_output', P('model_x.bin'), '--meta_output', P('meta_x'), check=False)
        assert bad.returncode != 0 and text in bad.stdout, bad.stdout[-2000:]
        assert not os.path.exists(P('model_x.bin')) and not os.path.exists(P('meta_x'))

    # ... --label_rows alone, and with --new_words
    refused(fold('--label_rows'), b'--label_rows needs --ll_new_words')
    refused(fold('--new_words', '--label_rows'), b'--label_rows needs --ll_new_words')
    # ... a vectorspace dump
    rng = np.random.RandomState(5)
    R_e = rng.uniform(-0.3, 0.3, (len(meta[3]), 8)).astype(np.float32)
    vs_fn = models.VectorSpacePredictFn(W=rng.uniform(-0.3, 0.3, (16, 8)).astype(np.float32), b=np.zeros(8, np.float32))
    foldin.write_dump(P('vs.bin'), [argparse.Namespace(type=models.VectorSpaceLanguageModel), vs_fn, Rw_old, R_e])
    refused(fold('--ll_new_words', '--label_rows', model=P('vs.bin')), b'--ll_new_words needs a loglinear model')
    # ... an entity the trained meta does not know stays refused
    unknown = list(new_meta)
    unknown[3] = dict(unknown[3])
    unknown[3][len(unknown[3])] = 'NOT_A_TRAINED_PRODUCT'
    foldin.write_meta(P('new_meta_unknown'), unknown)
    refused(fold('--ll_new_words', '--label_rows', new_meta=P('new_meta_unknown')), b'fold the entities in first')
