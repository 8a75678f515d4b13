"""GPU: the command-line chain of a refresh on the corpus construction of tests/test_gpu_foldin_cli.py (the product-search
fixture, tests/golden/product_search): bin/prepare.py and bin/train.py on 120 of its products, bin/prepare.py
--vocabulary_from over new documents of 8 of those products AND of 12 products the model never saw, bin/fold_in.py without
and with --refresh, bin/query.py on the refreshed dump and meta."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import foldin, training
from sert_amd.utils import trec_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'product_search')
NUM_OLD, NUM_NEW, NUM_REFRESHED = 120, 12, 8


def _corpora(tmp_path):
    """Two documents per product, in the words of one topic plus a few of another (as tests/test_gpu_foldin_cli.py).  'old':
    the first NUM_OLD products.  'new': the next NUM_NEW products and, interleaved with them, two FURTHER documents of every
    fifteenth old product."""
    with open(os.path.join(GOLD, 'topics')) as f:
        topics = trec_utils.parse_topics(f)
    with open(os.path.join(GOLD, 'product_list')) as f:
        products = [line.strip() for line in f if line.strip()][:NUM_OLD + NUM_NEW]
    rng = np.random.RandomState(0)
    ids = list(topics)
    old, new = products[:NUM_OLD], products[NUM_OLD:]
    refreshed = old[::NUM_OLD // NUM_REFRESHED][:NUM_REFRESHED]
    parts = {'old': ([], []), 'new': ([], [])}

    def add(part, product, tag):
        own = topics[ids[rng.randint(len(ids))]].split()
        docs, assocs = parts[part]
        for d in range(2):
            other = topics[ids[rng.randint(len(ids))]].split()
            text = rng.choice(own, size=18).tolist() + rng.choice(other, size=4).tolist()
            docs.append('<DOC>\n<DOCNO> %s_%d </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n' % (tag, d, ' '.join(text)))
            assocs.append('%s %s_%d 1' % (product, tag, d))

    for i, product in enumerate(old):
        add('old', product, 'D%04d' % i)
    for i in range(max(NUM_NEW, NUM_REFRESHED)):
        if i < NUM_NEW:
            add('new', new[i], 'N%04d' % i)
        if i < NUM_REFRESHED:
            add('new', refreshed[i], 'R%04d' % i)
    for name, (docs, assocs) in parts.items():
        (tmp_path / (name + '.trectext')).write_text(''.join(docs))
        (tmp_path / (name + '.assocs')).write_text('\n'.join(assocs) + '\n')
    return old, set(new), set(refreshed)


def test_refresh_then_query(hip_lib, tmp_path):
    old, new, refreshed = _corpora(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    P = lambda name: str(tmp_path / name)

    def run(script, *args, **kw):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', script)] + list(args) + ['--loglevel', 'ERROR'], env=env,
                              check=kw.get('check', True), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)

    prep = ['--window_size', '4', '--overlapping', '--vocabulary_min_count', '1', '--validation_set_ratio', '0.1',
            '--no_instance_weights']
    run('prepare.py', '--seed', '3', P('old.trectext'), '--assoc_path', P('old.assocs'), '--meta_output', P('meta'),
        '--data_output', P('data.npz'), *prep)
    run('train.py', '--data', P('data.npz'), '--meta', P('meta'), '--type', 'vectorspace', '--iterations', '2', '--batch_size',
        '64', '--word_representation_size', '16', '--entity_representation_size', '16', '--num_negative_samples', '4',
        '--one_hot_classes', '--regularization_lambda', '0.01', '--model_output', P('model'), '--seed', '1')
    run('prepare.py', '--seed', '3', P('new.trectext'), '--assoc_path', P('new.assocs'), '--vocabulary_from', P('meta'),
        '--meta_output', P('new_meta'), '--data_output', P('new.npz'), *prep)
    fold = ['fold_in.py', '--meta', P('meta'), '--model', P('model_2.bin'), '--new_meta', P('new_meta'), '--data', P('new.npz'),
            '--iterations', '3', '--batch_size', '64', '--num_negative_samples', '4', '--seed', '1']
    # without --refresh a known id is refused, with today's message, and nothing is written
    refused = run(*fold, '--model_output', P('model_x.bin'), '--meta_output', P('meta_x'), check=False)
    assert refused.returncode != 0 and b'already in the trained model' in refused.stdout
    assert not os.path.exists(P('model_x.bin')) and not os.path.exists(P('meta_x'))
    run(*fold, '--refresh', '--model_output', P('model_ref.bin'), '--meta_output', P('meta_ref'))

    meta, meta_ref = foldin.read_meta(P('meta')), foldin.read_meta(P('meta_ref'))
    V_e = len(meta[3])
    assert V_e == NUM_OLD and len(meta_ref[3]) == NUM_OLD + NUM_NEW
    assert all(meta_ref[3][i] == meta[3][i] for i in range(V_e)) and meta_ref[1] == meta[1]
    assert set(meta_ref[3][i] for i in range(V_e, V_e + NUM_NEW)) == new
    for e in refreshed:                                              # the documents it had, then the ones it gained
        assert len(meta_ref[4][e]) == 4 and meta_ref[4][e][:2] == meta[4][e]
    assert all(len(meta_ref[4][e]) == 2 for e in new)
    R_e = training.read_checkpoint(P('model_2.bin'))['tables'][1]
    R_ref = training.read_checkpoint(P('model_ref.bin'))['tables'][1]
    assert R_e.shape[0] == V_e and R_ref.shape == (V_e + NUM_NEW, R_e.shape[1])
    index_of = dict((entity, i) for i, entity in meta[3].items())
    moved = sorted(index_of[e] for e in refreshed)
    kept = np.setdiff1d(np.arange(V_e), moved)
    assert np.array_equal(R_ref[kept].view(np.uint32), R_e[kept].view(np.uint32))      # the untouched rows: bit-equal
    assert all(not np.array_equal(R_ref[i], R_e[i]) for i in moved)                     # the refreshed rows differ
    assert np.isfinite(R_ref).all() and np.abs(R_ref[V_e:]).max() > 0

    run('query.py', '--meta', P('meta_ref'), '--model', P('model_ref.bin'), '--topics', os.path.join(GOLD, 'topics'),
        '--run_out', P('run'))
    with open(P('run_ef')) as f:
        ranking = trec_utils.parse_run(f)
    assert ranking and all(len(entries) == NUM_OLD + NUM_NEW for entries in ranking.values())
    assert all((new | refreshed) <= set(e for _, e in entries) for entries in ranking.values())
