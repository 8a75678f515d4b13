"""GPU: the command-line chain of a fold-in on the product-search fixture (tests/golden/product_search): bin/prepare.py and
bin/train.py on 300 of its products, bin/prepare.py --vocabulary_from and bin/fold_in.py for the other 38, bin/query.py on
the extended dump and meta."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sert_amd import foldin
from sert_amd.utils import trec_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'product_search')
NUM_NEW = 38


def _corpora(tmp_path):
    """Two documents per product of product_list, in the words of a topic the qrels judge it relevant for (any topic
    otherwise) plus a few words of another; the last NUM_NEW products' documents go to the 'new' corpus."""
    with open(os.path.join(GOLD, 'topics')) as f:
        topics = trec_utils.parse_topics(f)
    with open(os.path.join(GOLD, 'product_list')) as f:
        products = [line.strip() for line in f if line.strip()]
    relevant_for = {}
    for name in ('validation', 'test'):
        with open(os.path.join(GOLD, 'qrel_' + name)) as f:
            for topic, rel in trec_utils.parse_qrels(f).items():
                for entity, gain in rel.items():
                    if gain > 0 and topic in topics:
                        relevant_for.setdefault(entity, topic)
    rng = np.random.RandomState(0)
    ids = list(topics)
    new = set(products[-NUM_NEW:])
    parts = {'old': ([], []), 'new': ([], [])}
    for i, product in enumerate(products):
        own = topics[relevant_for.get(product, ids[rng.randint(len(ids))])].split()
        docs, assocs = parts['new' if product in new else 'old']
        for d in range(2):
            other = topics[ids[rng.randint(len(ids))]].split()
            text = rng.choice(own, size=18).tolist() + rng.choice(other, size=4).tolist()
            docs.append('<DOC>\n<DOCNO> D%04d_%d </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n' % (i, d, ' '.join(text)))
            assocs.append('%s D%04d_%d 1' % (product, i, d))
    for name, (docs, assocs) in parts.items():
        (tmp_path / (name + '.trectext')).write_text(''.join(docs))
        (tmp_path / (name + '.assocs')).write_text('\n'.join(assocs) + '\n')
    return products, new


def test_fold_in_then_query_ranks_the_new_products(hip_lib, tmp_path):
    products, new = _corpora(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    P = lambda name: str(tmp_path / name)

    def run(script, *args):
        subprocess.run([sys.executable, os.path.join(ROOT, 'bin', script)] + list(args) + ['--loglevel', 'ERROR'], env=env,
                       check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)

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
    run(*fold, '--model_output', P('model_ext.bin'), '--meta_output', P('meta_ext'))
    run('query.py', '--meta', P('meta_ext'), '--model', P('model_ext.bin'), '--topics', os.path.join(GOLD, 'topics'),
        '--run_out', P('run'))
    meta, meta_ext = foldin.read_meta(P('meta')), foldin.read_meta(P('meta_ext'))
    V_e = len(meta[3])
    assert V_e == len(products) - NUM_NEW and len(meta_ext[3]) == len(products)
    assert set(meta_ext[3][i] for i in range(V_e, len(products))) == new
    assert all(meta_ext[3][i] == meta[3][i] for i in range(V_e)) and meta_ext[1] == meta[1]
    assert all(meta_ext[4][e] for e in new)                        # the new products' documents
    with open(P('run_ef')) as f:
        ranking = trec_utils.parse_run(f)
    assert ranking and all(len(entries) == len(products) for entries in ranking.values())     # every entity, old and new
    assert all(new <= set(e for _, e in entries) for entries in ranking.values())
    # a new entity id that the trained meta already knows is refused: folding the same entities into the EXTENDED model
    again = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'fold_in.py'), '--meta', P('meta_ext'), '--model',
                            P('model_ext.bin')] + fold[5:] + ['--model_output', P('model_x.bin'), '--meta_output', P('meta_x')],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert again.returncode != 0 and b'already in the trained model' in again.stdout
    assert not os.path.exists(P('model_x.bin')) and not os.path.exists(P('meta_x'))
