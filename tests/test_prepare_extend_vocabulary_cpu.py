"""CPU: ``bin/prepare.py --vocabulary_from META --extend_vocabulary`` appends the documents' new words behind the trained
vocabulary and changes nothing without the flag; sert_amd.foldin.extend_meta_words / extend_words_dump write the extended
meta and dump of bin/fold_in.py --new_words consistently.  No device."""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

from sert_amd import foldin
from sert_amd import prepare as prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _doc(name, text):
    return '<DOC>\n<DOCNO> %s </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n' % (name, text)


def _prepare(tmp_path, docs, assocs, meta, data, extra=(), min_count=2):
    (tmp_path / (meta + '.trectext')).write_text(''.join(docs))
    (tmp_path / (meta + '.assocs')).write_text('\n'.join(assocs) + '\n')
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'prepare.py'), '--seed', '3', str(tmp_path / (meta + '.trectext')),
           '--assoc_path', str(tmp_path / (meta + '.assocs')), '--window_size', '4', '--vocabulary_min_count', str(min_count),
           '--validation_set_ratio', '0.2', '--meta_output', str(tmp_path / meta), '--data_output', str(tmp_path / data),
           '--loglevel', 'ERROR'] + list(extra)
    subprocess.check_call(cmd)
    return np.load(str(tmp_path / data), allow_pickle=True), foldin.read_meta(str(tmp_path / meta))


@pytest.fixture(scope='module')
def corpora(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('extend_vocabulary')
    rng = np.random.RandomState(0)
    old_words = 'alpha beta gamma delta kappa lambda sigma omega'.split()
    docs = [_doc('D%02d' % d, ' '.join(rng.choice(old_words, size=20))) for d in range(8)]
    assocs = ['E%d D%02d 1' % (d % 2, d) for d in range(8)]
    _, old_meta = _prepare(tmp, docs, assocs, 'meta', 'data.npz')
    # new documents of the TRAINED entities: known words, new words of different counts (zx81 12, bq7 12, kz 8 per corpus),
    # a word below the minimum count (once1: once in all), a one-letter word, a stop word and a number
    text = ' '.join(['omega'] * 4 + ['zx81', 'bq7'] * 3 + ['kz'] * 2 + ['q', 'the', '1984', 'alpha'])
    new_docs = [_doc('N%02d' % d, text + (' once1' if d == 0 else '')) for d in range(4)]
    new_assocs = ['E%d N%02d 1' % (d % 2, d) for d in range(4)]
    return tmp, old_meta, new_docs, new_assocs


def test_new_words_are_appended_in_vocabulary_order(corpora):
    tmp, old_meta, new_docs, new_assocs = corpora
    words, tokens = old_meta[1], old_meta[2]
    V_w = len(words)
    data, new_meta = _prepare(tmp, new_docs, new_assocs, 'new_meta', 'new.npz',
                              ['--vocabulary_from', str(tmp / 'meta'), '--extend_vocabulary'])
    new_words, new_tokens = new_meta[1], new_meta[2]
    # trained ids are untouched: every trained entry is there as it was
    assert all(new_words[w] == words[w] for w in words) and all(new_tokens[i] == tokens[i] for i in range(V_w))
    # appended: count descending, then word -- bq7 and zx81 (12 each), kz (8), <num> (4); not the rare word, the one-letter
    # word or the stop word
    appended = [new_tokens[i] for i in range(V_w, len(new_tokens))]
    expect = ['bq7', 'zx81', 'kz'] + ([] if prep.NUMERIC_TOKEN in words else [prep.NUMERIC_TOKEN])
    assert appended == expect and len(new_words) == len(new_tokens) == V_w + len(expect)
    assert [new_words[w].id for w in appended] == list(range(V_w, V_w + len(appended)))
    assert [new_words[w].count for w in appended[:3]] == [12, 12, 8]
    assert foldin.new_words_of(old_meta, new_meta) == appended
    # the five pickles: the namespace carries both flags, the entity index is the new documents' own, the associations too
    assert new_meta[0].vocabulary_from == str(tmp / 'meta') and new_meta[0].extend_vocabulary is True
    assert new_meta[3] == {0: 'E0', 1: 'E1'} and sorted(new_meta[4]) == ['E0', 'E1']
    assert sorted(new_meta[4]['E0']) == ['N00', 'N02']
    # the instances carry the new ids
    x = np.concatenate([data['x_train'], data['x_validate']])
    assert x.max() < len(new_words) and {new_words[w].id for w in ('bq7', 'zx81', 'kz')} <= set(np.unique(x).tolist())
    assert x.dtype == np.min_scalar_type(len(new_words) - 1)


def test_vocabulary_max_size_bounds_the_appended_words(corpora):
    tmp, old_meta, new_docs, new_assocs = corpora
    V_w = len(old_meta[1])
    _, capped = _prepare(tmp, new_docs, new_assocs, 'cap_meta', 'cap.npz',
                         ['--vocabulary_from', str(tmp / 'meta'), '--extend_vocabulary', '--vocabulary_max_size', str(V_w + 2)])
    assert [capped[2][i] for i in range(V_w, len(capped[2]))] == ['bq7', 'zx81']
    _, full = _prepare(tmp, new_docs, new_assocs, 'full_meta', 'full.npz',
                       ['--vocabulary_from', str(tmp / 'meta'), '--extend_vocabulary', '--vocabulary_max_size', str(V_w)])
    assert full[1] == old_meta[1] and full[2] == old_meta[2]


def test_without_the_flag_nothing_changes(corpora):
    """The same corpus and seed without --extend_vocabulary: the namespace lacks the flag, and the arrays of the npz and the
    meta are those of the --vocabulary_from path with no out-of-vocabulary token kept -- restated here as: the run whose
    documents had their out-of-vocabulary tokens deleted beforehand."""
    tmp, old_meta, new_docs, new_assocs = corpora
    extra = ['--vocabulary_from', str(tmp / 'meta')]
    data, meta = _prepare(tmp, new_docs, new_assocs, 'plain_meta', 'plain.npz', extra)
    assert not hasattr(meta[0], 'extend_vocabulary') and not hasattr(old_meta[0], 'extend_vocabulary')
    assert meta[1] == old_meta[1] and meta[2] == old_meta[2]
    known = ' '.join(['omega'] * 4 + ['alpha'])
    stripped = [_doc('N%02d' % d, known) for d in range(4)]
    ref, ref_meta = _prepare(tmp, stripped, new_assocs, 'ref_meta', 'ref.npz', extra)
    for key in ('x_train', 'x_validate', 'w_train'):
        assert np.array_equal(data[key], ref[key]) and data[key].dtype == ref[key].dtype, key
    for key in ('y_train', 'y_validate'):
        assert (data[key][()] != ref[key][()]).nnz == 0
    assert meta[1:] == ref_meta[1:]
    # --extend_vocabulary without --vocabulary_from is refused
    with pytest.raises(subprocess.CalledProcessError):
        _prepare(tmp, new_docs, new_assocs, 'bad_meta', 'bad.npz', ['--extend_vocabulary'])
    assert not os.path.exists(str(tmp / 'bad.npz'))


def _hand_made():
    Vw, Ve = 6, 3
    W = prep.Word
    words = {'w%d' % i: W(i, 10 - i) for i in range(Vw)}
    tokens = {i: 'w%d' % i for i in range(Vw)}
    meta = [types.SimpleNamespace(window_size=4), words, tokens, {i: 'E%d' % i for i in range(Ve)},
            {'E%d' % i: ['D%d' % i] for i in range(Ve)}]
    new_words = dict(words, zx81=W(Vw, 5), bq7=W(Vw + 1, 3))
    new_tokens = dict(tokens)
    new_tokens[Vw], new_tokens[Vw + 1] = 'zx81', 'bq7'
    new_meta = [types.SimpleNamespace(window_size=4, extend_vocabulary=True), new_words, new_tokens, {0: 'E2', 1: 'E0'},
                {'E2': ['N0', 'N1'], 'E0': ['N2']}]
    return meta, new_meta


def test_extend_meta_words():
    meta, new_meta = _hand_made()
    ext = foldin.extend_meta_words(meta, new_meta)
    assert ext[0] is meta[0] and ext[1] is new_meta[1] and ext[2] is new_meta[2]
    assert ext[3] == meta[3]                                      # known ids keep their internal indices; none is added
    assert ext[4] == {'E0': ['D0', 'N2'], 'E1': ['D1'], 'E2': ['D2', 'N0', 'N1']}
    assert meta[4]['E0'] == ['D0'] and len(meta[1]) == 6          # the inputs are not changed
    assert foldin.new_words_of(meta, new_meta) == ['zx81', 'bq7']
    assert foldin.new_words_of(meta, [None, dict(meta[1]), dict(meta[2]), {}, {}]) == []
    # refusals: an unknown entity (with the advice), a vocabulary that moved a trained id, a gap, a missing trained word
    unknown = list(new_meta)
    unknown[3] = {0: 'E2', 1: 'F9'}
    with pytest.raises(RuntimeError, match='fold the entities in first'):
        foldin.extend_meta_words(meta, unknown)
    W = prep.Word
    swapped_tokens = dict(new_meta[2])
    swapped_tokens[0], swapped_tokens[1] = 'w1', 'w0'
    gap_tokens = dict(meta[2])
    gap_tokens[7] = 'zx81'
    for words, tokens in (
            (dict(new_meta[1], w0=W(1, 10), w1=W(0, 9)), swapped_tokens),                               # two trained ids swapped
            (dict(meta[1], zx81=W(7, 5)), gap_tokens),                                                  # id 6 is missing
            (dict((w, e) for w, e in new_meta[1].items() if w != 'w3'), new_meta[2]),                    # a trained word is gone
            (meta[1], dict(list(meta[2].items())[:-1]))):                                               # fewer tokens than words
        bad = [new_meta[0], words, tokens, new_meta[3], new_meta[4]]
        with pytest.raises(RuntimeError, match='not the trained one'):
            foldin.extend_meta_words(meta, bad)


def test_extend_words_dump(tmp_path):
    rng = np.random.RandomState(1)
    Vw, Ve, Nw, dw, de = 6, 3, 2, 5, 4
    R_w, R_e = rng.randn(Vw, dw).astype(np.float32), rng.randn(Ve, de).astype(np.float32)
    new_rows = rng.randn(Nw, dw)
    args, predict = types.SimpleNamespace(batch_size=8), {'W': rng.randn(dw, de).astype(np.float32)}
    objects = foldin.extend_words_dump(args, predict, R_w, R_e, new_rows)
    assert objects[0] is args and objects[1] is predict and objects[3] is R_e
    foldin.write_dump(str(tmp_path / 'model.bin'), objects)
    with open(str(tmp_path / 'model.bin'), 'rb') as f:
        back = [pickle.load(f) for _ in range(4)]
    assert back[2].shape == (Vw + Nw, dw) and back[2].dtype == np.float32
    assert np.array_equal(back[2][:Vw], R_w) and np.array_equal(back[2][Vw:], new_rows.astype(np.float32))
    assert np.array_equal(back[3], R_e) and np.array_equal(back[1]['W'], predict['W']) and R_w.shape == (Vw, dw)
    with pytest.raises(AssertionError):
        foldin.extend_words_dump(args, predict, R_w, R_e, rng.randn(Nw, dw + 1))


def test_new_word_rows_are_drawn_at_the_trained_scale():
    """foldin.new_word_rows: from the global generator, uniform within Glorot's bound of the TRAINED (V_w, d_w) table -- the
    bound bin/train.py drew R_w in -- whatever the number of new words."""
    Vw, Nw, dw = 5000, 3, 16
    bound = np.sqrt(6.0 / (Vw + dw))
    np.random.seed(4)
    rows = foldin.new_word_rows(Vw, Nw, dw)
    np.random.seed(4)
    again = foldin.new_word_rows(Vw, Nw, dw)
    assert rows.shape == (Nw, dw) and rows.dtype == np.float32 and np.array_equal(rows, again)
    assert np.abs(rows).max() <= bound and np.abs(rows).max() > 0.5 * bound      # (48 draws: the largest is past half the bound)
    assert bound < 0.1 * np.sqrt(6.0 / (Nw + dw))       # the block's own Glorot bound would be ten times the trained rows'


def test_fold_in_refuses_a_dump_and_a_meta_of_different_models(tmp_path):
    """bin/fold_in.py --new_words: a dump whose R_w has another number of rows than --meta has words is refused with a message,
    under python -O too, before the data is read, and no output file exists."""
    from sert_amd import models
    meta, new_meta = _hand_made()
    P = lambda name: str(tmp_path / name)
    foldin.write_meta(P('meta'), meta)
    foldin.write_meta(P('new_meta'), new_meta)
    args = types.SimpleNamespace(type=models.VectorSpaceLanguageModel)
    foldin.write_dump(P('model.bin'), [args, {'W': np.zeros((5, 4), np.float32), 'b': np.zeros(4, np.float32)},
                                       np.zeros((len(meta[1]) + 1, 5), np.float32), np.zeros((3, 4), np.float32)])
    r = subprocess.run([sys.executable, '-O', os.path.join(ROOT, 'bin', 'fold_in.py'), '--new_words', '--meta', P('meta'),
                        '--model', P('model.bin'), '--new_meta', P('new_meta'), '--data', P('meta'), '--iterations', '1',
                        '--model_output', P('out.bin'), '--meta_output', P('out_meta'), '--loglevel', 'ERROR'],
                       env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode != 0 and b'they are not of the same model' in r.stdout, r.stdout[-2000:]
    assert b'7 word rows' in r.stdout and b'6 words' in r.stdout
    assert not os.path.exists(P('out.bin')) and not os.path.exists(P('out_meta'))
