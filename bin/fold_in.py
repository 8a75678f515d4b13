#!/usr/bin/env python
"""Fold unseen entities into a trained vectorspace model, on the device, without retraining it.

    python bin/prepare.py --seed 1 new_docs/*.trectext --assoc_path new_assocs --vocabulary_from meta \\
        --window_size 4 --meta_output new_meta --data_output new.npz
    python bin/fold_in.py --meta meta --model model_15.bin --new_meta new_meta --data new.npz --iterations 10 \\
        --model_output model_15_ext.bin --meta_output meta_ext
    python bin/query.py --meta meta_ext --model model_15_ext.bin --topics topics --top 100 --run_out run

The word table, the projection and the trained entity rows stay as they are; only the rows of the new entities learn
(sert_amd.foldin.EntityFoldIn), with the NCE objective of training, on the instances of ``--data``: the ``x_train`` /
``y_train`` / ``w_train`` of a bin/prepare.py run with ``--vocabulary_from META`` over the new entities' documents.
``--model_output`` is a model dump with R_e extended by the new rows, ``--meta_output`` the meta with the entity index
and the associations extended (new entity e of ``--new_meta`` gets internal index V_e + e); bin/query.py serves the pair
unchanged.  A new entity id that ``--meta`` already knows is refused.

With ``--refresh`` such an id is not refused: the entity GAINED documents (new reviews of a known product), and its trained
row learns too, in place -- it keeps its internal index, the output dump has its row replaced and the rows of the really
new entities appended (V_e is unchanged when nothing is new), the output meta has its associations merged
(sert_amd.foldin.merge_meta).  A refreshed row starts from its trained value and learns from the instances given: to keep
its old evidence, pass the entity's old documents along with the new ones.

    python bin/fold_in.py --refresh --meta meta --model model_15.bin --new_meta new_meta --data new.npz --iterations 10 \\
        --model_output model_15_ref.bin --meta_output meta_ref

A dump of a LOGLINEAR model (bin/train.py --type loglinear: expert finding) takes a path of its own, chosen by the dump's
model type: the word table and the trained columns of the output layer stay as they are, each new entity gets a column of W
and an entry of b (sert_amd.foldin.LogLinearFoldIn) that learn with the model's own loss over all V_e + N entities.  The same
command line; ``--num_negative_samples`` is not read (there is nothing to sample), ``--refresh`` is refused (see
``--unfreeze_known``).  The output dump's predict function holds W (d, V_e + N) and b (V_e + N).

With ``--label_distributions`` (loglinear dumps only) the fold-in learns from the loss the expert-finding recipe trains with,
bin/train.py --type loglinear WITHOUT --one_hot_classes: ``y_train`` of ``--data`` is used as the sparse matrix of label
distributions it is -- one row per instance over the entities of ``--new_meta`` -- and ``w_train`` as bin/train.py uses it.
An entity id of ``--new_meta`` that ``--meta`` knows is then a frozen co-label, not an error: a new person's documents are
mostly co-authored with people the model knows.  Such an id keeps its internal index and its column of W / b, bit for bit; its
share of a document's label mass enters the new columns' gradient; its associations gain the new documents.  The unknown ids
become columns V_e .. in the order of ``--new_meta`` (sert_amd.foldin.label_columns); if none is unknown there is nothing to
fold in and the run is refused.

    python bin/fold_in.py --label_distributions --meta meta --model model_15.bin --new_meta new_meta --data new.npz \\
        --iterations 10 --model_output model_15_ext.bin --meta_output meta_ext

With ``--unfreeze_known`` (loglinear dumps only) an entity id of ``--new_meta`` that ``--meta`` knows is neither refused nor
frozen: the person GAINED documents, and their column of W and their bias learn too, in place -- they keep their internal
index, the output dump has their column and bias replaced and the really new entities' appended (V_e is unchanged when nothing
is new), every other column keeps its bits, and the output meta has the associations merged (sert_amd.foldin.merge_meta).
Without ``--label_distributions`` the instances are one per label, as above; with it the label rows are used as they are and
every known id among their columns learns.  A refreshed column starts from its trained value and learns from the instances
given: to keep its old evidence, pass the entity's old documents along with the new ones.

    python bin/fold_in.py --unfreeze_known --label_distributions --meta meta --model model_15.bin --new_meta new_meta \\
        --data new.npz --iterations 10 --model_output model_15_ref.bin --meta_output meta_ref

With ``--new_words`` (vectorspace dumps only) the VOCABULARY grows instead: ``--new_meta`` / ``--data`` come from a
bin/prepare.py run with ``--vocabulary_from META --extend_vocabulary`` over new documents of trained entities, whose new words
(brand names, model numbers) carry the token ids V_w ..  The trained word rows, the projection and the whole entity table stay
as they are; only the rows of the new words learn (sert_amd.foldin.WordFoldIn), drawn at the scale bin/train.py drew the trained R_w, on
the windows that hold a new word (the others cannot move a trainable row and are dropped).  Every entity of ``--new_meta`` must
be known to ``--meta``: fold new entities in first and prepare against the extended meta.  ``--model_output`` is a dump with
R_w extended by the new rows, ``--meta_output`` the meta with the extended vocabulary; bin/query.py serves the pair unchanged.

    python bin/prepare.py --seed 1 new_docs/*.trectext --assoc_path new_assocs --vocabulary_from meta --extend_vocabulary \\
        --window_size 4 --meta_output new_meta --data_output new.npz
    python bin/fold_in.py --new_words --meta meta --model model_15.bin --new_meta new_meta --data new.npz --iterations 10 \\
        --model_output model_15_words.bin --meta_output meta_words

With ``--ll_new_words`` (loglinear dumps only) the same happens to an expert-finding model: new documents by people the model
knows bring project names and acronyms the vocabulary has never seen, which bin/query.py drops from every query.  ``--new_meta``
/ ``--data`` come from the same bin/prepare.py run (``--vocabulary_from META --extend_vocabulary``); the trained word rows and
the whole output layer W, b stay as they are and only the rows of the new words learn (sert_amd.foldin.LogLinearWordFoldIn),
with the model's own loss, one instance per label, on the windows that hold a new word.  ``--model_output`` is a dump whose R_w
-- in the dump and in its predict function -- has the new rows appended; ``--num_negative_samples`` is not read.

    python bin/fold_in.py --ll_new_words --meta meta --model model_15.bin --new_meta new_meta --data new.npz --iterations 10 \\
        --model_output model_15_words.bin --meta_output meta_words

With ``--ll_new_words --label_rows`` the new word rows learn from the loss the expert-finding recipe trains with: ``y_train`` of
``--data`` stays the sparse matrix it is -- one instance per window, its labels a distribution over the document's people, as
bin/train.py --type loglinear learns without ``--one_hot_classes`` -- instead of one instance per label.  The columns are moved
from ``--new_meta``'s entity index to the trained one; an entity the trained meta does not know stays refused (fold the entities
in first).  This is the loss that produced the frozen R_w, W and b beside the new rows, and there are as many instances as
windows, not windows times co-authors.  ``--label_rows`` is not ``--label_distributions``, which is the entity fold-in's flag
(unknown ids become new columns) and stays refused with ``--ll_new_words``.

    python bin/fold_in.py --ll_new_words --label_rows --meta meta --model model_15.bin --new_meta new_meta --data new.npz \\
        --iterations 10 --model_output model_15_words.bin --meta_output meta_words
"""
import argparse
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import foldin, models, training  # noqa: E402
from sert_amd.utils import argparse_utils as au  # noqa: E402
from sert_amd.utils import logging_utils  # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--loglevel', type=str, default='INFO')
    parser.add_argument('--meta', type=au.existing_file_path, required=True)
    parser.add_argument('--model', type=au.existing_file_path, required=True)
    parser.add_argument('--new_meta', type=au.existing_file_path, required=True)
    parser.add_argument('--data', type=au.existing_file_path, required=True)
    parser.add_argument('--iterations', type=au.positive_int, required=True)
    parser.add_argument('--batch_size', type=au.positive_int, default=1024)
    parser.add_argument('--num_negative_samples', type=au.positive_int, default=10)
    parser.add_argument('--regularization_lambda', type=float, default=0.01)
    parser.add_argument('--seed', type=int, default=None)
    parser.add_argument('--device', type=int, default=0)
    parser.add_argument('--refresh', action='store_true', default=False,
                        help='entity ids of --new_meta that --meta knows are refreshed (their trained rows learn from the '
                             'instances given, in place) instead of refused; the rest are new.  A refreshed row learns from '
                             'the instances given: to keep its old evidence, pass the entity\'s old documents along with '
                             'the new ones.')
    parser.add_argument('--label_distributions', action='store_true', default=False,
                        help='loglinear dumps only: learn from the label distributions of --data (y_train as the sparse matrix '
                             'it is, as bin/train.py does without --one_hot_classes) instead of one instance per label.  Entity '
                             'ids of --new_meta that --meta knows are accepted as frozen co-labels: they keep their index and '
                             'their trained column, and their associations gain the new documents; the unknown ids become the '
                             'new columns.  Refused if no id is unknown.')
    parser.add_argument('--unfreeze_known', action='store_true', default=False,
                        help='loglinear dumps only: entity ids of --new_meta that --meta knows are neither refused nor frozen '
                             'co-labels -- their trained columns of W and their biases learn from the instances given, in place; '
                             'the rest are new (none need be).  A refreshed column learns from the instances given: to keep its '
                             'old evidence, pass the entity\'s old documents along with the new ones.')
    parser.add_argument('--new_words', action='store_true', default=False,
                        help='vectorspace dumps only: fold in the new WORDS of --new_meta (bin/prepare.py --vocabulary_from META '
                             '--extend_vocabulary) instead of entities: their rows of R_w learn, everything trained stays as it '
                             'is.  Every entity of --new_meta must be known to --meta.')
    parser.add_argument('--ll_new_words', action='store_true', default=False,
                        help='loglinear dumps only: fold in the new WORDS of --new_meta (bin/prepare.py --vocabulary_from META '
                             '--extend_vocabulary) instead of entities: their rows of R_w learn with the model\'s own loss, '
                             'R_w, W and b stay as they are.  Every entity of --new_meta must be known to --meta.')
    parser.add_argument('--label_rows', action='store_true', default=False,
                        help='with --ll_new_words only: learn from the label rows of --data (y_train as the sparse matrix it is, '
                             'as bin/train.py --type loglinear does without --one_hot_classes) instead of one instance per '
                             'label.  Every entity of --new_meta must be known to --meta.')
    parser.add_argument('--model_output', type=au.nonexisting_file_path, required=True)
    parser.add_argument('--meta_output', type=au.nonexisting_file_path, required=True)
    return parser


def load_model(path):
    """The pickle stream of bin/train.py, as bin/query.py reads it: namespace, predict_fn, R_w, R_e (an optimiser-state
    trailer is not carried over: the trained rows do not move)."""
    dump = training.read_checkpoint(path)
    if len(dump['tables']) < 2:
        raise RuntimeError('%s holds no entity representations: a fold-in needs a vectorspace model.' % path)
    return [dump['args'], dump['predict_fn']] + dump['tables'][:2]


def one_hot_training_set(path):
    """(x, y int, w) of a bin/prepare.py npz, label distributions expanded as bin/train.py --one_hot_classes does."""
    training_set, validation_set = training.load_data_sets(path)
    (x, y, w), _ = training.to_one_hot(training_set, validation_set)
    return x, np.asarray(y), w


def fold_in_loglinear(args):
    """A loglinear dump (namespace, LogLinearPredictFn, R_w): the new entities get columns of the output layer and biases of
    their own (sert_amd.foldin.LogLinearFoldIn) with the model's loss over all V_e + N entities; there are no negatives to
    draw, so --num_negative_samples is not read.  --refresh is refused: it is the vectorspace flag.
    --label_distributions: the instances keep their label rows, and ids the trained meta knows are frozen co-labels.
    --unfreeze_known: ids the trained meta knows are refreshed -- their columns and biases learn too."""
    if args.refresh:
        raise RuntimeError('--refresh needs a vectorspace model: the trained columns of a loglinear model are refreshed with '
                           '--unfreeze_known.')
    dump = training.read_checkpoint(args.model)
    model_args, predict_fn, R_w = dump['args'], dump['predict_fn'], dump['tables'][0]
    meta = foldin.read_meta(args.meta)
    new_meta = foldin.read_meta(args.new_meta)
    if new_meta[1] != meta[1]:
        raise RuntimeError('%s was not prepared with --vocabulary_from %s: the token ids differ.' % (args.new_meta, args.meta))
    new_index = new_meta[3]
    new_entity_ids = [new_index[e] for e in range(len(new_index))]
    associations = dict((e, new_meta[4].get(e, [])) for e in new_entity_ids)
    W, b = np.asarray(predict_fn.W), np.asarray(predict_fn.b)
    refresh = None
    if args.unfreeze_known:
        # known ids are refreshed in order of first appearance, unknown ones the new columns V_e ..
        extended_meta, refresh, added_ids, slots = foldin.merge_meta(meta, new_entity_ids, associations)
        if not len(refresh) and not added_ids:
            raise RuntimeError('nothing to fold in: %s names no entity.' % args.new_meta)
    if args.label_distributions:
        # known ids keep their trained index -- frozen co-labels, or refreshed with --unfreeze_known --, unknown ones are the
        # new columns V_e ..
        extended_meta, columns, added_ids = foldin.label_columns(meta, new_entity_ids, associations)
        if not added_ids and not args.unfreeze_known:
            raise RuntimeError('nothing to fold in: %s knows every entity id of %s.' % (args.meta, args.new_meta))
        (x, y, w), _ = training.load_data_sets(args.data)
        assert y.shape[1] <= len(new_entity_ids)
        y = foldin.remap_label_columns(y, columns, W.shape[1] + len(added_ids))
    elif args.unfreeze_known:
        x, y, w = one_hot_training_set(args.data)
        assert y.size == 0 or int(y.max()) < len(new_entity_ids)
        y = slots[y] if y.size else y           # (entity index of --new_meta -> slot)
    else:
        # (refuses a known entity id before anything is computed)
        extended_meta = foldin.extend_meta(meta, new_entity_ids, associations)
        added_ids = new_entity_ids
        x, y, w = one_hot_training_set(args.data)
        assert y.size == 0 or int(y.max()) < len(new_entity_ids)
    new_W = models._glorot_uniform((W.shape[0], len(added_ids)))       # as models.LanguageModel initialises W; b: zeros
    fold = foldin.LogLinearFoldIn(R_w, W, b, new_W, None, (x, y, w), batch_size=args.batch_size,
                                  regularization_lambda=args.regularization_lambda, window_size=meta[0].window_size,
                                  device=args.device, refresh=refresh)
    mean, stddev = fold.train_error()
    logging.info('Epoch 0: fold-in error %.6f (stddev %.6f).', mean, stddev)
    for epoch in range(1, args.iterations + 1):
        num_batches, loss = fold.train()
        mean, stddev = fold.train_error()
        logging.info('Epoch %d: %d batches, mean training loss %.6f; fold-in error %.6f (stddev %.6f).',
                     epoch, num_batches, loss, mean, stddev)
    for path in (args.model_output, args.meta_output):
        directory = os.path.dirname(path)
        if directory and not os.path.exists(directory):
            os.makedirs(directory)
    Wn, bn = fold.get_new_dense()
    if refresh is None:
        objects = foldin.extend_ll_dump(model_args, predict_fn, R_w, Wn, bn)
    else:
        Wr, br = fold.get_refreshed_dense()
        objects = foldin.refresh_ll_dump(model_args, predict_fn, R_w, refresh, Wr, br, Wn, bn)
    foldin.write_dump(args.model_output, objects)
    foldin.write_meta(args.meta_output, extended_meta)
    logging.info('Saved the extended model "%s" (%d + %d entities, %d refreshed) and its meta "%s".', args.model_output,
                 W.shape[1], len(added_ids), 0 if refresh is None else len(refresh), args.meta_output)
    fold.close()


def fold_in_words(args):
    """--new_words on a vectorspace dump: the rows of the new words of --new_meta learn (sert_amd.foldin.WordFoldIn)."""
    if args.refresh or args.unfreeze_known or args.label_distributions:
        raise RuntimeError('--new_words folds in words, not entities: --refresh, --unfreeze_known and --label_distributions '
                           'do not apply.')
    model_args, predict_fn, R_w, R_e = load_model(args.model)
    if getattr(model_args, 'type', None) is not models.VectorSpaceLanguageModel:
        raise RuntimeError('--new_words needs a model trained as vectorspace (found %r).' % (getattr(model_args, 'type', None),))
    meta = foldin.read_meta(args.meta)
    new_meta = foldin.read_meta(args.new_meta)
    # (refuses a vocabulary that does not extend the trained one and an entity the model does not know, before anything is computed)
    extended_meta = foldin.extend_meta_words(meta, new_meta)
    new_words = foldin.new_words_of(meta, new_meta)
    if not new_words:
        raise RuntimeError('nothing to fold in: %s holds no word that %s does not know.' % (args.new_meta, args.meta))
    R_w = np.asarray(R_w)
    V_w = R_w.shape[0]
    if V_w != len(meta[1]):
        raise RuntimeError('%s holds %d word rows but %s names %d words: they are not of the same model.'
                           % (args.model, V_w, args.meta, len(meta[1])))
    x, y, w = one_hot_training_set(args.data)
    # labels: entity index of --new_meta -> trained index
    index_of = dict((entity_id, index) for index, entity_id in meta[3].items())
    trained = np.array([index_of[new_meta[3][e]] for e in range(len(new_meta[3]))], dtype=np.int32)
    y = trained[y] if y.size else y.astype(np.int32)
    # a window without a new word cannot move a trainable row
    keep = (np.asarray(x) >= V_w).any(axis=1)
    logging.info('Dropped %d of %d windows that hold no new word.', int((~keep).sum()), int(keep.size))
    if not keep.any():
        raise RuntimeError('nothing to fold in: no window of %s holds a new word.' % args.data)
    x, y = np.asarray(x)[keep].astype(np.int32), y[keep]
    w = None if w is None else np.asarray(w)[keep]
    new_rows = foldin.new_word_rows(V_w, len(new_words), R_w.shape[1])
    fold = foldin.WordFoldIn(
        R_w, R_e, predict_fn.W, predict_fn.b, new_rows, (x, y, w), batch_size=args.batch_size,
        num_negative_samples=args.num_negative_samples, regularization_lambda=args.regularization_lambda,
        window_size=meta[0].window_size, seed=args.seed, device=args.device)
    mean, stddev = fold.train_error()
    logging.info('Epoch 0: fold-in error %.6f (stddev %.6f).', mean, stddev)
    for epoch in range(1, args.iterations + 1):
        num_batches, loss = fold.train()
        mean, stddev = fold.train_error()
        logging.info('Epoch %d: %d batches, mean training loss %.6f; fold-in error %.6f (stddev %.6f).',
                     epoch, num_batches, loss, mean, stddev)
    for path in (args.model_output, args.meta_output):
        directory = os.path.dirname(path)
        if directory and not os.path.exists(directory):
            os.makedirs(directory)
    foldin.write_dump(args.model_output, foldin.extend_words_dump(model_args, predict_fn, R_w, R_e,
                                                                  fold.get_new_word_representations()))
    foldin.write_meta(args.meta_output, extended_meta)
    logging.info('Saved the extended model "%s" (%d + %d words) and its meta "%s".', args.model_output, V_w, len(new_words),
                 args.meta_output)
    fold.close()


def fold_in_ll_words(args):
    """--ll_new_words on a loglinear dump (namespace, LogLinearPredictFn, R_w): the rows of the new words of --new_meta learn
    (sert_amd.foldin.LogLinearWordFoldIn); there are no negatives to draw, so --num_negative_samples is not read.
    --label_rows: the instances keep their label rows, columns moved to the trained entity index."""
    if args.refresh or args.unfreeze_known or args.label_distributions:
        raise RuntimeError('--ll_new_words folds words into a loglinear model, one instance per label: --refresh, '
                           '--unfreeze_known and --label_distributions do not apply.')
    dump = training.read_checkpoint(args.model)
    model_args, predict_fn = dump['args'], dump['predict_fn']
    if getattr(model_args, 'type', None) is not models.LanguageModel:
        raise RuntimeError('--ll_new_words needs a loglinear model: the words of a vectorspace model are folded in with '
                           '--new_words (found %r).' % (getattr(model_args, 'type', None),))
    R_w = np.asarray(dump['tables'][0])
    meta = foldin.read_meta(args.meta)
    new_meta = foldin.read_meta(args.new_meta)
    V_w = R_w.shape[0]
    W, b = np.asarray(predict_fn.W), np.asarray(predict_fn.b)
    if V_w != len(meta[1]) or W.shape[1] != len(meta[3]):
        raise RuntimeError('%s holds %d word rows and %d entities but %s names %d words and %d entities: they are not of the '
                           'same model.' % (args.model, V_w, W.shape[1], args.meta, len(meta[1]), len(meta[3])))
    # (refuses a vocabulary that does not extend the trained one and an entity the model does not know, before anything is computed)
    extended_meta = foldin.extend_meta_words(meta, new_meta)
    new_words = foldin.new_words_of(meta, new_meta)
    if not new_words:
        raise RuntimeError('nothing to fold in: %s holds no word that %s does not know.' % (args.new_meta, args.meta))
    # labels: entity index of --new_meta -> trained index
    index_of = dict((entity_id, index) for index, entity_id in meta[3].items())
    trained = np.array([index_of[new_meta[3][e]] for e in range(len(new_meta[3]))], dtype=np.int32)
    if args.label_rows:
        (x, y, w), _ = training.load_data_sets(args.data)
        assert y.shape[1] <= trained.size
        y = foldin.remap_label_columns(y, trained, W.shape[1])
    else:
        x, y, w = one_hot_training_set(args.data)
        y = trained[y] if y.size else y.astype(np.int32)
    # a window without a new word cannot move a trainable row
    keep = (np.asarray(x) >= V_w).any(axis=1)
    logging.info('Dropped %d of %d windows that hold no new word.', int((~keep).sum()), int(keep.size))
    if not keep.any():
        raise RuntimeError('nothing to fold in: no window of %s holds a new word.' % args.data)
    x, y = np.asarray(x)[keep].astype(np.int32), y[keep]
    w = None if w is None else np.asarray(w)[keep]
    new_rows = foldin.new_word_rows(V_w, len(new_words), R_w.shape[1])
    fold = foldin.LogLinearWordFoldIn(R_w, W, b, new_rows, (x, y, w), batch_size=args.batch_size,
                                      regularization_lambda=args.regularization_lambda, window_size=meta[0].window_size,
                                      device=args.device)
    mean, stddev = fold.train_error()
    logging.info('Epoch 0: fold-in error %.6f (stddev %.6f).', mean, stddev)
    for epoch in range(1, args.iterations + 1):
        num_batches, loss = fold.train()
        mean, stddev = fold.train_error()
        logging.info('Epoch %d: %d batches, mean training loss %.6f; fold-in error %.6f (stddev %.6f).',
                     epoch, num_batches, loss, mean, stddev)
    for path in (args.model_output, args.meta_output):
        directory = os.path.dirname(path)
        if directory and not os.path.exists(directory):
            os.makedirs(directory)
    foldin.write_dump(args.model_output, foldin.extend_ll_words_dump(model_args, predict_fn, R_w,
                                                                     fold.get_new_word_representations()))
    foldin.write_meta(args.meta_output, extended_meta)
    logging.info('Saved the extended model "%s" (%d + %d words) and its meta "%s".', args.model_output, V_w, len(new_words),
                 args.meta_output)
    fold.close()


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        logging_utils.configure_logging(args)
    except IOError:
        return -1
    if args.seed is not None:
        np.random.seed(args.seed)

    if args.new_words and args.ll_new_words:
        raise RuntimeError('--new_words and --ll_new_words exclude each other: --new_words folds words into a vectorspace dump, '
                           '--ll_new_words into a loglinear one.')
    if args.label_rows and (args.new_words or not args.ll_new_words):
        raise RuntimeError('--label_rows needs --ll_new_words: it keeps the label rows of --data for a word fold-in into a '
                           'loglinear model.  A vectorspace model (--new_words) learns from one entity per instance (NCE); an '
                           'entity fold-in into a loglinear model takes label rows with --label_distributions.')
    if args.new_words:
        if getattr(training.read_checkpoint(args.model)['args'], 'type', None) is models.LanguageModel:
            raise RuntimeError('--new_words needs a vectorspace model: the words of a loglinear model are folded in with '
                               '--ll_new_words.')
        return fold_in_words(args)
    if args.ll_new_words:
        return fold_in_ll_words(args)

    # the dump's model type decides: a loglinear dump takes the path of its own, anything else the vectorspace one below
    if getattr(training.read_checkpoint(args.model)['args'], 'type', None) is models.LanguageModel:
        return fold_in_loglinear(args)

    if args.unfreeze_known:
        raise RuntimeError('--unfreeze_known needs a loglinear model: the trained rows of a vectorspace model are refreshed '
                           'with --refresh.')
    if args.label_distributions:
        raise RuntimeError('--label_distributions needs a loglinear model: a vectorspace model learns from one entity per '
                           'instance (NCE), with or without it.')
    model_args, predict_fn, R_w, R_e = load_model(args.model)
    if getattr(model_args, 'type', None) is not models.VectorSpaceLanguageModel:
        raise RuntimeError('a fold-in needs a model trained as vectorspace (found %r).' % (getattr(model_args, 'type', None),))
    meta = foldin.read_meta(args.meta)
    new_meta = foldin.read_meta(args.new_meta)
    if new_meta[1] != meta[1]:
        raise RuntimeError('%s was not prepared with --vocabulary_from %s: the token ids differ.' % (args.new_meta, args.meta))
    new_index = new_meta[3]
    new_entity_ids = [new_index[e] for e in range(len(new_index))]
    associations = dict((e, new_meta[4].get(e, [])) for e in new_entity_ids)
    refresh = None
    if args.refresh:
        extended_meta, refresh, added_ids, slots = foldin.merge_meta(meta, new_entity_ids, associations)
    else:
        # (refuses a known entity id before anything is computed)
        extended_meta = foldin.extend_meta(meta, new_entity_ids, associations)
        added_ids = new_entity_ids

    x, y, w = one_hot_training_set(args.data)
    assert y.size == 0 or int(y.max()) < len(new_entity_ids)
    if args.refresh:
        y = slots[y] if y.size else y           # (entity index of --new_meta -> slot)
    window_size = meta[0].window_size
    new_rows = models._glorot_uniform((len(added_ids), R_e.shape[1]))      # as bin/train.py initialises R_e
    fold = foldin.EntityFoldIn(
        R_w, R_e, predict_fn.W, predict_fn.b, new_rows, (x, y, w), batch_size=args.batch_size,
        num_negative_samples=args.num_negative_samples, regularization_lambda=args.regularization_lambda,
        window_size=window_size, seed=args.seed, device=args.device, refresh=refresh)

    mean, stddev = fold.train_error()
    logging.info('Epoch 0: fold-in error %.6f (stddev %.6f).', mean, stddev)
    for epoch in range(1, args.iterations + 1):
        num_batches, loss = fold.train()
        mean, stddev = fold.train_error()
        logging.info('Epoch %d: %d batches, mean training loss %.6f; fold-in error %.6f (stddev %.6f).',
                     epoch, num_batches, loss, mean, stddev)

    for path in (args.model_output, args.meta_output):
        directory = os.path.dirname(path)
        if directory and not os.path.exists(directory):
            os.makedirs(directory)
    if args.refresh:
        objects = foldin.refresh_dump(model_args, predict_fn, R_w, R_e, refresh, fold.get_refreshed_representations(),
                                      fold.get_new_representations())
    else:
        objects = foldin.extend_dump(model_args, predict_fn, R_w, R_e, fold.get_new_representations())
    foldin.write_dump(args.model_output, objects)
    foldin.write_meta(args.meta_output, extended_meta)
    logging.info('Saved the extended model "%s" (%d + %d entities, %d refreshed) and its meta "%s".', args.model_output,
                 R_e.shape[0], len(added_ids), 0 if refresh is None else len(refresh), args.meta_output)
    fold.close()


if __name__ == "__main__":
    sys.exit(main())
