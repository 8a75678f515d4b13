#!/usr/bin/env python
"""Training CLI -- drop-in for the reference's bin/train.py (same flags, same
files in and out), executed on MI355X through sert_amd.models.

    python bin/train.py --data data.npz --meta meta --type vectorspace \
        --batch_size 4096 --word_representation_size 300 \
        --entity_representation_size 128 --num_negative_samples 10 \
        --one_hot_classes --iterations 15 --model_output model

Inputs (bin/prepare.py:372-416): ``data.npz`` with x_train (N,n) uint,
y_train (0-d object array holding a csr_matrix (N,V_e) f32), optional w_train,
x_validate, y_validate; ``meta`` = pickle stream (args, words, tokens, ...).
Output: ``<model_output>_<epoch>.bin`` = pickle stream [args, predict_fn, R_w,
(R_e)] (bin/train.py:289-300) readable by bin/query.py.

Additive: --type vectorspace_softmax, --ignore_weights (the reference reads
args.ignore_weights but never defines it, train.py:81), --seed, --device,
--save_optimizer_state, --resume <model_k.bin> (continue behind epoch k of a run that was
dumped with --save_optimizer_state: same results as the uninterrupted run), --gpus N
(data parallel over N GPUs of this node, one process each, started by this script;
--batch_size is the GLOBAL batch).  Any launcher that sets RANK / LOCAL_RANK / WORLD_SIZE
works as well.  --eval_topics FILE... --eval_qrels NAME=FILE... [--eval_top K]: retrieval
quality (NDCG, MAP, reciprocal rank, P@5) of the live model on every named qrel set, on the
device, before epoch 1 and after every epoch; written to <model_output>_retrieval.json and
the best epoch by the first set's NDCG logged at the end (sert_amd/evaluation.py).  K is the
evaluated depth, any positive number for either model kind (default: every entity for
loglinear, min(100, entities) for vectorspace); K at or above the number of entities means
every entity, and the NDCG entry is then named 'ndcg' instead of 'ndcg_cut_K'.  A vectorspace
depth above 1024 is evaluated without ranking, by counting the judged entities' ranks.
"""
import argparse
import logging
import os
import pickle
import sys

import numpy as np
import scipy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import distributed, models, training  # noqa: E402
from sert_amd.training import error_delta, sparse_to_one_hot_multiple, train  # noqa: E402,F401
from sert_amd.utils import argparse_utils as au  # noqa: E402
from sert_amd.utils import embedding_utils, logging_utils  # noqa: E402

MODELS = {
    'loglinear': models.LanguageModel,
    'vectorspace': models.VectorSpaceLanguageModel,
    # additive (not in the reference): vectorspace encoder + full softmax over entities
    'vectorspace_softmax': models.VectorSpaceSoftmaxLanguageModel,
}

def named_file(value):
    """NAME=FILE -> (NAME, FILE), e.g. validation=qrel_validation."""
    name, sep, path = value.partition('=')
    if not sep or not name:
        raise argparse.ArgumentTypeError('expected NAME=FILE, got %r' % value)
    return name, au.existing_file_path(path)


def retrieval_evaluators(args, model, words, entity_indices_inv):
    """[(set name, RetrievalEvaluator)] of --eval_topics / --eval_qrels, in the order given."""
    from sert_amd import evaluation
    from sert_amd.utils import trec_utils
    handles = [open(name, 'r') for name in args.eval_topics]
    try:
        topics = trec_utils.parse_topics(handles)
    finally:
        for handle in handles:
            handle.close()
    k = getattr(args, 'eval_top', None)
    if k is None and args.type is not models.LanguageModel:
        k = min(100, len(entity_indices_inv))       # (the product-search setting, --top 100)
    evaluators = []
    for name, path in args.eval_qrels:
        with open(path, 'r') as f:
            qrels = trec_utils.parse_qrels(f)
        evaluators.append((name, evaluation.RetrievalEvaluator(model, topics, qrels, words, entity_indices_inv, k)))
    return evaluators


# (flag, keyword arguments) -- the reference's surface first (train.py:28-61)
FLAGS = [
    ('--loglevel', dict(type=str, default='INFO')),
    ('--data', dict(type=au.existing_file_path, required=True)),
    ('--meta', dict(type=au.existing_file_path, required=True)),
    ('--type', dict(choices=sorted(MODELS), required=True)),
    ('--iterations', dict(type=au.positive_int, default=1)),
    ('--batch_size', dict(type=au.positive_int, default=1024)),
    ('--word_representation_size', dict(type=au.positive_int, default=300)),
    ('--representation_initializer', dict(type=au.existing_file_path, default=None)),
    ('--entity_representation_size', dict(type=au.positive_int, default=None)),
    ('--num_negative_samples', dict(type=au.positive_int, default=None)),
    ('--one_hot_classes', dict(action='store_true', default=False)),
    ('--regularization_lambda', dict(type=au.ratio, default=0.01)),
    ('--model_output', dict(type=str, required=True)),
    # additive
    ('--ignore_weights', dict(action='store_true', default=False)),
    ('--seed', dict(type=int, default=None)),
    ('--device', dict(type=int, default=None)),
    ('--save_optimizer_state', dict(action='store_true', default=False)),
    ('--resume', dict(type=au.existing_file_path, default=None)),
    ('--gpus', dict(type=au.positive_int, default=1)),
    # retrieval evaluation per epoch; absent from the namespace (which is pickled into every dump) unless given
    ('--eval_topics', dict(type=au.existing_file_path, nargs='+', default=argparse.SUPPRESS)),
    ('--eval_qrels', dict(type=named_file, nargs='+', default=argparse.SUPPRESS, metavar='NAME=FILE')),
    ('--eval_top', dict(type=au.positive_int, default=argparse.SUPPRESS, metavar='K',
                        help='evaluated depth: any K >= 1 for either model kind; K at or above the number of entities '
                             'evaluates every entity (the NDCG entry is then named ndcg).  Default: every entity for '
                             'loglinear, min(100, entities) for vectorspace.')),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    for flag, kwargs in FLAGS:
        parser.add_argument(flag, **kwargs)
    return parser


def glorot_uniform(shape):
    """U(-a, a), a = sqrt(6 / (rows + cols)), from the global np.random -- what
    lasagne.init.GlorotUniform().sample gives at train.py:128-129 and :170-171."""
    limit = np.sqrt(6.0 / sum(shape))
    return np.random.uniform(-limit, limit, size=shape).astype(np.float32)


def initial_word_representations(args, words, tokens):
    table = glorot_uniform((len(words), args.word_representation_size))
    if not args.representation_initializer:
        return table
    # pre-trained vectors override the random rows; for duplicated words in the
    # initialiser file the last one wins (train.py:131-151)
    pretrained = dict(embedding_utils.load_binary_representations(
        args.representation_initializer, tokens))
    hits = 0
    for word, entry in words.items():
        vector = pretrained.get(word.lower())
        if vector is not None:
            table[entry.id] = vector
            hits += 1
    logging.info('Initialized representations from pre-learned collection '
                 'for %d words (%.2f%%).', hits, 100.0 * hits / float(len(words)))
    return table


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    evaluate_retrieval = hasattr(args, 'eval_topics') or hasattr(args, 'eval_qrels')
    if evaluate_retrieval and not (hasattr(args, 'eval_topics') and hasattr(args, 'eval_qrels')):
        parser.error('--eval_topics and --eval_qrels go together')
    if hasattr(args, 'eval_top') and not evaluate_retrieval:
        parser.error('--eval_top needs --eval_topics and --eval_qrels')
    if args.entity_representation_size is None:
        args.entity_representation_size = args.word_representation_size
    # the model class itself travels in the dumped namespace (train.py:68)
    args.type = MODELS[args.type]

    try:
        logging_utils.configure_logging(args)
    except IOError:
        return -1
    logging_utils.log_module_info(np, scipy)

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # one process per GPU, started here; this process only waits for them
        command = [sys.executable, os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv)
        return distributed.launch(command, args.gpus)

    ctx = distributed.init_from_env()
    if args.seed is not None:
        np.random.seed(args.seed)
    elif ctx.world_size > 1:
        np.random.seed(distributed.broadcast_object(int(np.random.randint(1 << 30))))

    training_set, validation_set = training.load_data_sets(args.data, args.ignore_weights)
    num_entities = training_set[1].shape[1]
    assert num_entities > 1
    if args.one_hot_classes:
        training_set, validation_set = training.to_one_hot(training_set, validation_set)

    logging.info('Loading meta-data from %s.', args.meta)
    with open(args.meta, 'rb') as f:
        # args of prepare, word -> entry(.id), id -> word; the entity maps that
        # follow in the stream are only needed at query time
        data_args, words, tokens = (pickle.load(f) for _ in range(3))
        entity_indices_inv = pickle.load(f) if evaluate_retrieval else None

    options = dict(
        batch_size=args.batch_size,
        window_size=data_args.window_size,
        representations_init=distributed.broadcast_array(
            initial_word_representations(args, words, tokens)),
        regularization_lambda=args.regularization_lambda,
        training_set=training_set,
        validation_set=validation_set)
    eval_words = words if evaluate_retrieval else None
    del words, tokens

    if args.type is models.LanguageModel:
        options['output_layer_size'] = num_entities
    else:
        options['entity_representations_init'] = distributed.broadcast_array(
            glorot_uniform((num_entities, args.entity_representation_size)))
        options['num_negative_samples'] = args.num_negative_samples

    if args.device is not None:
        args.type.device = args.device
    checkpoint = None
    if args.resume:
        checkpoint = training.read_checkpoint(args.resume)
        if checkpoint['trailer'] is not None:   # the sampler seed is fixed at construction
            args.type.sampler_seed = checkpoint['trailer']['sampler_state']['seed']
    model = args.type(**options)
    if checkpoint is not None:
        training.restore(model, checkpoint)

    extras = {}
    if evaluate_retrieval:
        extras['retrieval'] = retrieval_evaluators(args, model, eval_words, entity_indices_inv)
    train(model, args.iterations, args.model_output,
          abort_threshold=1e-5, early_stopping=False,
          additional_args=[args],
          save_optimizer_state=args.save_optimizer_state,
          resume_from=checkpoint, **extras)

    distributed.shutdown()


if __name__ == "__main__":
    sys.exit(main())
