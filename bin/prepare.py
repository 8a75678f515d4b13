#!/usr/bin/env python
"""Instance generator CLI -- drop-in for the reference's bin/prepare.py flags:
TREC-text documents + ``entity document 1`` associations -> ``--data_output``
(npz) and ``--meta_output`` (pickle stream) for bin/train.py / bin/query.py.

    python bin/prepare.py --seed 1 docs/*.trectext --assoc_path assocs \
        --window_size 4 --overlapping --resample --no_instance_weights \
        --meta_output meta --data_output data.npz

``--remove_stopwords nltk`` (the default) uses a built-in English stop list
because nltk is unavailable offline; ``--num_workers`` is accepted and ignored
(single process).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sert_amd import prepare as prep  # noqa: E402
from sert_amd.utils import argparse_utils as au  # noqa: E402
from sert_amd.utils import logging_utils  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--loglevel', type=str, default='INFO')
    p.add_argument('--seed', type=au.positive_int, required=True)
    p.add_argument('document_paths', type=au.existing_file_path, nargs='+')
    p.add_argument('--encoding', type=str, default='latin1')
    p.add_argument('--assoc_path', type=au.existing_file_path, required=True)
    p.add_argument('--num_workers', type=int, default=1)
    p.add_argument('--vocabulary_min_count', type=int, default=2)
    p.add_argument('--vocabulary_min_word_size', type=int, default=2)
    p.add_argument('--vocabulary_max_size', type=int, default=65536)
    p.add_argument('--remove_stopwords', type=str, default='nltk')
    p.add_argument('--validation_set_ratio', type=au.ratio, default=0.01)
    p.add_argument('--window_size', type=int, default=10)
    p.add_argument('--overlapping', action='store_true', default=False)
    p.add_argument('--stride', type=au.positive_int, default=None)
    p.add_argument('--resample', action='store_true', default=False)
    p.add_argument('--no_shuffle', action='store_true', default=False)
    p.add_argument('--no_padding', action='store_true', default=False)
    p.add_argument('--no_instance_weights', action='store_true', default=False)
    p.add_argument('--meta_output', type=au.nonexisting_file_path, required=True)
    p.add_argument('--data_output', type=au.nonexisting_file_path, required=True)
    # additive (bin/fold_in.py); absent from the namespace (which is pickled into the meta) unless given
    p.add_argument('--vocabulary_from', type=au.existing_file_path, default=argparse.SUPPRESS, metavar='META',
                   help='take the vocabulary (token ids) of a trained model\'s meta file instead of extracting one: '
                        'for documents of entities that are folded into that model; out-of-vocabulary tokens are dropped')
    p.add_argument('--extend_vocabulary', action='store_true', default=argparse.SUPPRESS,
                   help='with --vocabulary_from META: tokens of the documents outside META\'s vocabulary that pass '
                        '--vocabulary_min_count, --vocabulary_min_word_size and the stop list are appended as ids V_w, V_w + 1, ... '
                        '(count descending, then word; at most --vocabulary_max_size words in all) instead of dropped: for '
                        'bin/fold_in.py --new_words.  The trained ids do not move.')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        logging_utils.configure_logging(args)
    except IOError:
        return -1
    if args.remove_stopwords not in ('none', 'nltk') and not os.path.exists(args.remove_stopwords):
        sys.stderr.write('Invalid stopword removal strategy "%s".\n' % args.remove_stopwords)
        return -1
    for path in (args.meta_output, args.data_output):
        directory = os.path.dirname(path)
        if directory and not os.path.exists(directory):
            os.makedirs(directory)
    prep.prepare(args)


if __name__ == "__main__":
    sys.exit(main())
