"""Retrieval quality of the model that is being trained (additive; no counterpart in sert/).

The reference's pipelines choose the epoch by retrieval quality: dump every epoch, start
bin/query.py per dump, run trec_eval per run file, keep the best validation ``ndcg_cut_100``
(product-search.sh:136-170; W3C-expert-finding.sh:108-124 reports ndcg, map, recip_rank, P_5).
``RetrievalEvaluator`` does the same against the LIVE model: topics and relevance judgements
are uploaded to the model's device once, ``evaluate()`` ranks every topic with the parameters
as they are at that moment and computes the per-topic metrics on the device
(include/sert_hip.h: sert_reval_*).  Only the (topics, 5) float64 figures come back.

DEPTH.  A loglinear model ranks any depth.  A vectorspace model ranks up to min(entities, 1024)
entities per topic through the top-k kernels; for every other depth -- ``k=None`` (every
entity), k above 1024, k above the number of entities -- the evaluator does not rank at all:
every figure depends only on the ranks of the topic's judged entities, and those are counted
in one pass over the topic's cosine row (sert_reval_create_counted; DESIGN.md, "Evaluation
depth without a sort").  ``metrics_from_ranks`` is that definition on the host.

Population (``trec_utils.evaluate_run``'s rule): the means run over the topics OF THE QREL
FILE.  A judged topic that is absent from the topics file, or none of whose terms is in the
vocabulary (bin/query.py:129-137 skips it), scores 0 on every metric.

Judgements of entities the model does not know count in the ideal DCG and in the number of
relevant entities (they are relevant and cannot be retrieved) but are not uploaded.

TIES.  The device ranks equal scores by lowest entity index.  A run file put through
``trec_utils.evaluate_run`` (or trec_eval) is re-sorted, equal scores by entity id descending.
The evaluator scores the ranking the device produced; on a ranking with tied scores inside
the evaluated depth the two can differ, on a tie-free one they agree.
"""
import collections
import math

import numpy as np

from sert_amd import _capi, inference
from sert_amd.utils import trec_utils

METRICS = ('ndcg', 'map', 'recip_rank', 'P_5', 'num_rel_ret')     # columns of sert_reval_run, in order


def topic_tokens(text, words):
    """In-vocabulary token ids of a topic; OOV terms are dropped (bin/query.py:129-137)."""
    ids = []
    for term in trec_utils.parse_query(text):
        entry = words.get(term)
        if entry is not None:
            ids.append(entry.id)
    return ids


def ideal_dcg(relevance, depth):
    """Float64 ideal DCG at `depth` over ALL judgements of a topic -- the denominator of trec_utils.ndcg_at_k."""
    ideal = sorted((r for r in relevance.values() if r > 0), reverse=True)[:depth]
    return sum(g / math.log2(i + 2) for i, g in enumerate(ideal))


def host_metrics(ranked_entities, relevance, depth):
    """The evaluator's metrics of one topic on the host: the trec_utils functions on the first `depth` entries of a
    ranking of entity ids.  What the device kernel is checked against, and the path of a topic the device hands back."""
    ranked = list(ranked_entities)[:depth]
    return {'ndcg': trec_utils.ndcg_at_k(ranked, relevance, depth),
            'map': trec_utils.average_precision(ranked, relevance),
            'recip_rank': trec_utils.reciprocal_rank(ranked, relevance),
            'P_5': trec_utils.precision_at(ranked, relevance, 5),
            'num_rel_ret': float(sum(1 for e in ranked if relevance.get(e, 0.0) > 0))}


def metrics_from_ranks(ranks, gains, depth, ideal_dcg, num_rel):
    """The evaluator's metrics of one topic from the 1-based RANKS of its judged entities (those the model knows), in
    float64: what the device computes for a counted handle (csrc/kernels_reval.h: reval_metrics_from_ranks), restated.

    ranks / gains: aligned, one entry per judged entity; ranks pairwise distinct.  Only entries of rank <= depth count.
    ideal_dcg / num_rel: over ALL the topic's judgements, as ``ideal_dcg()`` and the number of gains > 0 give them.
    -> dict over METRICS, equal to ``host_metrics`` on any ranking that places those entities at those ranks."""
    inside = [(int(r), float(g)) for r, g in zip(ranks, gains) if int(r) <= depth]
    dcg = 0.0
    for r, g in inside:                         # (every judged entity, whatever the sign of its gain: trec_utils.ndcg_at_k)
        dcg += g / math.log2(r + 1)
    hit_ranks = sorted(r for r, g in inside if g > 0)
    ap = 0.0
    for h, r in enumerate(hit_ranks, 1):        # (h: the hits of rank <= r)
        ap += h / float(r)
    return {'ndcg': dcg / ideal_dcg if ideal_dcg > 0 else 0.0,
            'map': ap / num_rel if num_rel > 0 else 0.0,
            'recip_rank': 1.0 / hit_ranks[0] if hit_ranks else 0.0,
            'P_5': sum(1 for r in hit_ranks if r <= 5) / 5.0,
            'num_rel_ret': float(len(hit_ranks))}


TOPK_MAX = 1024       # the deepest ranking of sert_scorer_topk, and so of a vectorspace handle of sert_reval_create


def uses_counting(kind, k, num_entities):
    """Whether RetrievalEvaluator evaluates a model of `kind` at depth k through a counted handle: a vectorspace kind at any
    depth sert_reval_create refuses for it (k None, above 1024, above the number of entities)."""
    return kind != _capi.KIND_LOGLINEAR and (k is None or k > min(num_entities, TOPK_MAX))


ZERO = dict((name, 0.0) for name in METRICS)

EvalArrays = collections.namedtuple(
    'EvalArrays', 'population device_topics token_lists judgements ideal_dcg num_rel depth num_entities')


def build_arrays(topics, qrels, words, entity_indices_inv, k=None):
    """Host half of the evaluator: what sert_reval_create is given.

    topics: topic id -> text (trec_utils.parse_topics); qrels: topic id -> {entity id -> relevance}
    (trec_utils.parse_qrels); words: word -> entry with ``.id``; entity_indices_inv: internal entity index ->
    entity id (the 4th pickle of bin/prepare.py's meta file); k: entities ranked per topic, None = all.

    -> EvalArrays: ``population`` every topic of the qrels in file order; ``device_topics`` those of them that have a
    topic text with at least one in-vocabulary term, with per device topic its ``token_lists`` entry, its ``judgements``
    (internal indices ascending, gains) of KNOWN entities, its float64 ``ideal_dcg`` at ``depth`` and ``num_rel`` over all
    its judgements."""
    num_entities = len(entity_indices_inv)
    index_of = dict((str(entity_id), index) for index, entity_id in entity_indices_inv.items())
    depth = num_entities if k is None or k >= num_entities else int(k)
    population = list(qrels.keys())
    device_topics, token_lists, judgements, idcg, num_rel = [], [], [], [], []
    for topic in population:
        if topic not in topics:
            continue
        tokens = topic_tokens(topics[topic], words)
        if not tokens:
            continue
        relevance = qrels[topic]
        known = sorted((index_of[str(e)], float(r)) for e, r in relevance.items() if str(e) in index_of)
        device_topics.append(topic)
        token_lists.append(tokens)
        judgements.append((np.asarray([i for i, _ in known], dtype=np.int32),
                           np.asarray([r for _, r in known], dtype=np.float32)))
        idcg.append(ideal_dcg(relevance, depth))
        num_rel.append(sum(1 for r in relevance.values() if r > 0))
    return EvalArrays(population, device_topics, token_lists, judgements,
                      np.asarray(idcg, dtype=np.float64), np.asarray(num_rel, dtype=np.int32), depth, num_entities)


def mean_figures(table, depth, num_entities):
    """table: (population, len(METRICS)) float64 in topic order, zero rows for topics without figures -> the means, each a
    float64 sum over the column in topic order (the builtin sum over a list: no tree, no blocks) over the population size.

    The NDCG entry is named after what was ranked, as trec_eval names it: 'ndcg_cut_K' when the depth K cuts the ranking,
    'ndcg' when every entity is ranked -- also when a requested K is not below the number of entities (--eval_top 100 on a
    collection of 60 entities writes 'ndcg').  Readers that must not care use ndcg_key()."""
    n = max(1, table.shape[0])
    ndcg_name = 'ndcg' if depth >= num_entities else 'ndcg_cut_%d' % depth
    result = {}
    for c, name in enumerate(METRICS[:4]):
        result[ndcg_name if name == 'ndcg' else name] = sum(table[:, c].tolist()) / n
    result['num_q'] = int(table.shape[0])
    return result


def summarise(population, per_topic, depth, num_entities):
    """The means of mean_figures from a dict topic -> metrics; a topic of the population without an entry scores 0."""
    table = np.zeros((len(population), len(METRICS)), dtype=np.float64)
    for row, topic in enumerate(population):
        figures = per_topic.get(topic)
        if figures is not None:
            table[row] = [figures[name] for name in METRICS]
    result = mean_figures(table, depth, num_entities)
    result['per_topic'] = per_topic
    return result


def ndcg_key(result):
    """The name of the NDCG entry of an evaluate() result ('ndcg_cut_K' or 'ndcg')."""
    return next(name for name in result if name.startswith('ndcg'))


class RetrievalEvaluator(object):
    """NDCG / MAP / reciprocal rank / P@5 of `model` on a topic set, computed on the model's device.

    ``evaluate()`` may be called at any point between training steps; it changes nothing the training depends on.
    Data parallel: collective, every rank calls it (the word table is gathered first).  See the module docstring for
    the population rule, unknown entities and ties."""

    def __init__(self, model, topics, qrels, words, entity_indices_inv, k=None):
        self.model = model
        self.entity_indices_inv = entity_indices_inv
        self.qrels = qrels
        self.arrays = build_arrays(topics, qrels, words, entity_indices_inv, k)
        self.k = k
        row_of = dict((topic, row) for row, topic in enumerate(self.arrays.population))
        self._rows = np.asarray([row_of[topic] for topic in self.arrays.device_topics], dtype=np.int64)   # device topic -> population row
        self._eval = None
        if self.arrays.device_topics:
            a = self.arrays
            counted = uses_counting(model._engine.cfg.kind, k, a.num_entities)
            self._eval = _capi.RetrievalEval(model._engine, a.token_lists, a.judgements, a.ideal_dcg, a.num_rel, k, counted=counted)

    def _host_topic(self, tokens, relevance):
        """A loglinear topic the device could not rank (joint sum 0 or not finite): the per-token host path of
        bin/query.py (WordBatcher -> predict_fn -> LogLinearCallback.process' ranking), then the trec_utils functions."""
        model = self.model
        got = []
        batcher = inference.WordBatcher(model.predict_fn, model.batch_size, model.window_size,
                                        np.min_scalar_type(model.vocabulary_size - 1),
                                        lambda payload, distribution: got.append(distribution))
        batcher.submit(tokens)
        batcher.process()
        joint = inference.aggregate_distribution(got[0], mode='product', axis=0)
        joint /= joint.sum()
        order = np.argsort(joint)[::-1]
        ranked = [str(self.entity_indices_inv[int(i)]) for i in order[:self.arrays.depth]]
        return host_metrics(ranked, dict((str(e), r) for e, r in relevance.items()), self.arrays.depth)

    def evaluate(self, per_topic=True):
        """-> {'ndcg_cut_K' | 'ndcg', 'map', 'recip_rank', 'P_5', 'num_q'[, 'per_topic': topic -> metrics]}.

        The device's (topics, 5) array is placed into the population's rows and the means are taken over its columns; no
        Python object is made per topic unless ``per_topic`` is asked for (the epoch driver does not: at 10 000 topics
        the dicts cost several times the device's work)."""
        a = self.arrays
        table = np.zeros((len(a.population), len(METRICS)), dtype=np.float64)
        metrics = None
        if self._eval is not None:
            metrics, status = self._eval.run()
            for q in np.flatnonzero(status == _capi.LL_STATUS_HOST):
                figures = self._host_topic(a.token_lists[q], self.qrels[a.device_topics[q]])
                metrics[q] = [figures[name] for name in METRICS]
            table[self._rows] = metrics
        result = mean_figures(table, a.depth, a.num_entities)
        if per_topic:
            result['per_topic'] = {} if metrics is None else dict(
                (topic, dict(zip(METRICS, row))) for topic, row in zip(a.device_topics, metrics.tolist()))
        return result

    def close(self):
        if self._eval is not None:
            self._eval.close()
            self._eval = None
