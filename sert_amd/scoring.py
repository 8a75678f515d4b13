"""Ranker callbacks of the query path.  The reference keeps them inside
bin/query.py (lines 165-382); here they are importable.  A callback receives
what ``sert.inference`` produced for one query -- ``callback(payload, result,
topic_id=...)`` -- and reports a ranking through
``rank_callback(topic_id, entity_indices, scores)`` (best first).

  LogLinearCallback    result = (T, V_e) per-token entity distributions.
                       Score = product over the tokens (zeros skipped),
                       renormalised; EVERY entity is ranked (query.py:199-236).
                       ``process_batch`` takes the ranking of all queries of a
                       run from ONE device call (sert_ll_rank_queries; with
                       candidate lists sert_ll_rank_candidates, which ranks
                       and copies out the listed entities only).
  VectorSpaceCallback  result = (1, d_e) query projection.  Score of an entity =
                       (cosine + 1) / 2 against the L2-normalised entity table;
                       the best --top entities (or all) are ranked
                       (query.py:239-370).  Normalisation, the scoring GEMM and
                       the top-k selection run on the MI355X (sert_scorer_* of
                       include/sert_hip.h); ``process_batch`` scores all queries
                       of a run in ONE device call.
"""
import logging

import numpy as np

from sert_amd import _capi, inference, math_utils


def compute_normalised_entropy(distribution, base=2):
    """Normalised Shannon entropy of every row of a (T, V_e) matrix of
    distributions (each row must sum to one)."""
    assert distribution.ndim == 2
    assert np.allclose(distribution.sum(axis=1), 1.0)
    return [math_utils.entropy(row, base=base, normalize=True) for row in distribution]


class Callback(object):
    """Shared bookkeeping: remembers the raw result per topic and refuses to see
    a topic twice."""

    def __init__(self, args, model_args, tokens, f_debug_out, rank_callback):
        self.args, self.model_args = args, model_args
        self.tokens = tokens
        self.f_debug_out = f_debug_out
        self.rank_callback = rank_callback
        self.topic_projections = {}

    def _remember(self, topic_id, result):
        assert topic_id not in self.topic_projections
        self.topic_projections[topic_id] = np.ravel(result)

    def __call__(self, payload, result, topic_id):
        self._remember(topic_id, result)
        logging.debug('Result of shape %s for topic "%s".', result.shape, topic_id)
        self.process(payload, result, topic_id)

    def process(self, payload, distribution, topic_id):
        raise NotImplementedError()

    def should_average_input(self):
        raise NotImplementedError()


def _candidate_array(candidates, topic_id):
    """The candidate entity indices of a topic; none at all for a topic without a list."""
    return np.asarray(candidates.get(topic_id, ()), dtype=np.int64).reshape(-1)


class LogLinearCallback(Callback):
    """``candidates`` (optional): topic id -> array of internal entity indices.  When given, the ranking of a topic is
    filtered to its candidates before ``rank_callback``: same order, same scores.  The scores stay normalised over ALL
    entities (the model's distribution is over the whole collection), so those of a filtered ranking do not sum to one.
    The batched front end asks ``candidate_lists`` for the lists and has the device rank only them
    (sert_ll_rank_candidates): the same rank_callback calls, without the (Q, V_e) ranking crossing to the host."""

    def __init__(self, *args, **kwargs):
        self.candidates = kwargs.pop('candidates', None)
        super(LogLinearCallback, self).__init__(*args, **kwargs)

    def should_average_input(self):
        return False

    def candidate_lists(self, kwargs_list):
        """The candidate list of every query of ``kwargs_list`` (their submit() keywords), None without candidates; a topic
        without a list has an empty one."""
        if self.candidates is None:
            return None
        return [_candidate_array(self.candidates, kw['topic_id']) for kw in kwargs_list]

    def _report(self, topic_id, idx, score):
        if self.candidates is not None:
            keep = np.isin(idx, _candidate_array(self.candidates, topic_id))
            idx, score = idx[keep], score[keep]
        self.rank_callback(topic_id, idx, score)

    def process(self, payload, distribution, topic_id):
        per_token_entropy = compute_normalised_entropy(distribution, base=2)

        joint = inference.aggregate_distribution(distribution, mode='product', axis=0)
        assert joint.ndim == 1
        joint /= joint.sum()
        mass = joint.sum()
        if not np.isclose(mass, 1.0):
            logging.error('Encountered non-normalized distribution for topic "%s" '
                          '(mass=%.10f).', topic_id, mass)

        if self.f_debug_out is not None:
            words = [self.tokens[token] for token in payload]
            self.f_debug_out.write('Topic {0} {1}: {2}\n'.format(
                topic_id, math_utils.entropy(joint, base=2, normalize=True),
                list(zip(words, per_token_entropy))))

        # ascending argsort read backwards = best first; all V_e entities are ranked
        order = np.argsort(joint)[::-1]
        self._report(topic_id, order, joint[order])

    def process_batch(self, payloads, ranking, kwargs_list):
        """Additive: the queries of a run ranked on the device (inference.QueryRanking, from
        LogLinearPredictFn.rank_queries).  Per query, in order: the same ``_debug`` line, the same
        non-normalised-mass error and the same rank_callback call as ``process``.  A query whose status is
        HOST (joint sum 0 or not finite) goes through ``process`` itself, on the distributions
        ``ranking.distributions_of`` computes for it.

        A candidate ranking (``ranking.candidates``: each query's list ranked by the device) is reported as it is, without
        a second filter; its HOST queries take ``process`` and its filter as before.

        ``topic_projections`` holds, for a device-ranked query, its normalised joint in entity order when
        ``ranking.k`` is None, else the scores of its ranked k best in rank order (``process`` stores the
        raveled per-token distributions); for a device-ranked candidate query, whatever k, the ranked scores of its list in
        rank order -- the joint of the unlisted entities never leaves the device."""
        etype = type(math_utils.entropy(np.full(2, 0.5, np.float32), base=2, normalize=True))
        for q, (payload, kw) in enumerate(zip(payloads, kwargs_list)):
            topic_id = kw['topic_id']
            if ranking.status[q] == inference.QueryRanking.HOST:
                self(payload, ranking.distributions_of(q), **kw)
                continue
            idx, score = ranking.idx[q], ranking.score[q]
            listed = getattr(ranking, 'candidates', False)
            if ranking.k is None and not listed:
                joint = np.empty(score.shape[0], dtype=score.dtype)
                joint[idx] = score
                self._remember(topic_id, joint)
                mass = joint.sum()
                if not np.isclose(mass, 1.0):
                    logging.error('Encountered non-normalized distribution for topic "%s" '
                                  '(mass=%.10f).', topic_id, mass)
            else:
                self._remember(topic_id, score)
            if self.f_debug_out is not None:
                words = [self.tokens[token] for token in payload]
                self.f_debug_out.write('Topic {0} {1}: {2}\n'.format(
                    topic_id, etype(ranking.joint_entropy[q]),
                    list(zip(words, [etype(h) for h in ranking.token_entropy[q]]))))
            if listed:
                self.rank_callback(topic_id, idx, score)
            else:
                self._report(topic_id, idx, score)


class VectorSpaceCallback(Callback):
    """``candidates`` (optional): topic id -> array of internal entity indices.  When given, each topic's candidates -- not
    every entity -- are scored and ranked on the device (Scorer.rank_candidates; --top is its k), ``process_batch`` in one
    call for all topics; a topic without a list gets an empty ranking.  ``rank_callback`` is called as without."""

    def __init__(self, entity_representations, *args, **kwargs):
        self.device = kwargs.pop('device', 0)
        self.candidates = kwargs.pop('candidates', None)
        super(VectorSpaceCallback, self).__init__(*args, **kwargs)

        num_entities = entity_representations.shape[0]
        logging.info('Initializing k-NN for entity representations of shape %s.',
                     entity_representations.shape)

        k = self.args.top
        if k is None:
            logging.warning('Parameter k not set; defaulting to all entities (k=%d).',
                            num_entities)
        elif k > num_entities:
            logging.warning('Parameter k exceeds number of entities; '
                            'defaulting to all entities (k=%d).', num_entities)
            k = None
        self.n_neighbors = k

        # cosine ranking == euclidean k-NN on unit vectors; the device copy of the
        # table is normalised, the caller's array is left as it was
        self.normalize_representations = True
        self.scorer = _capi.Scorer(entity_representations, device=self.device)
        logging.info('Cosine scoring on %s.', _capi.device_info(self.device))

    def should_average_input(self):
        return True

    def _as_queries(self, projections, count):
        q = np.asarray(projections, dtype=np.float32).reshape(count, -1)
        assert q.shape[1] == self.model_args.entity_representation_size
        return q

    def process(self, payload, result, topic_id):
        identity = inference.aggregate_distribution(result, mode='identity', axis=0)
        rows = 1 if identity.ndim == 1 else identity.shape[0]
        assert rows == 1, 'one centroid per query'
        if self.candidates is not None:
            _, idx, score = self.scorer.rank_candidates(self._as_queries(identity, 1),
                                                        [_candidate_array(self.candidates, topic_id)], self.n_neighbors)
            self.rank_callback(topic_id, idx.astype(np.int64), score)
            return
        idx, score = self.scorer.rank(self._as_queries(identity, 1), self.n_neighbors)
        self.rank_callback(topic_id, idx[0].astype(np.int64), score[0])

    def process_batch(self, payloads, projections, kwargs_list):
        """Additive: all queued queries at once (the query block is built in the scorer's
        page-locked buffer, so it is uploaded without a staging copy)."""
        queries = self.scorer.query_buffer(len(payloads))
        np.copyto(queries, self._as_queries(projections, len(payloads)))
        for kw, q in zip(kwargs_list, queries):
            # (a copy: `queries` is the scorer's reusable page-locked block, overwritten by the next call)
            self._remember(kw['topic_id'], q.copy())
        if self.candidates is not None:
            at, idx, score = self.scorer.rank_candidates(
                queries, [_candidate_array(self.candidates, kw['topic_id']) for kw in kwargs_list], self.n_neighbors)
            for row, kw in enumerate(kwargs_list):
                self.rank_callback(kw['topic_id'], idx[at[row]:at[row + 1]].astype(np.int64), score[at[row]:at[row + 1]])
            return
        idx, score = self.scorer.rank(queries, self.n_neighbors)
        for row, kw in enumerate(kwargs_list):
            self.rank_callback(kw['topic_id'], idx[row].astype(np.int64), score[row])
