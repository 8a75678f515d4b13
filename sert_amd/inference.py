"""Drop-in for ``sert.inference`` (query batching in front of predict_fn).

Same entry point and classes as the reference (sert/inference.py):
``create(predict_fn, word_representations, batch_size, window_size,
vocabulary_size, result_callback)`` returns an object with
``submit(query_tokens, **kwargs)`` and ``process()``.

  * loglinear  -> WordBatcher: packs query tokens row-major into a fixed
    (batch_size, window_size) id batch + int8 mask, flushing through
    predict_fn when full (inference.py:28-143);
  * vectorspace -> EmbeddingMapper: mean of the query's word vectors ->
    predict_fn -> callback, one query at a time (inference.py:146-167).

Additive: ``create(..., batched=True)`` returns a BatchedEmbeddingMapper that
defers all queries to ``process()`` and pushes them through predict_fn and the
callback's ``process_batch`` in ONE device call each (the 10k x 100k scoring
config of BASELINE.json); for loglinear (a predict_fn with ``rank_queries``) a
BatchedWordRanker that ranks all queued queries in one ``rank_queries`` call, the
per-token distributions staying on the device.
"""
import logging

import numpy as np


def create(predict_fn, word_representations,
           batch_size, window_size, vocabulary_size,
           result_callback, batched=False):
    """The front end that fits the callback: callbacks that want the pooled query vector (vectorspace) get a mapper,
    the others (loglinear: per-token distributions) the fixed-shape batcher (sert/inference.py:5-25)."""
    assert result_callback is not None
    if not result_callback.should_average_input():
        ids = np.min_scalar_type(vocabulary_size - 1)          # id width of the packed batches (inference.py:10)
        logging.info('Instance elements will be stored using %s.', ids)
        if batched and hasattr(result_callback, 'process_batch') and hasattr(predict_fn, 'rank_queries'):
            return BatchedWordRanker(predict_fn, batch_size, window_size, ids, result_callback)
        return WordBatcher(predict_fn, batch_size, window_size, ids, result_callback)
    mapper = BatchedEmbeddingMapper if batched and hasattr(result_callback, 'process_batch') else EmbeddingMapper
    return mapper(predict_fn, word_representations, result_callback)


class WordBatcher(object):
    """Queries in front of the loglinear predict_fn, which takes exactly (batch_size, window_size) ids + an int8 mask
    (models.py:830-856).  Same surface and same batches as the reference's batcher (sert/inference.py:28-143, pinned by
    tests/test_golden_host.py), built differently: ``submit`` only QUEUES a query and books its rows; the id batch and the
    mask are filled for all queued queries at once when the batch goes out -- a query of T tokens that starts at row r
    owns the flat slots [r n, r n + T) of the row-major batch (that is what "long queries spill over several rows" means,
    inference.py:115-117, 132-143), so packing is one scatter of the concatenated tokens and a query's per-token
    distributions are one contiguous slice of the flattened result (inference.py:89-94)."""

    OVERFLOW, TRUNCATE = range(5, 7)

    def __init__(self, predict_fn, batch_size, window_size, instance_dtype, result_callback=None, overflow_mode=OVERFLOW):
        assert overflow_mode in (WordBatcher.OVERFLOW, WordBatcher.TRUNCATE)
        assert result_callback is None or callable(result_callback)
        self.predict_fn, self.callback = predict_fn, result_callback
        self.batch_size, self.window_size, self.overflow_mode = batch_size, window_size, overflow_mode
        self.batch = np.zeros((batch_size, window_size), dtype=instance_dtype)     # (padding slots carry token id 0)
        self.mask = np.zeros((batch_size, window_size), dtype=np.int8)
        self._queue = []            # (first row, tokens, kwargs) of the queries waiting for the next predict_fn call
        self._rows = 0              # rows booked by them

    @property
    def num_used_instances(self):
        return self._rows

    def submit(self, query_tokens, **kwargs):
        assert len(query_tokens) > 0
        if self.overflow_mode == WordBatcher.TRUNCATE and len(query_tokens) > self.window_size:
            logging.error('Truncated query "%s" as it exceeded the window size.', query_tokens)
            query_tokens = query_tokens[:self.window_size]
        rows = -(-len(query_tokens) // self.window_size)
        if rows > self.batch_size:
            raise RuntimeError()        # (more tokens than one batch holds: inference.py:124-125)
        if self._rows + rows > self.batch_size:
            self.process()              # (no room left: the batch goes out first, inference.py:126-128)
        self._queue.append((self._rows, query_tokens, kwargs))
        self._rows += rows

    def _pack(self):
        """Fill batch / mask from the queue: one scatter into the flattened arrays."""
        lengths = np.fromiter((len(q) for _, q, _ in self._queue), dtype=np.int64, count=len(self._queue))
        starts = np.fromiter((r for r, _, _ in self._queue), dtype=np.int64, count=len(self._queue)) * self.window_size
        ends = np.cumsum(lengths)
        # flat slot of every queued token: its query's first slot + its position in the query
        slots = np.repeat(starts - (ends - lengths), lengths) + np.arange(int(ends[-1]))
        self.batch.fill(0)
        self.mask.fill(0)
        self.batch.reshape(-1)[slots] = np.concatenate([np.asarray(q) for _, q, _ in self._queue])
        self.mask.reshape(-1)[slots] = 1
        return starts, lengths

    def process(self):
        if not self._queue:
            return
        logging.debug('Processing batch (batch size=%d, current batch=%d).', self.batch_size, self._rows)
        starts, lengths = self._pack()
        out = self.predict_fn(self.batch, self.mask)            # (B, n, V_e)
        per_token = out.reshape((-1, out.shape[-1]))
        for (_, payload, kwargs), s0, T in zip(self._queue, starts, lengths):
            self.callback(payload, per_token[s0:s0 + T], **kwargs)
        self._queue, self._rows = [], 0


class QueryRanking(object):
    """What ``rank_queries`` returns for Q queries (sert_ll_rank_queries): ``idx`` / ``score`` (Q, kk) best first,
    ``joint_entropy`` (Q,), ``token_entropy[q]`` the per-token entropies of query q, ``status`` (Q,) (``HOST``: the
    joint's sum is 0 or not finite, the query must take the host path), ``k`` as asked.  ``distributions_of(q)``,
    set by the front end, returns the (T, V_e) per-token distributions of query q as the unbatched path computes them.

    ``candidates`` True (rank_queries(candidates=...), sert_ll_rank_candidates): ``idx[q]`` / ``score[q]`` are per-query
    arrays of differing length -- query q's candidate list ranked, its best min(k, length) -- and not rows of a matrix."""

    DEVICE, HOST = 0, 1

    def __init__(self, idx, score, joint_entropy, token_entropy, status, k=None, candidates=False):
        self.idx, self.score, self.joint_entropy = idx, score, joint_entropy
        self.token_entropy, self.status, self.k = token_entropy, status, k
        self.candidates = candidates
        self.distributions_of = None

    def __len__(self):
        return len(self.status)


class BatchedWordRanker(object):
    """All loglinear queries at once (additive): ``submit`` queues, ``process`` ranks every queued query with ONE
    ``predict_fn.rank_queries`` call -- of the callback's candidate lists, when it has some (``callback.candidate_lists``) --
    and hands the ranking to ``callback.process_batch``.  A query that the device
    cannot rank (status HOST) gets its distributions from a one-query WordBatcher of the same (batch_size, window_size)
    shape, so that predict_fn runs at the shape the unbatched path uses and the query's output is that path's."""

    def __init__(self, predict_fn, batch_size, window_size, instance_dtype, result_callback, k=None):
        assert hasattr(result_callback, 'process_batch') and hasattr(predict_fn, 'rank_queries')
        self.predict_fn, self.callback = predict_fn, result_callback
        self.batch_size, self.window_size, self.instance_dtype = batch_size, window_size, instance_dtype
        self.k = k
        self.pending = []

    def submit(self, query_tokens, **kwargs):
        assert len(query_tokens) > 0
        if -(-len(query_tokens) // self.window_size) > self.batch_size:
            raise RuntimeError()        # (as WordBatcher: more tokens than one batch holds, inference.py:124-125)
        self.pending.append((list(query_tokens), kwargs))

    def _distributions(self, tokens):
        got = []
        batcher = WordBatcher(self.predict_fn, self.batch_size, self.window_size, self.instance_dtype,
                              lambda payload, distribution: got.append(distribution))
        batcher.submit(tokens)
        batcher.process()
        return got[0]

    def process(self):
        if not self.pending:
            return
        payloads = [p for p, _ in self.pending]
        # a callback that re-ranks candidate lists (LogLinearCallback(candidates=...)) names the pending queries' lists: only
        # they are ranked and copied out
        lists = self.callback.candidate_lists([kw for _, kw in self.pending]) if hasattr(self.callback, 'candidate_lists') else None
        if lists is None:
            ranking = self.predict_fn.rank_queries(payloads, k=self.k)
        else:
            ranking = self.predict_fn.rank_queries(payloads, k=self.k, candidates=lists)
        ranking.distributions_of = lambda q: self._distributions(payloads[q])
        self.callback.process_batch(payloads, ranking, [kw for _, kw in self.pending])
        self.pending = []


class EmbeddingMapper(object):
    """One query at a time: mean word vector -> predict_fn -> callback."""

    def __init__(self, predict_fn, word_representations, result_callback):
        assert result_callback is None or callable(result_callback)
        self.predict_fn, self.callback = predict_fn, result_callback
        self.word_representations = word_representations

    def submit(self, query_tokens, **kwargs):
        # (sert/inference.py:161-167: the query is the mean of its words' rows)
        self.callback(query_tokens, self.predict_fn(self.word_representations[query_tokens, :].mean(axis=0)), **kwargs)

    def process(self):
        """Nothing is ever queued: submit() answers immediately."""


class BatchedEmbeddingMapper(object):
    """All queries at once (additive): ``submit`` queues, ``process`` projects
    every queued query with a single predict_fn call on the (Q, d_w) matrix of
    mean word vectors and hands the (Q, d_e) projections to
    ``callback.process_batch``."""

    def __init__(self, predict_fn, word_representations, result_callback):
        assert hasattr(result_callback, 'process_batch')
        self.predict_fn = predict_fn
        self.word_representations = word_representations
        self.callback = result_callback
        self.pending = []

    def submit(self, query_tokens, **kwargs):
        assert len(query_tokens) > 0
        self.pending.append((list(query_tokens), kwargs))

    def process(self):
        if not self.pending:
            return
        d = self.word_representations.shape[1]
        avg = np.empty((len(self.pending), d), dtype=np.float32)
        for i, (tokens, _) in enumerate(self.pending):
            avg[i] = self.word_representations[tokens, :].mean(axis=0)
        projections = self.predict_fn(avg)
        self.callback.process_batch(
            [p for p, _ in self.pending], projections,
            [kw for _, kw in self.pending])
        self.pending = []


def _product_skipping_zeros(distribution, axis):
    # multiplied in log space with log(0) counted as 0: a zero entry is skipped, it does not annihilate the product
    return np.exp(np.ma.log(distribution).filled(0).sum(axis=axis))


_AGGREGATORS = {
    'sum': lambda dist, axis: np.mean(dist, axis=axis),              # (sic: the reference's 'sum' is the mean)
    'product': _product_skipping_zeros,
    'last': lambda dist, axis: np.take(dist, indices=dist.shape[axis] - 1, axis=axis),
    'max': lambda dist, axis: np.max(dist, axis=axis),
    'identity': lambda dist, axis: dist,
}


def aggregate_distribution(distribution, mode, axis):
    """Per-token distributions -> one (sert/inference.py:170-183); unknown modes raise NotImplementedError."""
    try:
        fn = _AGGREGATORS[mode]
    except KeyError:
        raise NotImplementedError()
    return fn(distribution, axis)
