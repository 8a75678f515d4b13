"""Inputs and the expectation shared by tests/test_ll_rerank_inputs_cpu.py and tests/test_gpu_ll_rerank.py: per-query candidate
lists for the loglinear re-ranker (include/sert_hip.h: sert_ll_rank_candidates).  Pure NumPy; every draw has a fixed seed and
every builder is cached, so the two test files see the same arrays.

The expectation is one function, filter_full_ranking: the contract says a DEVICE query's result is the full ranking
(sert_ll_rank_queries, k = -1) restricted to its list and cut to its head, so the expected arrays are made from the full
ranking's own arrays -- same order, same score bits."""
import functools

import numpy as np

LDS_MAX = 8192                                   # csrc/kernels_rank.h kRankLdsMax: longer lists take the slab path
K_VALUES = (None, 1, 10, 5000)
GOLDEN_K = (None, 1, 10, 40)
TIE_LEVELS = np.array([1.0, 2.0, 3.0, 5.0, 8.0], np.float32)     # (tests/test_gpu_ll_rank.py TIE_LEVELS)
# every LDS class on both sides of its edge, one list past LDS, the whole table
TIED_LENGTHS = {300: (1, 2, 150, 300), 8200: (0, 1, 2, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 8200)}


def draw_list(rng, V, length):
    """`length` distinct entities of V, ascending, int32."""
    return np.sort(rng.choice(V, size=length, replace=False)).astype(np.int32)


def filter_full_ranking(idx_full, score_full, lists, k=None):
    """The contract: per query (idx, score) = the full ranking's entries whose entity is in the query's list, in the full
    ranking's order, the first min(k, len) of them (k None: all).  idx_full / score_full: (Q, V_e) or per-query arrays."""
    out = []
    for q, lst in enumerate(lists):
        idx, score = np.asarray(idx_full[q]), np.asarray(score_full[q])
        keep = np.isin(idx, np.asarray(lst, dtype=np.int64))
        idx, score = idx[keep], score[keep]
        if k is not None:
            idx, score = idx[:k], score[:k]
        out.append((idx, score))
    return out


def split(out_indptr, idx, score):
    """The ragged result of a candidate call as a list of (idx, score) per query."""
    return [(idx[a:b], score[a:b]) for a, b in zip(out_indptr[:-1], out_indptr[1:])]


def golden_lists(V):
    """All entities, one entity, every other entity, none."""
    return [np.arange(V, dtype=np.int32), np.array([V // 3], dtype=np.int32), np.arange(0, V, 2, dtype=np.int32),
            np.zeros(0, dtype=np.int32)]


def tied_distributions(V, offsets):
    """(offsets[-1], V) token rows as _tied_distributions of tests/test_gpu_ll_rank.py makes them: every entry one of five
    positive levels, each row normalised in float32 -- entities that drew the same levels in a query's tokens go through the
    same float32 operations and share one joint value, bit for bit."""
    rng = np.random.RandomState(V)
    P = TIE_LEVELS[rng.randint(0, TIE_LEVELS.size, (offsets[-1], V))]
    return P / P.sum(axis=1, dtype=np.float32, keepdims=True)


@functools.lru_cache(maxsize=None)
def tied_case(V):
    """One query per length of TIED_LENGTHS[V], of one and two tokens in turn: (P, offsets, lists)."""
    lengths = TIED_LENGTHS[V]
    offsets = np.concatenate([[0], np.cumsum([1 + q % 2 for q in range(len(lengths))])]).astype(np.int64)
    rng = np.random.RandomState(7000 + V)
    return tied_distributions(V, offsets), offsets, [draw_list(rng, V, n) for n in lengths]


def log_joint64(dist):
    """L_e = sum_t log p_te with log 0 -> 0, float64 (tests/test_gpu_ll_rank.py host_log_joint)."""
    d = np.asarray(dist, dtype=np.float64)
    return np.where(d > 0, np.log(np.where(d > 0, d, 1.0)), 0.0).sum(axis=0)


def in_tie_runs(values):
    """How many elements of `values` share their value with another one."""
    _, counts = np.unique(values, return_counts=True)
    return int(counts[counts >= 2].sum())


def reversed_queries(P, offsets, lists):
    """The same queries, last first: (P, offsets, lists)."""
    Q = len(lists)
    rows = np.concatenate([np.arange(offsets[q], offsets[q + 1]) for q in reversed(range(Q))])
    offs = np.concatenate([[0], np.cumsum([offsets[q + 1] - offsets[q] for q in reversed(range(Q))])]).astype(np.int64)
    return P[rows], offs, lists[::-1]


@functools.lru_cache(maxsize=None)
def engine_case(name):
    """Weights, queries and lists of an engine problem: dict Rw, W, b, queries, lists.
      'small'  V_w = 2000, V_e = 715, d = 64, 50 queries of 1-6 tokens, lists of 0-715 entries (the first empty, the second
               the whole table, one handed over unsorted and with duplicates: the wrapper cleans it);
      'slab'   V_e = 9000, d = 32, 12 queries, one list above 8192 entries."""
    Vw, Ve, d, Q = {'small': (2000, 715, 64, 50), 'slab': (500, 9000, 32, 12)}[name]
    rng = np.random.RandomState(100 + Ve)
    Rw = rng.uniform(-0.5, 0.5, (Vw, d)).astype(np.float32)
    W = (rng.standard_normal((d, Ve)) * 0.25).astype(np.float32)
    queries = [list(rng.randint(0, Vw, rng.randint(1, 7))) for _ in range(Q)]
    if name == 'small':
        lengths = [0, Ve] + [int(n) for n in rng.randint(0, Ve + 1, Q - 2)]
        lengths[5] = 200
    else:
        lengths = [8500, 0, 1, 700, 1024, 1025, 3000, 4097, 8192, 9, 2048, 5000]
    lists = [draw_list(rng, Ve, n) for n in lengths]
    if name == 'small':
        lists[5] = np.concatenate([lists[5][::-1], lists[5][:3]])
    return dict(Rw=Rw, W=W, b=np.zeros(Ve, np.float32), queries=queries, lists=lists)


@functools.lru_cache(maxsize=None)
def host_case():
    """The construction of tests/test_gpu_ll_rank.py::test_host_status_query_takes_the_unbatched_path_bit_for_bit: near-flat
    logits over V_e = 4096 and a query of 60 tokens, whose joint underflows everywhere (S = 0), between two ordinary ones."""
    rng = np.random.RandomState(3)
    Vw, Ve, d = 300, 4096, 64
    Rw = rng.uniform(-0.5, 0.5, (Vw, d)).astype(np.float32)
    W = (rng.standard_normal((d, Ve)) * 1e-3).astype(np.float32)
    queries = [list(rng.randint(0, Vw, 3)), list(rng.randint(0, Vw, 60)), list(rng.randint(0, Vw, 2))]
    lists = [draw_list(rng, Ve, n) for n in (500, 40, 4096)]
    return dict(Rw=Rw, W=W, b=np.zeros(Ve, np.float32), queries=queries, lists=lists, window=8, batch=16)
