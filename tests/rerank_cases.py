"""Inputs and expectations shared by tests/test_rerank_inputs_cpu.py and tests/test_gpu_rerank.py: per-query candidate lists for
the re-ranking calls of the cosine scorer (include/sert_hip.h: sert_scorer_pairs, sert_scorer_rank_candidates).  Pure NumPy;
every draw has a fixed seed and every builder is cached, so the two test files see the same arrays."""
import functools

import numpy as np

from oracle import sert_oracle as O
from tests import util as U

LDS_MAX = 8192                                   # csrc/kernels_rank.h kRankLdsMax: longer lists take the slab path
EXACT_NAMES = ('tiny', 'mid', 'unaligned_rows', 'fused_smallest')
FORM_V, FORM_LENGTHS = 9000, (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 9000)
PREFILTER_V, PREFILTER_LENGTHS = 40000, (100, 9000, 40000)
WIDTHS = (4, 18, 128, 300)
K_LENGTHS = (0, 1, 3, 40, 1500, 2000, 8500, 0, 5)
K_VALUES = (1, 5, 1500, 20000)

# two chunks of several queries each: the second starts at query 4, behind non-zero candidate and output offsets, and holds two
# slab rows of unequal length (a padded slab), lists in two LDS classes and an empty list
CHUNK_LENGTHS = (8200, 300, 8300, 5, 8250, 1100, 0, 8193, 2000)
CHUNK_BOUNDS = [0, 4, 9]
CHUNK_BUDGETS = {None: 1000000, 7: 600000}       # k -> SERT_SCORE_RANK_BUDGET under which the planner cuts at CHUNK_BOUNDS
SORT_MAX_BINS, SORT_TILE = 2048, 2048            # csrc/kernels_sort.h kSortMaxBins, kSortTile


def ladder(V):
    """The list lengths of an exact problem over V entities."""
    return (1, 2, 3, 33, 257, V // 2, V)


def draw_list(rng, V, length):
    """`length` distinct entities of V, ascending, int32."""
    return np.sort(rng.choice(V, size=length, replace=False)).astype(np.int32)


def expected_ranking(cos, entities, k=None):
    """The contract for one list: `cos` the float32 cosines of `entities` (ascending).  -> (entities int32 in ranking order,
    float32 scores (cos + 1) / 2), the best min(k, len)."""
    cos = np.ascontiguousarray(cos, dtype=np.float32)
    order = O.rank_order(cos, k)
    with np.errstate(invalid='ignore'):
        val = (cos[order] + np.float32(1)) / np.float32(2)
    return np.asarray(entities, dtype=np.int32)[order], val.astype(np.float32)


def split(out_indptr, idx, val):
    """The ragged result of Scorer.rank_candidates as a list of (idx, val) per query."""
    return [(idx[a:b], val[a:b]) for a, b in zip(out_indptr[:-1], out_indptr[1:])]


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """An exact problem of tests/util.py with one list per query: the lengths of ladder(V) cycling over the queries (at least
    one round: the queries repeat where the problem has fewer than seven), then one empty list.  dict: E, P (queries, d),
    lists, c16 (per query the integer 16 cos of its list), want (per query the contract's (entities, scores))."""
    p = U.exact_score_problem(name)
    V, Q = p['E'].shape[0], p['P'].shape[0]
    rng = np.random.RandomState(9000 + U.EXACT_SHAPES[name][0])
    steps = ladder(V)
    nq = max(Q, len(steps)) + 1
    rows = np.arange(nq) % Q
    lengths = [min(steps[i % len(steps)], V) for i in range(nq - 1)] + [0]        # ('tiny' has fewer than 257 entities: all of them)
    lists = [draw_list(rng, V, n) for n in lengths]
    c16 = U.exact_cos16(p['Pi'][rows], p['Ei'])
    per_list = [c16[q, lst.astype(np.int64)] for q, lst in enumerate(lists)]
    want = []
    for lst, c in zip(lists, per_list):
        idx, val = U.exact_expected(c[None, :])
        want.append((lst[idx[0].astype(np.int64)], val[0]))
    return dict(E=p['E'], P=p['P'][rows], lists=lists, lengths=lengths, c16=per_list, want=want)


@functools.lru_cache(maxsize=None)
def form_case():
    """Every LDS size of the list kernel, filled and one over, and the slab path from its smallest list: (E, P, lists)."""
    E, P = U.gaussian_score_problem(FORM_V, 16, len(FORM_LENGTHS), seed=43)
    rng = np.random.RandomState(4301)
    return E, P, [draw_list(rng, FORM_V, n) for n in FORM_LENGTHS]


@functools.lru_cache(maxsize=None)
def chunk_case():
    """Lists of CHUNK_LENGTHS over a table of FORM_V entities: (E, P, lists)."""
    E, P = U.gaussian_score_problem(FORM_V, 16, len(CHUNK_LENGTHS), seed=59)
    rng = np.random.RandomState(5901)
    return E, P, [draw_list(rng, FORM_V, n) for n in CHUNK_LENGTHS]


def plan_chunks(lengths, k, budget):
    """sert_scorer_rank_candidates' planner restated (host/api_scorer_rerank.inc, ListShape::bytes of host/rank_lists.inc): the
    query bounds of its chunks.  A chunk takes the next query while its footprint stays within `budget` bytes -- 4 a candidate,
    8 a ranked entry and, for its lists beyond LDS_MAX, the (rows, lmax) slab, the sort scratch over it (16 bytes an element
    and the histograms) and the (rows, min(k, lmax)) positions and scores -- and its slab fits one sorted chunk; its first
    query always."""
    def footprint(pairs, outs, rows, lmax):
        b = pairs * 4 + outs * 8
        if rows:
            n = rows * lmax
            b += n * 4 + n * 16 + (SORT_MAX_BINS * -(-n // SORT_TILE) + SORT_MAX_BINS) * 4 + rows * (lmax if k is None else min(k, lmax)) * 8
        return b

    bounds, q = [0], 0
    while q < len(lengths):
        pairs = outs = rows = lmax = 0
        q0 = q
        while q < len(lengths):
            n = lengths[q]
            t = (pairs + n, outs + (n if k is None else min(k, n)), rows + (n > LDS_MAX), max(lmax, n) if n > LDS_MAX else lmax)
            fits = not t[2] or (t[2] <= SORT_MAX_BINS and t[2] * t[3] <= 2 ** 31 - 2 ** 20)
            if q > q0 and (not fits or footprint(*t) > budget):
                break
            pairs, outs, rows, lmax = t
            q += 1
        bounds.append(q)
    return bounds


@functools.lru_cache(maxsize=None)
def prefilter_case():
    """A bf16-prefiltered table (V >= 32768): (E, P, lists), the lengths of PREFILTER_LENGTHS cycling over 8 queries."""
    E, P = U.gaussian_score_problem(PREFILTER_V, 16, 8, seed=47)
    rng = np.random.RandomState(4701)
    return E, P, [draw_list(rng, PREFILTER_V, PREFILTER_LENGTHS[q % 3]) for q in range(8)]


@functools.lru_cache(maxsize=None)
def width_case(d):
    """V = 500, Q = 4, lists of 200 at row width d: (E, P, lists, per list the float64 cosines of the float32 inputs)."""
    E, P = U.gaussian_score_problem(500, d, 4, seed=50 + d)
    rng = np.random.RandomState(5100 + d)
    lists = [draw_list(rng, 500, 200) for _ in range(4)]
    E64, P64 = E.astype(np.float64), P.astype(np.float64)
    En = E64 / np.linalg.norm(E64, axis=1)[:, None]
    Pn = P64 / np.linalg.norm(P64, axis=1)[:, None]
    return E, P, lists, [En[lst.astype(np.int64)] @ Pn[q] for q, lst in enumerate(lists)]


def width_bound(d):
    """|device cosine - float64 cosine| for unit rows of width d: two normalisations of at most d/128 + 6 roundings each, a
    per-lane fmaf chain of at most d/32 terms and 5 tree adds on products whose absolute sum is at most 1 -- below
    (2 d + 8) 2^-24 for every d >= 4."""
    return (2 * d + 8) * 2.0 ** -24


ZERO_ROWS = lambda V: (3, V // 2, V - 1)          # noqa: E731
NAN_QUERIES = (1, 3)


@functools.lru_cache(maxsize=None)
def special_case(V):
    """Three all-zero entity rows, query 1 all zero and query 3 with a NaN; five lists that contain the zero rows: 200 drawn
    entities and the three (V = 1100: the LDS kernel) or every entity (V = 8300: the slab path).  (E, P, lists)."""
    E, P = U.gaussian_score_problem(V, 16, 5, seed=7)
    E[list(ZERO_ROWS(V))] = 0
    P[1] = 0
    P[3, 2] = np.nan
    rng = np.random.RandomState(700 + V)
    if V > LDS_MAX:
        lists = [np.arange(V, dtype=np.int32) for _ in range(5)]
    else:
        lists = [np.union1d(draw_list(rng, V, 200), np.array(ZERO_ROWS(V))).astype(np.int32) for _ in range(5)]
    return E, P, lists


def special_expected(E, P, lists):
    """The contract on the float32 cosines numpy computes for special_case (0 / 0 and NaN rows: NaN)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = U.oracle_cosines_f32(E, P)
    return [expected_ranking(cos[q, lst.astype(np.int64)], lst) for q, lst in enumerate(lists)]


@functools.lru_cache(maxsize=None)
def k_case():
    """Mixed lengths, two of them empty, over the table of form_case: (E, P, lists)."""
    E, P, _ = form_case()
    rng = np.random.RandomState(4401)
    return E, P, [draw_list(rng, FORM_V, n) for n in K_LENGTHS]
