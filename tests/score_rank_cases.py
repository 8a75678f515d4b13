"""Inputs shared by tests/test_score_rank_cpu.py and tests/test_gpu_score_rank.py: cosine rows no dot product of the library
returns (both zeros, NaNs of both signs, infinities, denormals, duplicates), for the ranking kernels of sert_scorer_rank
themselves (sert_debug_scorer_rank_select), and the chunk footprint of that call restated."""
import numpy as np

from oracle import sert_oracle as O

SPECIAL_V = (300, 8200)       # the LDS sort, the counting-sort passes (include/sert_hip_debug.h: the path goes by V)
SPECIAL_Q = 4

# csrc/kernels_sort.h: bins of a digit pass, keys per workgroup
SORT_MAX_BINS, SORT_TILE = 2048, 2048
PATH_TOPK, PATH_LDS, PATH_CSORT = 'topk', 'lds', 'csort'


def special_rows(V):
    """(4, V) float32.  Row 0: Gaussian values with +0 and -0 interleaved, +NaN and -NaN, +inf, -inf, denormals and duplicated
    values strewn in; row 1: all NaN, of both signs; row 2: nothing but the two zeros and a few numbers around them; row 3: a
    handful of distinct values, each hundreds of times, with infinities and NaNs."""
    rng = np.random.RandomState(500 + V)
    neg_nan = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]
    pos_nan = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
    den = np.float32(1e-41)
    rows = np.empty((SPECIAL_Q, V), dtype=np.float32)
    r = (0.3 * rng.randn(V)).astype(np.float32)
    r[3::7] = np.float32(0.0)
    r[5::14] = np.float32(-0.0)
    r[11::41] = pos_nan
    r[13::43] = neg_nan
    r[17::97] = np.inf
    r[19::101] = -np.inf
    r[23::53] = den
    r[29::59] = -den
    r[31::37] = r[2]                     # duplicates of one ordinary value
    r[1] = np.float32(0.25)              # two cosines with one emitted score: 0.25 + 2^-25 rounds away in (c + 1) / 2
    r[V - 1] = np.nextafter(np.float32(0.25), np.float32(1))
    rows[0] = r
    rows[1] = np.where(np.arange(V) % 3 == 0, neg_nan, pos_nan)
    z = np.where(rng.rand(V) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    z[::50] = (1e-3 * rng.randn(len(z[::50]))).astype(np.float32)
    rows[2] = z
    levels = np.array([-1.0, -0.25, -0.0, 0.0, 0.25, 1.0, np.inf, -np.inf, pos_nan, neg_nan], dtype=np.float32)
    rows[3] = levels[rng.randint(0, len(levels), size=V)]
    return rows


def expected(cos, k=None):
    """The contract's (idx int32, val float32) for float32 cosines (Q, V): rank_order per row, (cos + 1) / 2 afterwards."""
    cos = np.ascontiguousarray(cos, dtype=np.float32)
    keep = cos.shape[1] if k is None else min(k, cos.shape[1])
    idx = np.stack([O.rank_order(row, keep) for row in cos])
    with np.errstate(invalid='ignore'):
        val = (np.take_along_axis(cos, idx, axis=1) + np.float32(1)) / np.float32(2)
    return idx.astype(np.int32), val.astype(np.float32)


def rank_path(V, k):
    """The path sert_scorer_rank takes (include/sert_hip.h), and the ranked depth."""
    kk = V if k is None or k >= V else k
    return (PATH_TOPK if kk <= 1024 else PATH_LDS if V <= 8192 else PATH_CSORT), kk


def chunk_bytes(V, k, queries):
    """Device footprint of a chunk of `queries` queries (csrc/host/api_scorer_rank.inc: score_rank_bytes): the slab, two
    (Qc, kk) result sets, and for the counting-sort passes four key / value arrays, the histogram and the bin totals."""
    path, kk = rank_path(V, k)
    b = queries * V * 4 + queries * kk * 16
    if path == PATH_CSORT:
        n = queries * V
        b += n * 16 + (SORT_MAX_BINS * ((n + SORT_TILE - 1) // SORT_TILE) + SORT_MAX_BINS) * 4
    return b
