"""Operands for which a float32 GEMM has ONE right answer, known to the bit -- the inputs of the exact-product tests of
csrc/gemm_x3.h (tests/test_gpu_gemm.py on the device, tests/test_x3_split_cpu.py for the proof that they discriminate).

gemm_x3.h splits every operand into three bfloat16 pieces x = x0 + x1 + x2 and accumulates the six products a_p.b_q with
p + q <= 2.  Dense random operands under an absolute bound cannot tell that from a kernel that loses one of the small
products, or reads one plane of one operand from the wrong k on part of its K: such an error is a few 1e-6 at most.  The
four families here make it tens to thousands of units in the last place, or a wrong bit where none may differ:

  selection x full mantissa   every row of op(A) holds one non-zero, +-2^e at column k_i; B is dense, every element with all
                              three pieces non-zero.  C[i, j] = +-2^e B[k_i, j]: the products a0.b0, a0.b1, a0.b2 and nothing
                              else, every partial sum of them representable -> exact whatever the order.  Pins those three
                              products and from which k each plane of B is read.
  full mantissa x selection   the mirror image: a0.b0, a1.b0, a2.b0 and the planes of A.
  two-piece x two-piece       A a selection of hi + lo, B dense hi + lo (hi a bfloat16 in (1, 1.5), |lo| a bfloat16 in
                              [0.75, 1) 2^-8: x2 = 0, x1 = lo).  An output is ONE product of four exact partial products
                              a0.b0, a0.b1, a1.b0, a1.b1; three float32 additions of half an ulp each: within 4 ulp of the
                              exact product (room for an accumulator that truncates).  Without a1.b1 it is off by 2^-18
                              relative, 31 ulp or more.
  power-of-two scaling        dense U(-1, 1) operands as they are and with row i of op(A) times 2^r_i, column j of op(B)
                              times 2^c_j: a power of two commutes with every rounding while nothing underflows, so the
                              second product is the first times 2^(r_i + c_j) bit for bit.

Everything is built on LOGICAL operands op(A) (M, K) and op(B) (K, N); stored() lays one out the way a kernel form wants it.
"""
import numpy as np

E_RANGE = 30          # exponents of the selection values and of the scaling, [-30, 30]
ULP_BOUND = 4         # two-piece family: units in the last place of the exact product


def bf16_rne(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    x0 = bf16_rne(x)
    r1 = x - x0                      # exact in float32
    x1 = bf16_rne(r1)
    r2 = r1 - x1                     # exact in float32
    x2 = bf16_rne(r2)
    return x0, x1, x2


def rng_of(*key):
    return np.random.Generator(np.random.PCG64([int(k) & 0xffffffff for k in key]))


def stored(logical, transposed):
    """A logical operand as the contiguous array a kernel form reads: itself, or its transpose."""
    return np.ascontiguousarray(logical.T if transposed else logical)


def pow2(e):
    return np.ldexp(np.float32(1), np.asarray(e, dtype=np.int32)).astype(np.float32)


def selection(rng, lines, K, kper=None):
    """One (k, value) per line -- a row of op(A) or a column of op(B): value = +-2^e, e in [-E_RANGE, E_RANGE].  The k cover
    every index when there are lines enough; otherwise they are distinct and hold, first of all, the last 32 indices (every
    index of a ragged last 16-step and of the last group of four, and the full step before them), the first 16, and the
    two indices either side of every k-range boundary (kper: the length of a range of the split forms)."""
    if lines >= K:
        k = rng.permutation(lines) % K
    else:
        must = list(range(K - 1, max(K - 33, -1), -1)) + list(range(min(16, K)))
        if kper:
            for z in range(kper, K, kper):
                must += [z - 1, z]
        must = list(dict.fromkeys(must))[:lines]
        rest = np.setdiff1d(np.arange(K), must)
        k = np.concatenate([np.array(must, dtype=np.int64), rng.choice(rest, lines - len(must), replace=False)])
        k = rng.permutation(k)
    e = rng.integers(-E_RANGE, E_RANGE + 1, lines)
    sign = np.where(rng.integers(0, 2, lines) == 1, np.float32(-1), np.float32(1))
    return k.astype(np.int64), (sign * pow2(e)).astype(np.float32)


def place_rows(k, v, K):
    """op(A) (len(k), K) with v[i] at [i, k[i]]."""
    a = np.zeros((len(k), K), dtype=np.float32)
    a[np.arange(len(k)), k] = v
    return a


def place_cols(k, v, K):
    """op(B) (K, len(k)) with v[j] at [k[j], j]."""
    b = np.zeros((K, len(k)), dtype=np.float32)
    b[k, np.arange(len(k))] = v
    return b


def full_mantissa(rng, shape, k_axis, distinct=None):
    """Dense float32 with magnitudes in [0.5, 2), random signs, the lowest mantissa bit set (so x2 != 0) and all three
    pieces non-zero.  One binade per line along k (a column of op(B), a row of op(A)), so that all pieces of a line are
    multiples of one ulp: a piece taken from another k of the line moves the sum by a whole number of ulps, never by a
    tie that rounds back.  And every piece differs from the same piece at k - 1 and k + 1 (cyclically): no misrouted plane
    can go unnoticed anywhere.  (distinct: redraw until all that holds -- by default up to 2^21 elements; a larger operand
    takes its draw as it comes, with x2 != 0 everywhere and a piece in 250 or so equal to its neighbour or zero.)"""
    if distinct is None:
        distinct = int(np.prod(shape)) <= 1 << 21
    line_shape = [1 if a == k_axis else n for a, n in enumerate(shape)]
    expo = (126 + rng.integers(0, 2, line_shape)).astype(np.uint32)              # [0.5, 1) or [1, 2)
    sign = rng.integers(0, 2, shape).astype(np.uint32) << 31
    mant = (rng.integers(0, 1 << 22, shape).astype(np.uint32) << 1) | 1
    for _ in range(64):
        x = (sign | (expo << 23) | mant).view(np.float32)
        if not distinct:
            return x
        pieces = split3(x)
        bad = np.zeros(shape, dtype=bool)
        for p in pieces:
            bad |= p == 0
            if shape[k_axis] > 1:
                same = p == np.roll(p, 1, axis=k_axis)
                bad |= same | np.roll(same, -1, axis=k_axis)
        if not bad.any():
            return x
        n = int(bad.sum())
        mant[bad] = (rng.integers(0, 1 << 22, n).astype(np.uint32) << 1) | 1
    raise AssertionError('no full-mantissa draw with distinct neighbouring pieces')


def two_piece(rng, shape):
    """hi + lo: hi = 1 + j / 128, j in 1 .. 63 (a bfloat16 in (1, 1.5)), lo = +-m 2^-16, m in 192 .. 255 (a bfloat16,
    [0.75, 1) 2^-8 in magnitude), a random sign on the whole: x0 = hi, x1 = lo, x2 = 0."""
    hi = 1.0 + rng.integers(1, 64, shape) / 128.0
    lo = rng.integers(192, 256, shape) * 2.0 ** -16 * np.where(rng.integers(0, 2, shape) == 1, -1.0, 1.0)
    sign = np.where(rng.integers(0, 2, shape) == 1, -1.0, 1.0)
    x = (sign * (hi + lo)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), sign * (hi + lo))
    return x


def ulp_of(exact):
    """The float32 unit in the last place at the magnitude of a (float64) value."""
    return np.ldexp(1.0, np.floor(np.log2(np.abs(exact))).astype(np.int64) - 23)


def smallest_piece_is_normal(x):
    """No bfloat16 piece of x is subnormal: a non-zero piece is at least one float32 ulp of x, 2^-23 of its binade."""
    nz = np.abs(x[x != 0])
    return nz.size == 0 or float(nz.min()) >= 2.0 ** (-126 + 23)


# --------------------------------------------------------------------------- #
# the four families: logical operands and what the product must be
# --------------------------------------------------------------------------- #
def selection_a(M, N, K, seed, kper=None):
    """(op(A), op(B), expected): selection x full mantissa.  expected by indexing, exact."""
    rng = rng_of(1, M, N, K, seed)
    k, v = selection(rng, M, K, kper)
    B = full_mantissa(rng, (K, N), 0)
    return place_rows(k, v, K), B, v[:, None] * B[k, :]


def selection_b(M, N, K, seed, kper=None):
    """(op(A), op(B), expected): full mantissa x selection."""
    rng = rng_of(2, M, N, K, seed)
    k, v = selection(rng, N, K, kper)
    A = full_mantissa(rng, (M, K), 1)
    return A, place_cols(k, v, K), A[:, k] * v[None, :]


def two_piece_pair(M, N, K, seed, kper=None):
    """(op(A), op(B), exact): A a selection of two-piece values, B dense two-piece; exact = the products in float64
    (17 x 17 significant bits: exact there)."""
    rng = rng_of(3, M, N, K, seed)
    k, _ = selection(rng, M, K, kper)
    v = two_piece(rng, M)
    B = two_piece(rng, (K, N))
    return place_rows(k, v, K), B, v.astype(np.float64)[:, None] * B[k, :].astype(np.float64)


def scaled_pair(M, N, K, seed):
    """(op(A), op(B), r, c): dense U(-1, 1) operands (B times 1 / sqrt(K), as the float64 tests have them) and the exponents
    of the row scaling of op(A) and the column scaling of op(B)."""
    rng = rng_of(4, M, N, K, seed)
    A = rng.random((M, K), dtype=np.float32) * np.float32(2) - np.float32(1)
    B = (rng.random((K, N), dtype=np.float32) * np.float32(2) - np.float32(1)) * np.float32(1.0 / np.sqrt(K))
    return A, B, rng.integers(-E_RANGE, E_RANGE + 1, M), rng.integers(-E_RANGE, E_RANGE + 1, N)


def scale_rows(x, e):
    return (x * pow2(e)[:, None]).astype(np.float32)


def scale_cols(x, e):
    return (x * pow2(e)[None, :]).astype(np.float32)


# --------------------------------------------------------------------------- #
# the shapes of the device tests: the smallest that reach every kernel form (asserted: tests/test_x3_split_cpu.py)
# --------------------------------------------------------------------------- #
# sert_debug_gemm, tb = 0 and 1.  gemm_x3.h takes a product with 128 row tiles (M >= 16384 at N <= 128 in 128-row tiles,
# M >= 32768 above in 256-row tiles: x3_big_size) or, from K = 256 and M = 1024 on, with 160 tiles of 128 x 128 -- 96 when a
# leading dimension or K is no multiple of four (x3_mid_size).  K = 36: two steps of 16 and a ragged one of a single group of
# four; 263 and 300: a ragged last step of 7 and of 12.
PLAIN_X3 = [
    ((16384 + 7, 128, 36), 'x3_128_vec'),       # 128 x 128 tiles, one column tile, ragged last row tile
    ((16400, 31, 16), 'x3_128_vec'),            # ... a single step, a quarter of a column tile
    ((32768 + 9, 200, 36), 'x3_256'),           # 256-column tiles
    ((32768 + 9, 300, 36), 'x3_320'),           # 320-column tiles (the last 20 columns of the tile beyond N)
    ((2050, 715, 263), 'x3_128_scalar'),        # mid-size, nothing a multiple of four: dword loaders
    ((3500, 716, 300), 'x3_128_vec'),           # mid-size, aligned
]
# the fp32 MFMA kernels of gemm.h (what SERT_GEMM_FP32=1 falls back to): the same expectations hold for a true float32
# product.  (M, N) of TANH_SHAPES with K = 8, and 172 x 3 = 516 tiles of 128 x 128 at N = 300 for the 128 x 160-tile kernel.
PLAIN_F32 = [
    ((4096, 4096, 8), 'f32_tile128'),
    ((1000, 300, 8), 'f32_tile64'),
    ((22000, 300, 8), 'f32_tile128x160'),
]
# sert_debug_gemm_splitk (M, N, K, splits): A^T.B over K >= 4096 with 16 tiles x k ranges or more (x3_shape_ok)
SPLITK = [
    ((128, 128, 4096 + 24, 16), 'x3_ta_single'),     # ranges of 272, the last one 40: two steps and a half
    ((300, 161, 4096 + 16, 16), 'x3_ta_320x160'),    # two column tiles, the second one column wide
    ((400, 130, 4096, 8), 'x3_ta_tiles'),            # 4 x 2 tiles of 128 x 128
]
# sert_debug_gemm_longk (M, N, K, splits, tb): A.op(B) in k ranges
LONGK = [
    ((1100, 128, 8192 + 8, 128, 1), 'x3_128_vec'),   # 103 ranges of 80, the last one 40 (64 slabs or more: the sixteen-group combine)
    ((3500, 300, 715, 5, 1), 'x3_128_scalar'),       # ranges of 144, the last one 139
    ((3500, 300, 715, 5, 0), 'x3_128_scalar'),
]


def k_range(K, splits):
    """The length of a k range of the split forms (whole steps of 16), as sert_debug_gemm_splitk / _longk cut K."""
    per = -(-K // splits)
    return -(-per // 16) * 16
