"""Every GEMM kernel of the library against float64, through sert_debug_gemm -- the same dispatch (launch_gemm) a training
step uses, so a shape lands on the kernel the step would run it on: the bf16-pipe kernel with exactly split operands
(gemm_x3.h: 128 row tiles or more -- M >= 16384 for N <= 128, M >= 32768 above --, A not transposed, or A^T.B over K >= 4096; SERT_GEMM_FP32=1 sends those shapes to the fp32 MFMA kernels too), the
128x128-tile kernel, the 64x64-tile one, the 128x160-tile one (N just above a multiple of 128) and -- against a variants build (SERT_LIB=.../libsert_variants.so) with
SERT_GEMM_DIRECT_MIN_K=256 / SERT_GEMM_STREAM=1 -- the two kernels of round 4 that feed A straight from global memory into
v_mfma_f32_16x16x4_f32 (variants/gemm_direct.h, variants/gemm_stream.h; measured equal or slower, not in the product).
The float64 bounds price the fp32 accumulation; that gemm_x3.h forms each of its six piece products, every plane from its own
k, is pinned further down by operands whose product is known to the bit (tests/x3_families.py)."""
import numpy as np
import pytest

from tests import x3_families as F
from tests.util import C

pytestmark = pytest.mark.gpu


def _ref(A, B, ta, tb, epi, bias):
    a = A.astype(np.float64).T if ta else A.astype(np.float64)
    b = B.astype(np.float64).T if tb else B.astype(np.float64)
    c = a @ b
    if epi:
        c = c + bias.astype(np.float64)
    if epi == 2:
        c = np.tanh(c)
    return c


@pytest.mark.parametrize('M,N,K,ta,tb,epi', [
    # the streaming projection kernel: h.W + b -> tanh, da.W^T; ragged last strip, fewer strips than waves x 2, many
    (65536, 128, 128, 0, 0, 2), (65536, 128, 128, 0, 1, 0), (8192 + 5, 128, 128, 0, 0, 2), (8192 + 5, 128, 128, 0, 1, 0),
    (20000, 128, 128, 0, 0, 1), (20000, 128, 128, 0, 1, 1), (16384, 128, 128, 0, 0, 0),
    # just outside its shape conditions: the tiled kernels
    (8191, 128, 128, 0, 0, 2), (65536, 128, 112, 0, 0, 2), (4099, 128, 128, 0, 1, 0), (30000, 112, 128, 0, 1, 0),
    # 64x64 tiles, 128x128 tiles, 128x160 tiles, odd sizes (scalar loaders), A^T.B
    (1000, 300, 300, 0, 0, 2), (4096, 1000, 128, 0, 0, 1), (3000, 128, 1000, 0, 1, 0), (333, 77, 45, 0, 0, 1),
    (128, 128, 5000, 1, 0, 0), (300, 301, 2000, 1, 0, 0), (257, 129, 64, 1, 1, 0),
    # long-K shapes (variants build + SERT_GEMM_DIRECT_MIN_K=256: gemm_direct.h): 256-row and 128-row tiles, both B layouts, ragged M, N
    # (last column tile 104 / 44 wide), K with a partial last slab and a partial last 16-k block (1000 = 15 x 64 + 40)
    (65536, 128, 1000, 0, 0, 0), (65536, 128, 1000, 0, 1, 0), (20000, 1000, 256, 0, 1, 1), (44467, 128, 1000, 0, 1, 0),
    (9000, 300, 300, 0, 0, 2), (9001, 300, 300, 0, 1, 0), (4096, 1000, 260, 0, 0, 1), (2049, 256, 4096, 0, 0, 0),
    (4096, 4096, 512, 0, 1, 0),
    # gemm_x3.h (every shape above with 128 row tiles or more goes there too): its three tile shapes (128, 256 and 320
    # columns), one and several column tiles, both B layouts, ragged M / N / K (K = 36: two full steps and a quarter)
    (8192 + 100, 200, 100, 0, 0, 1), (8192 + 100, 200, 100, 0, 1, 1), (10000, 320, 304, 0, 1, 0), (12000, 130, 36, 0, 0, 2),
    (65536, 300, 300, 0, 0, 2), (65536, 300, 300, 0, 1, 0), (8200, 257, 64, 0, 0, 0), (8200, 31, 16, 0, 1, 0),
    (16384 + 7, 128, 128, 0, 0, 2), (32768 + 9, 300, 300, 0, 1, 0), (32768, 257, 64, 0, 0, 1), (16400, 31, 16, 0, 1, 0), (33000, 1000, 128, 0, 0, 1),
    (33000, 1000, 128, 0, 1, 0), (32768, 700, 36, 0, 0, 2),
    # few rows, a wide N, K >= 256: a tile for every CU from the columns (the loglinear logits over 100 000 entities)
    (2304, 20000, 300, 0, 0, 1), (1100, 30000, 256, 0, 1, 0), (1030, 80000, 260, 0, 0, 0),
    # mid-size products in 128 x 128 tiles, any alignment (the loglinear model of a batch of 1024 over 715 experts: N and the
    # leading dimensions no multiple of four, K = 715 with a partial last piece and a partial last step)
    (3500, 715, 300, 0, 0, 1), (3500, 300, 715, 0, 1, 0), (4099, 513, 301, 0, 0, 2), (2050, 1001, 263, 0, 1, 1), (3000, 716, 300, 0, 0, 0),
])
def test_gemm_dispatch_against_float64(hip_lib, M, N, K, ta, tb, epi):
    rng = np.random.RandomState(M + 3 * N + 7 * K + ta + 2 * tb)
    A = rng.uniform(-1, 1, (K, M) if ta else (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (N, K) if tb else (K, N)).astype(np.float32)
    B *= np.float32(1.0 / np.sqrt(K))
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32) if epi else None
    got = C.debug_gemm(A, B, ta=ta, tb=tb, epi=epi, bias=bias)
    ref = _ref(A, B, ta, tb, epi, bias)
    assert np.all(np.isfinite(got))                       # (the output is pre-filled with NaN: every element was written)
    # fp32 accumulation over K terms of magnitude <= 1/sqrt(K): ~1e-6; fast_tanh adds <= 4 ulp
    assert np.abs(got - ref).max() < (2e-6 if epi != 2 else 3e-6) * max(1.0, np.sqrt(K / 128.0))


@pytest.mark.parametrize('M,N,K,splits', [
    (128, 128, 65536, 512), (300, 300, 65536, 113), (128, 128, 8192 + 24, 7), (300, 300, 4096 + 16, 3), (300, 160, 20000, 40),
    (100, 36, 16384, 64), (320, 320, 8192, 8), (301, 299, 9000, 5),
    # several 128 x 128 output tiles per k range (the loglinear dW, the full softmax's dR_e), ragged last tiles
    (128, 1000, 20000, 20), (1000, 128, 16384, 16), (400, 128, 8192, 32), (130, 260, 4096 + 48, 3),
    # a shorter K with an output wide enough to fill the machine by itself (the loglinear dW over 100 000 entities): one k range
    (300, 41000, 1040, 1), (100, 33000, 1536, 2), (257, 36000, 1100, 1),
    # ... or k ranges enough (the loglinear dW of a batch of 1024: 300 x 715 over ~3 500 distinct words in 57 ranges)
    (300, 715, 3500, 57), (128, 715, 2000, 40),
    # outside gemm_x3.h's split-K shapes (K < 4096): the fp32 MFMA kernels
    (128, 128, 2048, 16), (400, 128, 2048, 8),
])
def test_split_k_with_column_sums_against_float64(hip_lib, M, N, K, splits):
    """dW = h^T.da and db = the column sums of da, as a training step computes them: split-K partial slabs with the column
    sums riding along, combined in a fixed order."""
    rng = np.random.RandomState(M + 3 * N + 7 * K)
    A = rng.uniform(-1, 1, (K, M)).astype(np.float32)
    B = (rng.uniform(-1, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
    got, colsum = C.debug_gemm_splitk(A, B, splits)
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(colsum))
    # fp32 accumulation: a chain of K / splits terms of magnitude <= 1 / sqrt(K) per k range (the bound of the test above
    # for that length), then the order-fixed combine of the ranges
    tol = 2e-6 * max(1.0, np.sqrt(K / splits / 128.0), np.sqrt(K / 128.0) / 8)
    assert np.abs(got - ref).max() < tol
    assert np.abs(colsum - B.astype(np.float64).sum(axis=0)).max() < tol


@pytest.mark.parametrize('tb', [0, 1])
def test_non_finite_operands_stay_confined_to_their_rows_and_columns(hip_lib, tb):
    """gemm_x3.h splits an operand as x0 = bf16(x), x1 = bf16(x - x0), ...: an Inf gives Inf - Inf = NaN in the second piece, so
    where the fp32 MFMA path may return +-Inf this one returns NaN -- either way non-finite (a training step raises on a
    non-finite loss, sert/models.py:372-379), and only in the row of A / column of B the value sits in."""
    M, N, K = 16384 + 64, 128, 128
    rng = np.random.RandomState(7)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = (rng.uniform(-1, 1, (N, K) if tb else (K, N)) / np.sqrt(K)).astype(np.float32)
    A[5, 17] = np.inf
    A[9000, 100] = np.nan
    if tb:
        B[77, 3] = -np.inf
    else:
        B[3, 77] = -np.inf
    got = C.debug_gemm(A, B, ta=0, tb=tb)
    bad = ~np.isfinite(got)
    assert bad[5].all() and bad[9000].all() and bad[:, 77].all()
    bad[5] = bad[9000] = False
    bad[:, 77] = False
    assert not bad.any()


@pytest.mark.parametrize('M,N,K,splits,tb', [
    (2304, 300, 100000, 64, 1), (2304, 300, 50000 + 24, 37, 0), (1100, 128, 65536, 128, 1),
    # a medium K in a few ranges, unaligned (the loglinear dG over 715 experts)
    (3500, 300, 715, 5, 1), (3500, 300, 715, 5, 0),
    # too few tiles x ranges for gemm_x3.h: the fp32 MFMA kernels
    (512, 128, 8192, 8, 1),
])
def test_long_k_in_ranges_against_float64(hip_lib, M, N, K, splits, tb):
    """A.op(B) over a long K cut into k ranges with partial slabs and an order-fixed combine -- the loglinear dG = dZ.W^T over
    a large entity vocabulary (gemm_long_k)."""
    rng = np.random.RandomState(M + 3 * N + 7 * K)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = (rng.uniform(-1, 1, (N, K) if tb else (K, N)) / np.sqrt(K)).astype(np.float32)
    got = C.debug_gemm_longk(A, B, splits, tb=tb)
    ref = A.astype(np.float64) @ (B.astype(np.float64).T if tb else B.astype(np.float64))
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref).max() < 2e-6 * max(1.0, np.sqrt(K / splits / 128.0), np.sqrt(K / 128.0) / 8)


def test_dispatch_on_seeded_random_shapes(hip_lib):
    """Thirty seeded shapes around the dispatch thresholds of gemm_x3.h (row counts about 1024 and 128 tiles, column counts
    about 128 / 256 / 320 and not multiples of four, K about 256 and odd): whichever kernel takes a shape, the result
    is the float64 product to the fp32 accumulation bound."""
    rng = np.random.RandomState(2024)
    for case in range(30):
        tb = int(rng.randint(2))
        epi = int(rng.randint(3)) if not tb else int(rng.choice([0, 1]))
        M = int(rng.choice([1000, 1024, 1500, 3000, 4096, 9000, 16384, 16500, 33000]) + rng.randint(0, 40))
        N = int(rng.choice([7, 100, 127, 128, 129, 200, 256, 257, 300, 320, 321, 715, 1000]))
        K = int(rng.choice([16, 36, 100, 255, 256, 257, 300, 301, 512, 715]))
        A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
        B = (rng.uniform(-1, 1, (N, K) if tb else (K, N)) / np.sqrt(K)).astype(np.float32)
        bias = rng.uniform(-0.5, 0.5, N).astype(np.float32) if epi else None
        got = C.debug_gemm(A, B, ta=0, tb=tb, epi=epi, bias=bias)
        ref = _ref(A, B, 0, tb, epi, bias)
        assert np.all(np.isfinite(got)), (case, M, N, K, tb, epi)
        err = np.abs(got - ref).max()
        assert err < (2e-6 if epi != 2 else 3e-6) * max(1.0, np.sqrt(K / 128.0)), (case, M, N, K, tb, epi, err)


def test_k_range_forms_on_seeded_random_shapes(hip_lib):
    """Sixteen seeded shapes of A^T.B (+ column sums) in k ranges and eight of A.op(B) in k ranges, around the thresholds
    of the split-K forms of gemm_x3.h (128 / 320 rows, 160-column tiles, K about 1024 and 4096, ragged last ranges)."""
    rng = np.random.RandomState(77)
    for case in range(16):
        M = int(rng.choice([36, 128, 129, 300, 320, 321, 400]))
        N = int(rng.choice([36, 128, 160, 161, 300, 715, 1000]))
        K = int(rng.choice([1000, 1024, 2033, 4095, 4096, 9000]) + rng.randint(0, 17))
        splits = int(rng.choice([1, 2, 7, 16, 43]))
        A = rng.uniform(-1, 1, (K, M)).astype(np.float32)
        B = (rng.uniform(-1, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
        got, colsum = C.debug_gemm_splitk(A, B, splits)
        tol = 2e-6 * max(1.0, np.sqrt(K / splits / 128.0), np.sqrt(K / 128.0) / 8)
        assert np.abs(got - A.astype(np.float64).T @ B.astype(np.float64)).max() < tol, (case, M, N, K, splits)
        assert np.abs(colsum - B.astype(np.float64).sum(axis=0)).max() < tol, (case, M, N, K, splits)
    for case in range(8):
        tb = int(rng.randint(2))
        M = int(rng.choice([1024, 2300, 3500]) + rng.randint(0, 9))
        N = int(rng.choice([128, 300, 301]))
        K = int(rng.choice([715, 4096, 20000]) + rng.randint(0, 5))
        splits = int(rng.choice([3, 5, 19]))
        A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
        B = (rng.uniform(-1, 1, (N, K) if tb else (K, N)) / np.sqrt(K)).astype(np.float32)
        got = C.debug_gemm_longk(A, B, splits, tb=tb)
        ref = A.astype(np.float64) @ (B.astype(np.float64).T if tb else B.astype(np.float64))
        assert np.abs(got - ref).max() < 2e-6 * max(1.0, np.sqrt(K / splits / 128.0), np.sqrt(K / 128.0) / 8), (case, M, N, K, splits, tb)


# --------------------------------------------------------------------------- #
# every piece product of gemm_x3.h, to the bit (tests/x3_families.py; that the families reject a kernel with one product
# missing or one plane misrouted, on every element, is proved on the CPU: tests/test_x3_split_cpu.py)
# --------------------------------------------------------------------------- #
# (form, M, N, K, splits, tb): every shape that reaches a kernel form of its own (F.PLAIN_X3 ...: asserted through
# sert_debug_gemm_route in tests/test_x3_split_cpu.py), both B layouts of sert_debug_gemm, and one shape per fp32 kernel -- the
# same expectations hold for a true float32 product, which is what all of them get under SERT_GEMM_FP32=1
EXACT_CASES = ([('plain', M, N, K, 1, tb) for (M, N, K), _ in F.PLAIN_X3 + F.PLAIN_F32 for tb in (0, 1)] +
               [('splitk', M, N, K, splits, 0) for (M, N, K, splits), _ in F.SPLITK] +
               [('longk', M, N, K, splits, tb) for (M, N, K, splits, tb), _ in F.LONGK])
exact_cases = pytest.mark.parametrize('form,M,N,K,splits,tb', EXACT_CASES, ids=['%s-%dx%dx%d-s%d-tb%d' % c for c in EXACT_CASES])


def _product(form, A, B, splits, tb, epi=0, bias=None):
    """op(A) (M, K) . op(B) (K, N) through one of the three hooks, each operand laid out as the form stores it
    -> (C, column sums of B or None)."""
    if form == 'plain':
        return C.debug_gemm(A, F.stored(B, tb), tb=tb, epi=epi, bias=bias), None
    if form == 'splitk':
        return C.debug_gemm_splitk(F.stored(A, True), B, splits)
    return C.debug_gemm_longk(A, F.stored(B, tb), splits, tb=tb), None


def _kper(form, K, splits):
    return None if form == 'plain' else F.k_range(K, splits)


def _same_bits(got, expected, what):
    assert np.all(np.isfinite(got)), what                  # (the output is pre-filled with NaN: every element was written)
    if not np.array_equal(got, expected):
        bad = np.argwhere(got != expected)
        i, j = bad[0]
        raise AssertionError('%s: %d of %d elements differ, rows %d..%d, columns %d..%d; first [%d, %d]: got %r, expected %r'
                             % (what, len(bad), got.size, bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(),
                                i, j, got[i, j], expected[i, j]))


def _column_sums_hold(colsum, B, K, splits):
    """The column sums that ride along the split-K form, under the bound of test_split_k_with_column_sums_against_float64."""
    tol = 2e-6 * max(1.0, np.sqrt(K / splits / 128.0), np.sqrt(K / 128.0) / 8)
    assert np.all(np.isfinite(colsum))
    assert np.abs(colsum - B.astype(np.float64).sum(axis=0)).max() < tol


def _shrink(form, K):
    """Split-K form: a power of two that brings a dense B of magnitudes [0.5, 2) down to the 1 / sqrt(K) the column-sum bound
    was written for (exact: it moves exponents only)."""
    return F.pow2(-int(np.ceil(np.log2(np.sqrt(K)))) - 1) if form == 'splitk' else np.float32(1)


@exact_cases
def test_selection_times_full_mantissa_is_exact(hip_lib, form, M, N, K, splits, tb):
    """One +-2^e per row of op(A), B with all three pieces non-zero everywhere: C[i, j] = +-2^e B[k_i, j] bit for bit -- the
    products a0.b0, a0.b1, a0.b2 and the k every plane of B is read from.  sert_debug_gemm: also with a bias of small
    integers behind it (acc + bias is one float32 addition: the expectation makes the same one)."""
    A, B, expected = F.selection_a(M, N, K, 0, _kper(form, K, splits))
    B, expected = B * _shrink(form, K), expected * _shrink(form, K)
    got, colsum = _product(form, A, B, splits, tb)
    _same_bits(got, expected, 'store')
    if form == 'splitk':
        _column_sums_hold(colsum, B, K, splits)
    if form == 'plain':
        bias = F.rng_of(9, N).integers(-3, 4, N).astype(np.float32)
        _same_bits(_product(form, A, B, splits, tb, epi=1, bias=bias)[0], expected + bias[None, :], 'bias')


@exact_cases
def test_full_mantissa_times_selection_is_exact(hip_lib, form, M, N, K, splits, tb):
    """The mirror image: one +-2^e per column of op(B), A with all three pieces non-zero: C[i, j] = +-2^e A[i, k_j] -- the
    products a0.b0, a1.b0, a2.b0 and the k every plane of A is read from."""
    A, B, expected = F.selection_b(M, N, K, 0, _kper(form, K, splits))
    got, colsum = _product(form, A, B, splits, tb)
    _same_bits(got, expected, 'store')
    if form == 'splitk':
        _column_sums_hold(colsum, B, K, splits)            # (one non-zero per column: the sum is that value)
    if form == 'plain':
        bias = F.rng_of(9, N).integers(-3, 4, N).astype(np.float32)
        _same_bits(_product(form, A, B, splits, tb, epi=1, bias=bias)[0], expected + bias[None, :], 'bias')


@exact_cases
def test_two_piece_operands_keep_the_a1_b1_product(hip_lib, form, M, N, K, splits, tb):
    """Operands of two bfloat16 pieces each (x2 = 0): an output is one product made of the four exact partial products
    a0.b0, a0.b1, a1.b0, a1.b1 -- three float32 additions, 1.5 ulp under round-to-nearest; the bound is F.ULP_BOUND = 4 ulp of
    the exact product (derived, with room for an accumulator that truncates; not measured).  Without a1.b1 every element
    is 31 ulp or more away (tests/test_x3_split_cpu.py)."""
    A, B, exact = F.two_piece_pair(M, N, K, 0, _kper(form, K, splits))
    B, exact = B * _shrink(form, K), exact * float(_shrink(form, K))
    got, colsum = _product(form, A, B, splits, tb)
    assert np.all(np.isfinite(got))
    off = np.abs(got.astype(np.float64) - exact) / F.ulp_of(exact)
    worst = np.unravel_index(off.argmax(), off.shape)
    print('two-piece %s %dx%dx%d tb=%d: worst %.2f ulp' % (form, M, N, K, tb, off[worst]))
    assert off[worst] <= F.ULP_BOUND, (worst, off[worst], got[worst], exact[worst])
    if form == 'splitk':
        _column_sums_hold(colsum, B, K, splits)


@exact_cases
def test_power_of_two_scaling_commutes_with_the_product(hip_lib, form, M, N, K, splits, tb):
    """Dense U(-1, 1) operands as they are, and with row i of op(A) times 2^r_i and column j of op(B) times 2^c_j, r and c
    in [-30, 30]: no piece of a scaled operand is subnormal, so every rounding on the way lands on the scaled value and
    the second product is the first times 2^(r_i + c_j) bit for bit (store epilogue).  The column sums of the split-K form are
    float32 additions of B's elements in a fixed order: they scale the same way."""
    A, B, r, c = F.scaled_pair(M, N, K, 0)
    A2, B2 = F.scale_rows(A, r), F.scale_cols(B, c)
    assert F.smallest_piece_is_normal(A2) and F.smallest_piece_is_normal(B2)
    got, colsum = _product(form, A, B, splits, tb)
    got2, colsum2 = _product(form, A2, B2, splits, tb)
    assert np.all(np.isfinite(got))
    nz = np.abs(got[got != 0])
    assert nz.min() >= 2.0 ** -60 and nz.max() <= 2.0 ** 60       # (the scaled expectation itself neither under- nor overflows)
    _same_bits(got2, F.scale_cols(F.scale_rows(got, r), c), 'scaled')
    if form == 'splitk':
        _column_sums_hold(colsum, B, K, splits)
        assert np.array_equal(colsum2, colsum * F.pow2(c))


# --------------------------------------------------------------------------- #
# the tanh epilogue (fast_tanh, gemm.h) over its whole range, and NaN
# --------------------------------------------------------------------------- #
# one shape per kernel family that has the epilogue, (M, N) of the list above with K = 8: gemm_x3.h (M >= 16384), the
# 128x128-tile kernel (1024 big tiles, K < 256) and the 64x64-tile one (fewer than 512 big tiles)
TANH_SHAPES = [(16384 + 7, 128), (4096, 4096), (1000, 300)]


def _ulp(x, k):
    """x moved by k units in the last place, away from zero for k > 0."""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if (k > 0) == (x > 0) else 0) if x != 0 else np.float32(k), dtype=np.float32)
    return x


def _tanh_values():
    """Pre-activations through both branches of fast_tanh and across its thresholds: 0, the switch at |x| = 0.25 (and one
    ulp to either side), a grid over [-30, 30], the band where float32 tanh saturates (7.9 ... 9.1), the clamp at 10 (and
    one ulp to either side), 88, 1e30, infinity."""
    v = [0.0, -0.0]
    for s in (1.0, -1.0):
        v += [s * 0.25, s * _ulp(0.25, -1), s * _ulp(0.25, 1), s * 7.9, s * 9.1, s * np.float32(12 * np.log(2.0)), s * 10.0,
              s * _ulp(10.0, -1), s * _ulp(10.0, 1), s * 88.0, s * 1e30, s * np.inf, s * 1e-30, s * 1e-3]
    v += list(np.linspace(-30, 30, 81))
    return np.array(v, dtype=np.float32)


@pytest.mark.parametrize('M,N', TANH_SHAPES)
def test_tanh_epilogue_over_its_whole_range(hip_lib, M, N):
    """K = 8 and exact products: A.B is a row-dependent multiple of 0.25 in {-0.5, ..., 0.5} whatever the summation order
    (terms +-1, +-2, +-0.5 that cancel in pairs, and the shift), the bias places the values of _tanh_values -- rows with
    shift 0 see them exactly, the others one rounded sum away.  Element by element against float64 tanh under the bound
    of test_gemm_dispatch_against_float64 for epi = 2: where |a| is large tanh' ~ 0, so a wrong branch (the polynomial
    past 0.25, a missing clamp, a NaN from Inf / Inf) is far outside it."""
    K = 8
    vals = _tanh_values()
    bias = vals[np.arange(N) % len(vals)]
    shift = ((np.arange(M) % 5) - 2).astype(np.float32) * np.float32(0.25)
    A = np.tile(np.array([1, -1, 2, -2, 0.5, -0.5, 0, 0], np.float32), (M, 1))
    A[:, 6] = shift
    B = np.ones((K, N), np.float32)
    got = C.debug_gemm(A, B, epi=2, bias=bias)
    with np.errstate(invalid='ignore'):
        pre = shift[:, None] + bias[None, :]                 # float32: the one rounding the kernel's acc + bias makes
    assert np.all(np.isfinite(pre) | np.isinf(pre))
    ref = np.tanh(pre.astype(np.float64))
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref)
    worst = np.unravel_index(err.argmax(), err.shape)
    assert err.max() < 3e-6, (worst, pre[worst], got[worst], ref[worst])
    assert np.all(np.abs(got) <= 1) and np.array_equal(np.signbit(got), np.signbit(pre))    # tanh(-0.0) = -0.0 included
    # shift 0: the planted values themselves; saturation is exact
    row = got[2]
    assert np.all(row[np.abs(bias) >= 10] == np.sign(bias[np.abs(bias) >= 10])) and np.all(row[bias == 0] == 0)


@pytest.mark.parametrize('M,N', TANH_SHAPES)
def test_tanh_epilogue_keeps_a_nan_in_its_row(hip_lib, M, N):
    """A NaN in A[r, :] under the tanh epilogue: row r non-finite and only row r, as np.tanh gives it (fminf(NaN, 10) = 10
    and NaN < 0.25 is false: fast_tanh once returned +-1 for a NaN)."""
    K = 8
    rng = np.random.RandomState(M + N)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    bias = rng.uniform(-12, 12, N).astype(np.float32)
    rows = [3, M // 2 + 1, M - 1]
    for k, r in enumerate(rows):
        A[r, (3 * k) % K] = np.nan
    got = C.debug_gemm(A, B, epi=2, bias=bias)
    bad = ~np.isfinite(got)
    assert bad[rows].all(), [int(bad[r].sum()) for r in rows]
    bad[rows] = False
    assert not bad.any()


def test_predict_project_and_training_step_keep_a_nan(hip_lib):
    """predict_project of a block with one NaN row returns NaN in that row and the other rows unchanged (np.tanh does);
    and a training step whose batch touches a word row holding one NaN returns a non-finite loss, as the oracle's is --
    lambda = 0, so the L2 term does not carry the NaN into the loss: it has to travel through tanh, the clip of t, the
    sigmoid and the clip of s (fast_tanh and each fminf / fmaxf on the way once dropped it, and the batch loop's non-finite-loss guard,
    sert/models.py:372-379, never fired while the parameters filled with NaN).  Both NCE forms and the softmax variant."""
    from oracle import sert_oracle as O
    from tests import util as U
    for z, de in ((4, 48), (20, 32), (7, 70), (0, 48)):      # vs_nce_regs, vs_nce, vs_nce_scalar, fs_softmax_ce
        B, n, Vw, Ve, dw = 64, 5, 500, 37, 32
        p = U.make_vs_problem(3, B, n, z, Vw, Ve, dw, de, zipf=True)
        p['W'] *= np.float32(20.0)                   # saturated units beside the NaN ones
        if z:
            eng = U.vs_engine(p, B, n, z, 0.0)
        else:
            eng = C.Engine(kind=C.KIND_VECTORSPACE_SOFTMAX, batch_size=B, global_batch_size=B, window_size=n, vocab_size=Vw,
                           num_entities=Ve, word_dim=dw, entity_dim=de, num_negatives=0, id_bytes=p['X'].dtype.itemsize,
                           device=0, keep_grads=1, deterministic=1, lambda_=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=1)
            for which, a in ((C.T_RW, p['Rw']), (C.T_RE, p['Re']), (C.T_W, p['W']), (C.T_B, p['b'])):
                eng.set_tensor(which, a)
        avg = p['rng'].uniform(-1, 1, (9, dw)).astype(np.float32)
        clean = eng.predict_project(avg)
        avg[4, 7] = np.nan
        out = eng.predict_project(avg)
        assert np.isnan(out[4]).all() and np.isnan(np.tanh(avg @ p['W'] + p['b'])[4]).all()
        keep = np.arange(9) != 4
        assert np.array_equal(out[keep], clean[keep])
        # one NaN in the word row of the first token of the batch's last row
        p['Rw'][int(p['X'][B - 1, 0]), dw - 1] = np.nan
        eng.set_tensor(C.T_RW, p['Rw'])
        eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
        neg = p['rng'].randint(0, Ve, size=(B, z)).astype(np.int64) if z else None
        with np.errstate(invalid='ignore'):
            if z:
                ref = O.VectorSpaceOracle(B, n, z, p['Rw'], p['Re'], p['W'], p['b'], 0.0).train_step(p['X'], p['y'], p['w'], neg)
            else:
                ref = O.VectorSpaceSoftmaxOracle(B, n, p['Rw'], p['Re'], p['W'], p['b'], 0.0).train_step(p['X'], p['y'], p['w'])
        assert not np.isfinite(ref)
        loss = eng.train_batch(0, neg) if z else eng.train_batch(0)
        assert not np.isfinite(loss), (z, de, loss)
        eng.close()
