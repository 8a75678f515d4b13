"""The arithmetic behind csrc/gemm_x3.h, restated in NumPy (no GPU): a float32 splits EXACTLY into three bfloat16 pieces
(round to nearest even, as v_cvt_pk_bf16_f32 does), and the six products a_p b_q with p + q <= 2 -- each exact in the
bf16 MFMA, accumulated here in float64 -- leave an error two orders of magnitude below that of an fp32 GEMM.  The kernel
itself is pinned against float64 on the GPU (tests/test_gpu_gemm.py); this file pins the claim the kernel rests on -- and
proves that the exact-product families of tests/x3_families.py, which pin every one of the six products on the device,
reject a kernel that drops any of them or reads any plane from the wrong k, on every element of the output."""
import numpy as np
import pytest

from sert_amd import _capi as C
from tests import x3_families as F
from tests.x3_families import bf16_rne, split3


def test_three_bf16_pieces_add_up_to_the_float32_bit_for_bit():
    rng = np.random.RandomState(0)
    samples = [rng.standard_normal(200000).astype(np.float32),
               (rng.standard_normal(200000) * 1e-3).astype(np.float32),
               rng.uniform(-1, 1, 200000).astype(np.float32) * np.float32(2.0) ** rng.randint(-60, 60, 200000).astype(np.float32),
               np.array([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 3.0000002, 0.1, 1e-30, -1e30, 255.99998,
                         1.9999999, 2.0 ** -100], dtype=np.float32)]
    for x in samples:
        x0, x1, x2 = split3(x)
        # every piece is a bfloat16 (its low 16 bits are zero) ...
        for piece in (x0, x1, x2):
            assert not np.any(piece.view(np.uint32) & 0xffff)
        # ... and the three add up to x exactly
        total = x0.astype(np.float64) + x1.astype(np.float64) + x2.astype(np.float64)
        assert np.array_equal(total, x.astype(np.float64))


def test_six_products_are_closer_to_float64_than_an_fp32_gemm():
    rng = np.random.RandomState(1)
    M, K, N = 256, 300, 300
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    scale = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    a, b = split3(A), split3(B)
    six = sum(a[p].astype(np.float64) @ b[q].astype(np.float64) for p in range(3) for q in range(3) if p + q <= 2)
    nine = sum(a[p].astype(np.float64) @ b[q].astype(np.float64) for p in range(3) for q in range(3))
    err6 = (np.abs(six - ref) / scale).max()
    err9 = (np.abs(nine - ref) / scale).max()
    err32 = (np.abs((A @ B).astype(np.float64) - ref) / scale).max()
    assert err9 < 1e-15                       # nine products: the exact product of the exact splits
    assert err6 < 3 * 2.0 ** -24 * 0.2        # the three dropped ones: far below 3 . 2^-24 |a||b| (they rarely align)
    assert err6 < err32 / 20                  # ... and far below what the fp32 accumulation alone costs
    # three products (the "bf16 x 3" of some libraries) would NOT do: 1e-6, an order above fp32
    three = sum(a[p].astype(np.float64) @ b[q].astype(np.float64) for p, q in ((0, 0), (0, 1), (1, 0)))
    assert (np.abs(three - ref) / scale).max() > 2 * err32


# --------------------------------------------------------------------------- #
# the exact-product families (tests/x3_families.py): a model of the kernel, intact and with one defect at a time
# --------------------------------------------------------------------------- #
TERMS = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))       # the kernel's order, smallest first
# two steps of 16 and a ragged one of 8; rows and columns enough for the selection to visit every k
MUT_M, MUT_N, MUT_K = 96, 80, 40


def kernel_model(A, B, drop=None, roll=None):
    """op(A) (M, K) . op(B) (K, N) as gemm_x3.h forms it: six piece products, each exact, summed (in float64) and stored
    as float32.  drop = (p, q): without that product.  roll = ('a' | 'b', piece): that plane of that operand read from
    k - 1 in every product that uses it."""
    a, b = list(split3(A)), list(split3(B))
    if roll:
        if roll[0] == 'a':
            a[roll[1]] = np.roll(a[roll[1]], 1, axis=1)
        else:
            b[roll[1]] = np.roll(b[roll[1]], 1, axis=0)
    acc = np.zeros((A.shape[0], B.shape[1]))
    for p, q in TERMS:
        if (p, q) != drop:
            acc += a[p].astype(np.float64) @ b[q].astype(np.float64)
    return acc.astype(np.float32)


def _ulps_off_two_piece(drop=None, roll=None):
    A, B, exact = F.two_piece_pair(MUT_M, MUT_N, MUT_K, 0)
    return np.abs(kernel_model(A, B, drop, roll).astype(np.float64) - exact) / F.ulp_of(exact)


def test_families_are_built_as_described():
    A, B, _ = F.selection_a(MUT_M, MUT_N, MUT_K, 0)
    assert np.all((A != 0).sum(axis=1) == 1) and set(np.nonzero(A)[1]) == set(range(MUT_K))
    assert np.all((np.abs(B) >= 0.5) & (np.abs(B) < 2)) and np.all(B.view(np.uint32) & 1)
    assert all(np.all(p != 0) for p in split3(B))
    e = np.log2(np.abs(A[A != 0]))
    assert np.all(e == np.round(e)) and e.min() >= -F.E_RANGE and e.max() <= F.E_RANGE
    A, B, _ = F.selection_b(MUT_M, MUT_N, MUT_K, 0)
    assert np.all((B != 0).sum(axis=0) == 1) and set(np.nonzero(B)[0]) == set(range(MUT_K))
    assert all(np.all(p != 0) for p in split3(A))
    # fewer lines than k: distinct, with the last 32, the first 16 and both sides of every range boundary among them
    k, _ = F.selection(F.rng_of(5), 128, 4120, kper=272)
    assert len(set(k)) == 128 and set(range(4120 - 32, 4120)) | set(range(16)) | {271, 272, 3807, 3808} <= set(k)
    # two pieces and no third, in the selection and in the dense operand
    A, B, _ = F.two_piece_pair(MUT_M, MUT_N, MUT_K, 0)
    for x in (A[A != 0], B):
        x0, x1, x2 = split3(x)
        assert np.all(x2 == 0) and np.all(x1 != 0)
        assert np.all((np.abs(x0) >= 1) & (np.abs(x0) < 1.5)) and np.all((np.abs(x1) >= 0.75 * 2.0 ** -8) & (np.abs(x1) < 2.0 ** -8))
    # scaling: no piece of a scaled operand is subnormal (the whole split, and the cheap sufficient test the device tests use)
    A, B, r, c = F.scaled_pair(MUT_M, MUT_N, MUT_K, 0)
    for x in (F.scale_rows(A, r), F.scale_cols(B, c)):
        assert F.smallest_piece_is_normal(x)
        for p in split3(x):
            assert np.all((p == 0) | (np.abs(p) >= 2.0 ** -126))
    assert r.min() >= -F.E_RANGE and r.max() <= F.E_RANGE and len(set(r)) > 20 and len(set(c)) > 20


def test_the_intact_model_meets_every_family():
    for family in (F.selection_a, F.selection_b):
        A, B, expected = family(MUT_M, MUT_N, MUT_K, 0)
        assert np.array_equal(kernel_model(A, B), expected)
    assert _ulps_off_two_piece().max() <= 0.5            # (the model adds in float64: one rounding)
    A, B, r, c = F.scaled_pair(MUT_M, MUT_N, MUT_K, 0)
    plain = kernel_model(A, B)
    assert np.array_equal(kernel_model(F.scale_rows(A, r), F.scale_cols(B, c)), F.scale_cols(F.scale_rows(plain, r), c))


@pytest.mark.parametrize('drop', [(0, 1), (0, 2), (1, 0), (2, 0), (1, 1)])
def test_a_dropped_product_is_rejected_on_every_element(drop):
    """Each of the five small products removed in turn: the family that claims it fails everywhere -- the exact ones by a
    bit (their bound is zero), the two-piece one at four times its bound or more."""
    if drop == (1, 1):
        off = _ulps_off_two_piece(drop=drop)
        assert off.min() >= 4 * F.ULP_BOUND, off.min()
        assert off.min() >= 31                            # 2^-18 relative (x3_families.py)
        return
    family = F.selection_a if drop[0] == 0 else F.selection_b
    A, B, expected = family(MUT_M, MUT_N, MUT_K, 0)
    assert np.all(kernel_model(A, B, drop=drop) != expected)


@pytest.mark.parametrize('operand,piece', [('a', 0), ('a', 1), ('a', 2), ('b', 0), ('b', 1), ('b', 2)])
def test_a_plane_read_from_the_wrong_k_is_rejected_on_every_element(operand, piece):
    family = F.selection_a if operand == 'b' else F.selection_b
    A, B, expected = family(MUT_M, MUT_N, MUT_K, 0)
    assert np.all(kernel_model(A, B, roll=(operand, piece)) != expected)


def test_three_products_only_fail_every_family_that_looks_at_the_others():
    """The "bf16 x 3" kernel (a0.b0, a0.b1, a1.b0) the float64 tests cannot tell from the real one at K = 1000."""
    def three(A, B):
        a, b = split3(A), split3(B)
        return sum(a[p].astype(np.float64) @ b[q].astype(np.float64) for p, q in ((0, 1), (1, 0), (0, 0))).astype(np.float32)
    for family in (F.selection_a, F.selection_b):
        A, B, expected = family(MUT_M, MUT_N, MUT_K, 0)
        assert np.all(three(A, B) != expected)
    A, B, exact = F.two_piece_pair(MUT_M, MUT_N, MUT_K, 0)
    assert (np.abs(three(A, B).astype(np.float64) - exact) / F.ulp_of(exact)).min() >= 4 * F.ULP_BOUND


# --------------------------------------------------------------------------- #
# the shapes of the device tests reach every kernel form (sert_debug_gemm_route: the launchers' own predicates)
# --------------------------------------------------------------------------- #
def _routes(fp32):
    got = {}
    for (M, N, K), want in F.PLAIN_X3 + F.PLAIN_F32:
        for tb in (0, 1):
            got[('plain', M, N, K, tb)] = (C.debug_gemm_route(C.GEMM_FORM_PLAIN, M, N, K, tb=tb), want)
    for (M, N, K, splits), want in F.SPLITK:
        got[('splitk', M, N, K, splits)] = (C.debug_gemm_route(C.GEMM_FORM_SPLITK, M, N, K, splits=splits), want)
    for (M, N, K, splits, tb), want in F.LONGK:
        got[('longk', M, N, K, splits, tb)] = (C.debug_gemm_route(C.GEMM_FORM_LONGK, M, N, K, tb=tb, splits=splits), want)
    return got


def test_device_test_shapes_reach_every_kernel_form(hip_lib, monkeypatch):
    """Host only.  Every shape of the exact-product device tests lands on the kernel form it was chosen for, and together
    they reach all ten; a dispatch threshold that moves fails here instead of quietly dropping an instantiation from the
    tests.  Under SERT_GEMM_FP32=1 the same shapes all go to the fp32 kernels."""
    monkeypatch.delenv('SERT_GEMM_FP32', raising=False)
    routes = _routes(False)
    wrong = {k: v for k, v in routes.items() if v[0] != v[1]}
    assert not wrong, wrong
    assert {v[0] for v in routes.values()} == set(C.GEMM_ROUTES)
    # the unaligned start of an operand sends an aligned shape to the dword loaders
    assert C.debug_gemm_route(C.GEMM_FORM_PLAIN, 3500, 716, 300, align=4) == 'x3_128_scalar'
    monkeypatch.setenv('SERT_GEMM_FP32', '1')
    assert {v[0] for v in _routes(True).values()} == {'f32_tile64', 'f32_tile128', 'f32_tile128x160'}
    with pytest.raises(C.SertError):
        C.debug_gemm_route(C.GEMM_FORM_PLAIN, 0, 128, 128)
