"""Operands of 2 GiB and more: the shapes on both sides of every size guard of the GEMM dispatch, and loglinear batches whose
logit tables pass 2^31 and 2^32 bytes -- shared by the CPU proof of the inputs (test_big_offset_inputs_cpu.py) and the GPU
test (test_gpu_big_offsets.py).

A. GEMM.  gemm_x3.h addresses a tile as one buffer descriptor over the whole operand plus a 32-bit lane offset, the dword
loaders keep bit 31 of that offset as their "outside the tile" flag, and x3_shape_ok admits a shape only while the guarded
extent -- M.lda, N.ldb / K.ldb (A.op(B)), K.max(lda, ldb) (A^T.B) -- stays below GUARD = 2^29 elements (2 GiB); the fp32
MFMA kernels of gemm.h take their 16-byte loaders only for leading dimensions below LD_GUARD = 2^22.  GEMM_ROWS lists, per
guard and kernel form, the smallest pair of shapes `under` / `at` the guard with the route each takes
(sert_debug_gemm_route at this commit; the CPU test asserts all of them).

A uniform random fill of 2 GiB and a float64 product of it would cost seconds per case, so the operand that carries the
guarded extent is built from a POOL: line i along the guarded axis is 2^e(i) pool[h(i)], pool = 256 lines of U(-1, 1),
h a multiplicative hash of i, e(i) in [-4, 4].  The float64 reference is then the product of the POOL with the small
operand, gathered by h: every element of the output is checked, against got / 2^e (a power of two: exact), under the bounds
of test_gpu_gemm.py.  Where the guarded axis is K itself (A^T.B over 4 194 304 rows of A and of B) the pool runs along k --
rows k of A and of B are the pool lines h(k), each times a hashed sign, A's also times 2^e(k) with e in [-4, 0] so that
|a| <= 1 holds as the bound assumes -- and the reference is poolA^T diag(weights) poolB.  The last row (a leading dimension
of 2^22, K contiguous) does not fit a pool along a line: a plain random fill, and a float64 reference accumulated over
blocks of k, at 64 x 32 outputs.

B. Loglinear.  A full-batch oracle of a 10^9-element softmax is out of reach in NumPy; the cases TILE a small problem of P
rows whose P n tokens are distinct words: the engine's batch has B = c P rows, every token its own word (U = B n),
R_w[u] = R_small[u mod P n], labels and weights of period P.  Then loss, dW and db are the small problem's and
dR_w[u] = (P / B) dR_small[u mod P n] (test 4 of the CPU file proves the identity on the oracle).  P is odd: P n must not
divide the row distance that 2^31 or 2^32 bytes make in the table, or a wrapped read would land on an identical row.

The loss form a batch takes is decided in ll_forward (host/step_softmax_loglinear.inc): ll_row_wave and ll_row_from_table
only while the (n + 1) V_e 4 bytes of a row's slab would fit the fused kernel's 150 KB of LDS -- n <= 17 at V_e = 2048.
So the two cases that aim at those kernels have n = 17 (`wave_2to4GiB`, `table_over_4GiB`), and the windows of 40 and 64 at
the same table sizes are cases of their own, which the streaming kernels take with the slot table
(`stream_slots_2to4GiB`, `stream_slots_over_4GiB`)."""
import numpy as np

from oracle import sert_oracle as O

GUARD = 1 << 29            # elements: gemm_x3.h, x3_shape_ok
LD_GUARD = 1 << 22         # elements: gemm.h, gemm_f32_vec
POOL = 256
MARK31, MARK32 = 1 << 31, 1 << 32      # bytes

# id -> hook ('plain' = debug_gemm, 'splitk' = debug_gemm_splitk, 'longk' = debug_gemm_longk), the (M, N, K) under and at the
# guard, tb, splits, the construction (`build`: which operand carries the guarded extent, and along which axis the pool
# runs) and the route on either side.
GEMM_ROWS = {
    'a_rows_vec_tb0': dict(hook='plain', under=(131071, 128, 4096), at=(131072, 128, 4096), tb=0, splits=1, build='a_rows',
                           routes=('x3_128_vec', 'f32_tile128')),
    'a_rows_vec_tb1': dict(hook='plain', under=(131071, 128, 4096), at=(131072, 128, 4096), tb=1, splits=1, build='a_rows',
                           routes=('x3_128_vec', 'f32_tile128')),
    'a_rows_dword': dict(hook='plain', under=(131104, 128, 4095), at=(131105, 128, 4095), tb=0, splits=1, build='a_rows',
                         routes=('x3_128_scalar', 'f32_tile128')),
    'a_rows_256': dict(hook='plain', under=(131071, 256, 4096), at=(131072, 256, 4096), tb=0, splits=1, build='a_rows',
                       routes=('x3_256', 'f32_tile128')),
    'a_rows_320': dict(hook='plain', under=(131071, 300, 4096), at=(131072, 300, 4096), tb=1, splits=1, build='a_rows',
                       routes=('x3_320', 'f32_tile128x160')),
    'b_cols_plain': dict(hook='plain', under=(1024, 131068, 4096), at=(1024, 131072, 4096), tb=0, splits=1, build='b_cols',
                         routes=('x3_256', 'f32_tile128')),
    'b_rows_plain': dict(hook='plain', under=(1024, 131068, 4096), at=(1024, 131072, 4096), tb=1, splits=1, build='b_rows',
                         routes=('x3_256', 'f32_tile128')),
    'b_cols_ta_tiles': dict(hook='splitk', under=(128, 131068, 4096), at=(128, 131072, 4096), tb=0, splits=16, build='b_cols',
                            routes=('x3_ta_tiles', 'f32_tile128')),
    'b_cols_ta_320x160': dict(hook='splitk', under=(300, 131068, 4096), at=(300, 131072, 4096), tb=0, splits=16, build='b_cols',
                              routes=('x3_ta_320x160', 'f32_tile128')),
    'k_rows_ta_single': dict(hook='splitk', under=(128, 128, 4194288), at=(128, 128, 4194304), tb=0, splits=512, build='k_rows',
                             routes=('x3_ta_single', 'f32_tile128')),
    'dg_tb1': dict(hook='longk', under=(5368, 300, 100000), at=(5369, 300, 100000), tb=1, splits=64, build='a_rows',
                   routes=('x3_320', 'f32_tile128x160')),
    'dg_tb0': dict(hook='longk', under=(5368, 300, 100000), at=(5369, 300, 100000), tb=0, splits=64, build='a_rows',
                   routes=('x3_320', 'f32_tile128x160')),
    'dg_unaligned': dict(hook='longk', under=(5368, 300, 100001), at=(5369, 300, 100001), tb=1, splits=64, build='a_rows',
                         routes=('x3_128_scalar', 'f32_tile128')),
    'ld_2to22': dict(hook='longk', under=(64, 32, 4194300), at=(64, 32, 4194304), tb=1, splits=64, build='k_plain',
                     routes=('f32_tile128', 'f32_tile128')),
}
SIDES = ('under', 'at')


def guarded_extent(row, side):
    """The number the row's guard looks at, in elements, and the bound it is compared with."""
    M, N, K = row[side]
    if row['build'] == 'a_rows':
        return M * K, GUARD                       # M.lda
    if row['build'] == 'b_rows':
        return N * K, GUARD                       # N.ldb, B stored (N, K)
    if row['build'] == 'b_cols':
        return K * N, GUARD                       # K.ldb, B stored (K, N) -- of A.B and of A^T.B (lda = M is smaller)
    if row['build'] == 'k_rows':
        return K * max(M, N), GUARD               # K.max(lda, ldb)
    return K, LD_GUARD                            # the leading dimension of both operands


def bound(row, side):
    """The float64 bounds of test_gpu_gemm.py for the row's hook, unchanged."""
    M, N, K = row[side]
    if row['hook'] == 'plain':
        return 2e-6 * max(1.0, np.sqrt(K / 128.0))
    return 2e-6 * max(1.0, np.sqrt(K / row['splits'] / 128.0), np.sqrt(K / 128.0) / 8)


def hash_lines(count, along_k=False):
    """(h, e) of the lines 0 .. count - 1 along a guarded axis: h in [0, POOL), e in [-4, 4] -- in [-4, 0] for the pool
    along k, where the scale cannot be divided out of a sum over k and |a| <= 1 has to hold as it is."""
    i = np.arange(count, dtype=np.uint64)
    h = (((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(24)).astype(np.int64)
    spread = 5 if along_k else 9
    e = ((((i * np.uint64(2246822519)) & np.uint64(0xffffffff)) >> np.uint64(15)) % np.uint64(spread)).astype(np.int64) - 4
    return h, e


def hash_signs(count):
    """Two independent +-1 per line (float32), for the pool along k."""
    i = np.arange(count, dtype=np.uint64)
    bit = lambda mult: ((((i * np.uint64(mult)) & np.uint64(0xffffffff)) >> np.uint64(31)) & np.uint64(1)).astype(np.float32)
    return np.float32(1) - 2 * bit(3266489917), np.float32(1) - 2 * bit(668265263)


def line_distances(row):
    """The distances, in lines of the guarded axis, a wrong offset would confuse: what 2^31 and 2^32 bytes make (where
    shorter than the axis) and one tile of every tile height in use (128, 256, 320 lines)."""
    M, N, K = row['at']
    per_line = {'a_rows': K, 'b_rows': K, 'b_cols': 1, 'k_rows': max(M, N)}[row['build']] * 4      # bytes from a line to the next
    count = lines_of(row, 'at')
    out = [t for t in (128, 256, 320)]
    for mark in (MARK31, MARK32):
        if mark % per_line == 0 and 0 < mark // per_line < count:
            out.append(mark // per_line)
    # (half the extent: where the mark would lie for a guard off by a factor of two)
    out.append(count // 2)
    return out


def lines_of(row, side):
    M, N, K = row[side]
    return {'a_rows': M, 'b_rows': N, 'b_cols': N, 'k_rows': K}[row['build']]


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (k + 1) for k, c in enumerate(name)))


def _uniform(rng, shape):
    return (rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1))


def _gather_lines(pool, h, scale):
    """out[i] = scale[i] * pool[h[i]] without a temporary of the output's size."""
    out = np.empty((len(h), pool.shape[1]), dtype=np.float32)
    np.take(pool, h, axis=0, out=out, mode='clip')
    out *= scale[:, None]
    return out


class GemmOperands(object):
    """The operands of one row of GEMM_ROWS at its `at` shape, and what the reference needs.  sides(side) -> the stored
    arrays of a side (views where a slice of the big operand is contiguous); reference(side) -> a function of an output
    block."""

    def __init__(self, name, small_only=False):
        self.name, self.row = name, GEMM_ROWS[name]
        row, rng = self.row, _rng(name)
        M, N, K = row['at']
        build = row['build']
        self.h = self.e = None
        if build == 'a_rows':
            self.h, self.e = hash_lines(M)
            self.pool = _uniform(rng, (POOL, K))
            self.small = _uniform(rng, (N, K) if row['tb'] else (K, N)) * np.float32(1.0 / np.sqrt(K))
            b64 = self.small.astype(np.float64)
            self.pool_product = self.pool.astype(np.float64) @ (b64.T if row['tb'] else b64)            # (POOL, N)
        elif build in ('b_rows', 'b_cols'):
            self.h, self.e = hash_lines(N)
            self.pool = _uniform(rng, (POOL, K)) * np.float32(1.0 / np.sqrt(K))
            # the other operand: A (M, K), or stored (K, M) for A^T.B
            self.small = _uniform(rng, (K, M) if row['hook'] == 'splitk' else (M, K))
            a64 = self.small.astype(np.float64)
            self.pool_product = (a64.T if row['hook'] == 'splitk' else a64) @ self.pool.astype(np.float64).T   # (M, POOL)
            self.pool_colsum = self.pool.astype(np.float64).sum(axis=1)                                   # (POOL,)
        elif build == 'k_rows':
            self.h, self.e = hash_lines(K, along_k=True)
            self.pool = _uniform(rng, (POOL, M))                                                           # lines of A (K, M)
            self.pool_b = _uniform(rng, (POOL, N)) * np.float32(1.0 / np.sqrt(K))                          # lines of B (K, N)
        self.scale = None if self.e is None else np.ldexp(np.float32(1), self.e).astype(np.float32)
        if build == 'k_rows':
            # 16 384 copies of each pool line ADD UP along k: without signs the sums are fifty times a random product's and
            # so is their fp32 rounding, which the bound does not price.  A hashed sign per k and operand (exact, |a| <= 1)
            # makes the sum over k the random walk the bound was written for.
            sign_a, self.scale_b = hash_signs(K)
            self.scale *= sign_a
        self.big = self.big_b = None
        if small_only:
            return
        if build in ('a_rows', 'b_rows'):
            self.big = _gather_lines(self.pool, self.h, self.scale)
        elif build == 'b_cols':
            self.big = np.take(np.ascontiguousarray(self.pool.T), self.h, axis=1)                          # (K, N)
            self.big *= self.scale[None, :]
        elif build == 'k_rows':
            self.big = _gather_lines(self.pool, self.h, self.scale)
            self.big_b = _gather_lines(self.pool_b, self.h, self.scale_b)
        else:
            self.big = _uniform(rng, (M, K))
            self.big_b = _uniform(rng, (N, K)) * np.float32(1.0 / np.sqrt(K))

    def stored(self, side):
        """(A, B) as the row's hook takes them, at the shape of `side`."""
        row = self.row
        M, N, K = row[side]
        build = row['build']
        if build == 'a_rows':
            return self.big[:M], self.small
        if build == 'b_rows':
            return self.small, self.big[:N]
        if build == 'b_cols':
            return self.small, np.ascontiguousarray(self.big[:, :N])
        if build == 'k_rows':
            return self.big[:K], self.big_b[:K]
        return np.ascontiguousarray(self.big[:, :K]), np.ascontiguousarray(self.big_b[:, :K])

    def k_rows_reference(self, side, h=None, scale=None, scale_b=None):
        """(C, column sums of B) in float64 for the pool along k: per pool line, the sum over the k that hold it of the
        product of the two operands' scales (and of B's alone) -- exact --, then poolA^T diag(.) poolB.  h, scale, scale_b:
        another assignment of lines to k than the case's own (the CPU test's failure modes)."""
        K = self.row[side][2]
        h = self.h[:K] if h is None else h
        scale = (self.scale[:K] if scale is None else scale).astype(np.float64)
        scale_b = (self.scale_b[:K] if scale_b is None else scale_b).astype(np.float64)
        wt = np.bincount(h, weights=scale * scale_b, minlength=POOL)
        wt_b = np.bincount(h, weights=scale_b, minlength=POOL)
        a64, b64 = self.pool.astype(np.float64), self.pool_b.astype(np.float64)
        return (a64 * wt[:, None]).T @ b64, wt_b @ b64

    def k_plain_reference(self, side, block=1 << 18):
        K = self.row[side][2]
        acc = np.zeros((self.big.shape[0], self.big_b.shape[0]))
        for k0 in range(0, K, block):
            acc += self.big[:, k0:min(K, k0 + block)].astype(np.float64) @ self.big_b[:, k0:min(K, k0 + block)].astype(np.float64).T
        return acc

    def worst_error(self, side, got, colsum=None, block=8192):
        """max |got / 2^e - reference| over EVERY element (and over the column sums), blockwise along the guarded axis."""
        row = self.row
        M, N, K = row[side]
        build = row['build']
        assert got.shape == (M, N), (got.shape, row[side])
        if build == 'k_rows':
            ref, cs = self.k_rows_reference(side)
            return float(np.abs(got - ref).max()), float(np.abs(colsum - cs).max())
        if build == 'k_plain':
            return float(np.abs(got - self.k_plain_reference(side)).max()), None
        worst = worst_cs = 0.0
        for i0 in range(0, lines_of(row, side), block):
            sl = slice(i0, min(lines_of(row, side), i0 + block))
            inv = (1.0 / self.scale[sl]).astype(np.float64)
            if build == 'a_rows':
                worst = max(worst, float(np.abs(got[sl] * inv[:, None] - self.pool_product[self.h[sl]]).max()))
            else:
                worst = max(worst, float(np.abs(got[:, sl] * inv[None, :] - self.pool_product[:, self.h[sl]]).max()))
                if colsum is not None:
                    worst_cs = max(worst_cs, float(np.abs(colsum[sl] * inv - self.pool_colsum[self.h[sl]]).max()))
        return worst, (worst_cs if colsum is not None else None)


_gemm_cache = {}


def gemm_operands(name):
    """The operands of a row, built once and kept until ANOTHER row is asked for (one 2 GiB operand alive at a time; the
    `under` and `at` cases of a row follow each other and share it)."""
    if name not in _gemm_cache:
        _gemm_cache.clear()
        _gemm_cache[name] = GemmOperands(name)
    return _gemm_cache[name]


def release_gemm_operands():
    _gemm_cache.clear()


# --------------------------------------------------------------------------- #
# B. tiled loglinear problems
# --------------------------------------------------------------------------- #
D, VE = 8, 2048
# id -> P, n, c (B = c P), V_e, the form of the step (Engine.ll_loss_form: form, param) and the mark the table passes
LL_TRAIN = {
    'wave_2to4GiB': dict(P=63, n=17, c=306, Ve=VE, form=('wave', 8), above=MARK31, below=MARK32),
    'table_over_4GiB': dict(P=63, n=17, c=490, Ve=VE, form=('table', 128), above=MARK32, below=None),
    'stream_slots_2to4GiB': dict(P=63, n=40, c=130, Ve=VE, form=('stream', 1), above=MARK31, below=MARK32),
    'stream_slots_over_4GiB': dict(P=63, n=64, c=131, Ve=VE, form=('stream', 1), above=MARK32, below=None),
}
# per-token logits of a validation batch (no index: one row of Z per token) past 2^32 bytes, both streaming forms
LL_EVAL = {
    'eval_tokens_over_4GiB_v4': dict(P=16, n=10, c=64, Ve=106000, form=('stream', 1), above=MARK32, below=None),
    'eval_tokens_over_4GiB_scalar': dict(P=16, n=10, c=64, Ve=106001, form=('stream', 0), above=MARK32, below=None),
}
LL_SEEDS = {name: 500 + k for k, name in enumerate(list(LL_TRAIN) + list(LL_EVAL))}


def table_bytes(case, c=None):
    """Bytes of the logit table the case's loss kernels read: one row of V_e floats per token (= per distinct word)."""
    return case['P'] * (case['c'] if c is None else c) * case['n'] * case['Ve'] * 4


def ll_small_problem(name, Ve=None):
    """The small problem of a case: P rows, every token its own word.  R_w is U(-1, 1) rather than Glorot-scale so that two
    words' logit rows differ by far more than the loss tolerance; the bias is narrow (0.3 / n around 0.3, as
    tests/ll_csr_cases.py argues for long windows) so that no probability comes near a clip bound."""
    case = (LL_TRAIN.get(name) or LL_EVAL[name])
    P, n = case['P'], case['n']
    Ve = case['Ve'] if Ve is None else Ve
    rng = np.random.RandomState(LL_SEEDS[name])
    Rw = rng.uniform(-1, 1, (P * n, D)).astype(np.float32)
    W = O.glorot_uniform(rng, (D, Ve))
    b = (0.3 + (0.3 / n) * rng.randn(Ve)).astype(np.float32)
    X = np.arange(P * n).reshape(P, n)
    y = rng.randint(0, Ve, size=P).astype(np.int32)
    w = rng.uniform(0.5, 2.0, P).astype(np.float32)
    return dict(Rw=Rw, W=W, b=b, X=X, y=y, w=w, P=P, n=n, Ve=Ve)


def ll_tiled(small, c, distinct=True):
    """The engine's problem: c copies of the small one.  distinct: every token its own word (a training split, U = B n);
    else the small problem's ids repeated (a validation split: no index, one logit row per token)."""
    P, n = small['P'], small['n']
    B = c * P
    vocab = B * n if distinct else P * n
    dt = np.min_scalar_type(vocab - 1)
    X = (np.arange(B * n).reshape(B, n) if distinct else np.tile(small['X'], (c, 1))).astype(dt)
    return dict(Rw=np.tile(small['Rw'], (c, 1)) if distinct else small['Rw'], W=small['W'], b=small['b'], X=X,
                y=np.tile(small['y'], c), w=np.tile(small['w'], c), B=B, n=n)


_ll_refs = {}


def ll_reference(name):
    """The oracle on the small problem of a case, once per process: float32 and float64 loss, gradients, per-row loss."""
    if name not in _ll_refs:
        s = ll_small_problem(name)
        out = {}
        for dt in (np.float32, np.float64):
            ora = O.LogLinearOracle(s['P'], s['n'], s['Rw'], s['W'], s['b'], 0.0, dtype=dt)
            loss, grads, f = ora.loss_and_grads(s['X'], s['y'], s['w'])
            out[np.dtype(dt).name] = dict(loss=loss, grads=grads, rowloss=np.asarray(f['loss']), Q=f['Q'], P3min=float(f['P3'].min()),
                                          P3max=float(f['P3'].max()), eval_loss=ora.eval_loss(s['X'], s['y']))
        _ll_refs[name] = (s, out)
    return _ll_refs[name]
