"""Shared helpers for the parity tests (oracle = checker, HIP engine = subject)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from oracle import sert_oracle as O
from sert_amd import _capi as C


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def row_err(a, b, rows=None, floor=1e-3):
    """Row-wise companion of rel_err: max over rows r of ||a_r - b_r||_2 / max(||b_r||_2, floor * median_r ||b_r||_2).
    rel_err is a bound against the largest element of the WHOLE tensor -- a wrong row whose magnitude is 1e-4
    of the largest row passes it; this one prices every row against its own norm (the floor only keeps rows that
    are numerically empty -- cancelled sums, untouched rows under lambda = 0 -- from dividing by ~0).  `rows`
    restricts the maximum to a subset (e.g. the rows a batch touches).  Returns (worst error, its row)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.ndim == 2, (a.shape, b.shape)
    if rows is not None:
        rows = np.asarray(rows)
        a, b = a[rows], b[rows]
    nb = np.sqrt((b * b).sum(axis=1))
    den = np.maximum(nb, floor * max(1e-30, float(np.median(nb))))
    e = np.sqrt(((a - b) ** 2).sum(axis=1)) / den
    i = int(np.argmax(e))
    return float(e[i]), (int(rows[i]) if rows is not None else i)


def id_dtype(vocab):
    return np.min_scalar_type(vocab - 1)


def make_vs_problem(seed, N, n, z, Vw, Ve, dw, de, weights='uniform', zipf=False):
    rng = np.random.RandomState(seed)
    Rw = O.glorot_uniform(rng, (Vw, dw))
    Re = O.glorot_uniform(rng, (Ve, de))
    W = O.glorot_uniform(rng, (dw, de))
    b = (0.1 * rng.randn(de)).astype(np.float32)
    if zipf:
        r = np.minimum(rng.zipf(1.1, size=(N, n)) - 1, Vw - 1)
        X = rng.permutation(Vw)[r]
    else:
        X = rng.randint(0, Vw, size=(N, n))
    X = X.astype(id_dtype(Vw))
    y = rng.randint(0, Ve, size=N).astype(np.int32)
    w = (np.ones(N) if weights == 'ones' else rng.uniform(0.5, 2.0, N)).astype(np.float32)
    return dict(Rw=Rw, Re=Re, W=W, b=b, X=X, y=y, w=w, rng=rng)


def vs_engine(p, B, n, z, lam, device=0, keep_grads=1, global_batch=None, seed=1234, **adam):
    Vw, dw = p['Rw'].shape
    Ve, de = p['Re'].shape
    e = C.Engine(kind=C.KIND_VECTORSPACE, batch_size=B, global_batch_size=global_batch or B,
                 window_size=n, vocab_size=Vw, num_entities=Ve, word_dim=dw, entity_dim=de,
                 num_negatives=z, id_bytes=p['X'].dtype.itemsize, device=device,
                 keep_grads=keep_grads, deterministic=1, lambda_=lam,
                 lr=adam.get('lr', 1e-3), beta1=adam.get('beta1', 0.9),
                 beta2=adam.get('beta2', 0.999), eps=adam.get('eps', 1e-8), seed=seed)
    e.set_tensor(C.T_RW, p['Rw'])
    e.set_tensor(C.T_RE, p['Re'])
    e.set_tensor(C.T_W, p['W'])
    e.set_tensor(C.T_B, p['b'])
    return e


def make_ll_problem(seed, N, n, Vw, Ve, d, labels='int'):
    import scipy.sparse as sp
    rng = np.random.RandomState(seed)
    Rw = O.glorot_uniform(rng, (Vw, d))
    W = O.glorot_uniform(rng, (d, Ve))
    b = (0.1 * rng.randn(Ve)).astype(np.float32)
    X = rng.randint(0, Vw, size=(N, n)).astype(id_dtype(Vw))
    w = rng.uniform(0.5, 2.0, N).astype(np.float32)
    if labels == 'int':
        y = rng.randint(0, Ve, size=N).astype(np.int32)
        ydense = y
    else:
        rows, cols, vals = [], [], []
        for i in range(N):
            k = rng.randint(1, 4)
            idx = np.sort(rng.choice(Ve, k, replace=False))
            rows += [i] * k
            cols += list(idx)
            vals += [1.0 / k] * k
        y = sp.csr_matrix((np.array(vals, dtype=np.float32), (rows, cols)), shape=(N, Ve))
        ydense = np.asarray(y.todense(), dtype=np.float32)
    return dict(Rw=Rw, W=W, b=b, X=X, y=y, ydense=ydense, w=w, rng=rng)


def ll_engine(p, B, n, lam, device=0, keep_grads=1, global_batch=None):
    Vw, d = p['Rw'].shape
    Ve = p['W'].shape[1]
    e = C.Engine(kind=C.KIND_LOGLINEAR, batch_size=B, global_batch_size=global_batch or B,
                 window_size=n, vocab_size=Vw, num_entities=Ve, word_dim=d, entity_dim=0,
                 num_negatives=0, id_bytes=p['X'].dtype.itemsize, device=device,
                 keep_grads=keep_grads, deterministic=1, lambda_=lam,
                 lr=1.0, beta1=0.95, beta2=0.0, eps=1e-6, seed=0)
    e.set_tensor(C.T_RW, p['Rw'])
    e.set_tensor(C.T_W, p['W'])
    e.set_tensor(C.T_B, p['b'])
    return e


# --------------------------------------------------------------------------- #
# Parameters AND optimiser state against the oracle
# --------------------------------------------------------------------------- #
# Neither the loss (forward only) nor the parameters see how large a gradient is: Adam's first update is
# lr * sign(g) wherever |g| >> sqrt(eps / (1 - beta2)), m_hat / sqrt(v_hat) does not change when every step's gradient
# is scaled by one positive factor, and Adadelta's first update saturates at +-sqrt(eps / (1 - rho)).  The moments
# do: m = (1 - beta1) g, v = (1 - beta2) g^2, accu = (1 - rho) g^2 after one step from a zero state.

TENSOR_TOL = 1e-4        # parameters (and optimiser moments), relative to the tensor's max
ROW_TOL32 = 2e-4         # row-wise, against the float32 oracle (sequential fp32 sums on the oracle's side)
ROW_TOL64 = 5e-5         # row-wise, against the float64 evaluation of the same oracle
ROW_TOL32_DENSE = 1e-3   # W, b and their moments against the float32 oracle: batch-long cancelling sums on both sides

# tensor ids of a parameter and of its two optimiser moments (STATE0 = Adam m / Adadelta accu, STATE1 = v / delta)
STATE_IDS = {'R_w': (C.T_RW, C.T_STATE0_RW, C.T_STATE1_RW), 'R_e': (C.T_RE, C.T_STATE0_RE, C.T_STATE1_RE),
             'W': (C.T_W, C.T_STATE0_W, C.T_STATE1_W), 'b': (C.T_B, C.T_STATE0_B, C.T_STATE1_B)}
# the oracle's parameter order (models.py:542-543): [R_e, R_w, W, b] (vectorspace, both kinds) or [R_w, W, b]
VS_PARAMS, LL_PARAMS = ('R_e', 'R_w', 'W', 'b'), ('R_w', 'W', 'b')
SECOND_MOMENTS = ('v', 'accu', 'delta')     # sums of squares: twice the row-wise relative error of g


def state_shapes(cfg):
    """(rows, cols) of every parameter of an engine config; b as one row."""
    if cfg.kind == C.KIND_LOGLINEAR:
        return {'R_w': (cfg.vocab_size, cfg.word_dim), 'W': (cfg.word_dim, cfg.num_entities),
                'b': (1, cfg.num_entities)}
    return {'R_w': (cfg.vocab_size, cfg.word_dim), 'R_e': (cfg.num_entities, cfg.entity_dim),
            'W': (cfg.word_dim, cfg.entity_dim), 'b': (1, cfg.entity_dim)}


def engine_state(eng, kind=None):
    """Every parameter and both optimiser moments of an engine, named as oracle_state names them.  Read through
    get_tensor: each read flushes the lazy word-table rows and settles the tail first."""
    kind = eng.cfg.kind if kind is None else kind
    assert kind == eng.cfg.kind, (kind, eng.cfg.kind)
    moments = ('accu', 'delta') if kind == C.KIND_LOGLINEAR else ('m', 'v')
    out = {}
    for name, shape in state_shapes(eng.cfg).items():
        par, s0, s1 = STATE_IDS[name]
        out[name] = eng.get_tensor(par, shape)
        out[moments[0] + '.' + name] = eng.get_tensor(s0, shape)
        out[moments[1] + '.' + name] = eng.get_tensor(s1, shape)
    return out


def oracle_state(ora):
    """The same dict from an oracle object, in the oracle's dtype.  Entries are reshaped VIEWS of the oracle's arrays
    (no copies of 600 MB tables): the optimiser updates them in place, so take the dict after the last step."""
    params = ora.params()
    names = VS_PARAMS if len(params) == 4 else LL_PARAMS
    assert len(params) == len(names)
    if hasattr(ora.opt, 'accu'):
        moments = (('accu', ora.opt.accu), ('delta', ora.opt.delta))
    else:
        moments = (('m', ora.opt.m), ('v', ora.opt.v))
    out = {}
    for k, name in enumerate(names):
        shape = (1, -1) if name == 'b' else params[k].shape
        out[name] = np.asarray(params[k]).reshape(shape)
        for mname, arrs in moments:
            out[mname + '.' + name] = np.asarray(arrs[k]).reshape(shape)
    return out


def check_tensor(name, got, ref32, ref64=None, rows=None, row_tol32=ROW_TOL32, row_tol64=ROW_TOL64):
    """global + row-wise bounds for one (rows, cols) tensor; returns the figures for the log line."""
    g = rel_err(got, ref32)
    assert g < TENSOR_TOL, (name, 'rel_err', g)
    r32, at32 = row_err(got, ref32, rows)
    assert r32 < row_tol32, (name, 'row_err vs float32 oracle', r32, 'row', at32, 'tolerance', row_tol32,
                             'W, b and their moments take %g against the FLOAT32 oracle -- batch-long cancelling sums, the '
                             'oracle\'s own BLAS sum is 3.7e-4 off row-wise at C4 -- and the float64 bound (%g) does the '
                             'testing where a float64 reference is given' % (ROW_TOL32_DENSE, ROW_TOL64))
    out = '%s rel %.1e row32 %.1e' % (name, g, r32)
    if ref64 is not None:
        r64, at64 = row_err(got, ref64, rows)
        o64, _ = row_err(ref32, ref64, rows)
        assert r64 < row_tol64, (name, 'row_err vs float64 oracle', r64, 'row', at64, 'tolerance', row_tol64)
        out += ' row64 %.1e (oracle32 vs 64: %.1e)' % (r64, o64)
    return out


def state_row_tol32(name):
    """Row bound against the float32 oracle for one state entry: ROW_TOL32 for the parameters and the tables' moments,
    ROW_TOL32_DENSE for the moments of W and b, twice either for a second moment."""
    moment, _, par = name.rpartition('.')
    if not moment:
        return ROW_TOL32
    rt = ROW_TOL32_DENSE if par in ('W', 'b') else ROW_TOL32
    return 2 * rt if moment in SECOND_MOMENTS else rt


def check_state(got, ref32, ref64=None, rows=None, names=None, prefix=''):
    """Check every entry of oracle_state(...) -- parameters and both moments -- globally and row by row.
    got / ref32 / ref64: dicts of engine_state / oracle_state.  rows: {parameter name: row indices} restricts the
    row-wise maximum of that parameter and its moments (e.g. the rows a batch touches); names: a subset of the keys.
    Returns the log lines."""
    names = list(ref32) if names is None else list(names)
    missing = [k for k in names if k not in got]
    assert not missing, ('state entries not read', missing)
    log = []
    for k in names:
        sub = (rows or {}).get(k.rpartition('.')[2])
        square = k.rpartition('.')[0] in SECOND_MOMENTS
        log.append(prefix + check_tensor(k, got[k], ref32[k], None if ref64 is None else ref64[k], rows=sub,
                                         row_tol32=state_row_tol32(k), row_tol64=(2 if square else 1) * ROW_TOL64))
    return log


# --------------------------------------------------------------------------- #
# The cosine scorer: the Gaussian-data check, and problems whose ranking is known exactly
# --------------------------------------------------------------------------- #

def check_topk_against_oracle(E, Pj, idx, val, k):
    """(idx, val) of a top-k call against the float64 oracle: identical ranking except where the fp64 score gap is below
    1e-6, scores within 1e-6, k distinct entities."""
    E64, P64 = E.astype(np.float64), Pj.astype(np.float64)
    for q in range(Pj.shape[0]):
        order, sc = O.vectorspace_rank(P64[q], E64, top=k)
        full = None
        for r in np.nonzero(idx[q] != order)[0]:
            if full is None:
                full = O.vectorspace_scores(P64[q], E64)
            assert abs(full[idx[q][r]] - sc[r]) < 1e-6
        assert np.abs(val[q] - sc).max() < 1e-6
        assert len(set(idx[q].tolist())) == k


# Exact problems.  Rows have entries in {0, +-1} with exactly 1, 4 or 16 of them non-zero: the norm is 1, 2 or 4, the unit row
# has entries +-1, +-1/2 or +-1/4, every product of two entries is a multiple of 1/16 and a cosine is a sum of at most 16 of
# them, in [-1, 1] -- a multiple of 1/16 with at most 5 significant bits at every partial sum, in ANY summation order.  That is
# exact in fp32 and in bf16 (8 significant bits), so whatever GEMM, dot product or prefilter the scorer runs, it must produce
# 16 cos = <p, e> 16 / (|p| |e|) as an integer, and the ranking -- mass ties at 33 levels included -- is known from integer
# arithmetic alone.  tests/test_score_contract_cpu.py proves the claim on every shape below; it is the licence for the GPU
# tests to demand equal indices and bit-equal values with no exemption.
EXACT_NNZ = (1, 4, 16)
# (seed, V, d, Q, mix of entity rows over EXACT_NNZ) by name; the queries are an even mix
EXACT_SHAPES = {
    'tiny': (101, 50, 16, 6, (0.3, 0.3, 0.4)),
    'k_is_v': (102, 300, 16, 6, (0.3, 0.3, 0.4)),
    'unaligned_rows': (103, 4099, 20, 6, (0.3, 0.3, 0.4)),        # V % 4 = 3: every row but each fourth starts off 16 bytes
    'mid': (104, 5000, 16, 6, (0.3, 0.3, 0.4)),
    'radix_fallback': (105, 6000, 16, 6, (0.8, 0.1, 0.1)),         # most rows one-hot: thousands tied at 0 and at +-1/4
    'fused_smallest': (106, 32768, 16, 12, (0.5, 0.1, 0.4)),
    'fused_ragged': (107, 40001, 16, 12, (0.5, 0.1, 0.4)),
    'prefix': (108, 40000, 16, 12, (0.5, 0.1, 0.4)),
    'fused_dense': (110, 40001, 16, 12, (0.08, 0.02, 0.9)),        # enough entities above 1/2 for k = 1024 to keep fused rows
}


def exact_rows(rng, rows, d, mix):
    """(rows, d) int8 in {0, +-1}: exactly 1, 4 or 16 non-zeros per row (drawn with probabilities `mix`) at random places."""
    assert d >= max(EXACT_NNZ)
    nnz = rng.choice(EXACT_NNZ, size=rows, p=mix)
    places = np.argsort(rng.rand(rows, d), axis=1) < nnz[:, None]     # a row of a permutation: exactly nnz entries below nnz
    signs = rng.randint(0, 2, size=(rows, d)) * 2 - 1
    return (places * signs).astype(np.int8)


def exact_score_problem(name):
    """dict: E (V, d) / P (Q, d) float32 in {0, +-1}, and Ei / Pi the same as int8."""
    seed, V, d, Q, mix = EXACT_SHAPES[name]
    rng = np.random.RandomState(seed)
    Ei = exact_rows(rng, V, d, mix)
    Pi = exact_rows(rng, Q, d, (1 / 3.0, 1 / 3.0, 1 / 3.0))
    Pi[:3] = exact_rows(np.random.RandomState(seed + 1000), 3, d, (0, 0, 1))[:3]   # 16 non-zeros: few ties at the top
    return dict(E=Ei.astype(np.float32), P=Pi.astype(np.float32), Ei=Ei, Pi=Pi)


def exact_cos16(Pi, Ei):
    """(Q, V) int64 = 16 cos, in integer arithmetic: <p, e> * 16 / (|p| |e|), the norms 1, 2 or 4."""
    Pi, Ei = np.asarray(Pi, dtype=np.int64), np.asarray(Ei, dtype=np.int64)
    isqrt = {1: 1, 4: 2, 16: 4}
    nq = np.array([isqrt[int(n)] for n in (Pi != 0).sum(axis=1)], dtype=np.int64)
    ne = np.array([isqrt[int(n)] for n in (Ei != 0).sum(axis=1)], dtype=np.int64)
    dots = np.zeros((Pi.shape[0], Ei.shape[0]), dtype=np.int64)
    for c in range(Pi.shape[1]):                  # (an integer matmul, column by column: no BLAS for int64)
        dots += Pi[:, c, None] * Ei[None, :, c]
    den = nq[:, None] * ne[None, :]
    assert np.all((dots * 16) % den == 0)
    return dots * 16 // den


def exact_expected(c16, k=None, nan_entities=(), nan_queries=()):
    """The contract's (idx, val) for integer cosines c16 (Q, V): rank_order of every row, val = (c16 + 16) / 32 as float32.
    Entities / queries listed as NaN (zero, NaN or infinite rows: no direction) score NaN against everything."""
    cos = c16.astype(np.float32) / np.float32(16)
    cos[:, list(nan_entities)] = np.nan
    cos[list(nan_queries), :] = np.nan
    keep = cos.shape[1] if k is None else k
    idx = np.stack([O.rank_order(row, keep) for row in cos]).astype(np.int32)
    val = (np.take_along_axis(cos, idx.astype(np.int64), axis=1) + np.float32(1)) / np.float32(2)
    return idx, val


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN equal to any NaN (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def score_key(cos):
    """The scorer's 32-bit descending key of float32 cosines (csrc/common.h score_key), in numpy: ascending key = descending
    value, -0 as +0, NaN last."""
    c = np.ascontiguousarray(cos, dtype=np.float32)
    u = (c + np.float32(0)).view(np.uint32)                       # -0 + 0 = +0
    asc = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    return np.where(np.isnan(c), np.uint32(0xffffffff), ~asc).astype(np.uint32)


def threshold_bin_load(name, k):
    """Per query of an exact problem: how many entities share the 11-bit key bin of the k-th best -- what topk_rows has to
    fit into its 2048-entry candidate list."""
    p = exact_score_problem(name)
    cos = exact_cos16(p['Pi'], p['Ei']).astype(np.float32) / np.float32(16)
    out = []
    for row in cos:
        hist = np.bincount(score_key(row) >> 21, minlength=2048)
        out.append(int(hist[np.searchsorted(np.cumsum(hist), k)]))
    return out


def gaussian_score_problem(V, d, Q, seed=41):
    rng = np.random.RandomState(seed)
    return rng.randn(V, d).astype(np.float32), np.tanh(rng.randn(Q, d)).astype(np.float32)


def oracle_cosines_f32(E, P):
    """(Q, V) float32 cosines the way the oracle's float32 path computes them (unit rows, one matrix product)."""
    En = E / np.linalg.norm(E, axis=1)[:, None].astype(np.float32)
    Pn = P / np.linalg.norm(P, axis=1)[:, None].astype(np.float32)
    return (Pn @ En.T).astype(np.float32)


def count_score_collisions(cos, depth):
    """Number of rows of float32 cosines (Q, V) whose first `depth` entities (rank_order) hold two entities with one
    emitted score (cos + 1)/2 and two different cosines -- where ordering the score and ordering the cosine can part."""
    n = 0
    for row in cos:
        c = row[O.rank_order(row, depth)]
        sc = (c + np.float32(1)) / np.float32(2)
        n += int(np.any((sc[1:] == sc[:-1]) & (c[1:] != c[:-1])))
    return n
