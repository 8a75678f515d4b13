"""Entity tables that put the cosine scorer's bf16 prefilter AT its rounding-error bound -- shared by the CPU proof
(tests/test_score_bf16_inputs_cpu.py) and the GPU test (tests/test_gpu_score_bf16_bound.py).

csrc/kernels_score_bf16.h filters on bf16 copies of the unit rows and claims the fp32 ranking all the same, from
|s^ - s| <= delta = bf16_delta(d), the cut `s^_(k) - 2 delta` and the flag `s^_(k) - delta >= T + delta`.  Gaussian tables
sit at delta / 20 and bf16-exact tables at 0, so neither margin is exercised by them.  Here it is:

Building blocks.  dn(e) = 2^e (1 + 2^-8 - 2^-12) rounds DOWN to 2^e in bf16, up(e) = 2^e (1 + 2^-8 + 2^-12) rounds UP to
2^e (1 + 2^-7); the 2^-12 keeps the direction under the library's own fp32 l2_normalize_rows.  A query p carries dn values
on a dimension set A, up values on a disjoint set B and one filler F_p that makes |p| = 1.  A 'down' entity lives on A
(dn values) plus a filler F_e where p is 0: its bf16 score is LOW by s 2^-7 (15/16); an 'up' entity lives on B: HIGH by
as much.  A small component on F_p trims an entity's exact score continuously (F_e re-adjusted), the rounding pattern
untouched.  PATTERN gives nine dimensions per side with <p, e> = 0.661: with x = 1/4 + 1/16 + 1/64 the squares on the
dimensions where p = e and y = 2 x those where p = e / 2, |e|^2 = (x + y) c = 0.991 and |p|^2 = 2 (x + y / 4) c = 0.991
(c = (1 + 2^-8)^2), the vertex of the linear programme `maximise <p, e>`.  The reversal span -- how far an exact order
can be turned round in bf16 -- is then 2 s 2^-7 (15/16) = 0.0097 = 1.23 delta; no construction exceeds
sqrt(2) 2^-7 = 1.41 delta (|p_A|^2 + |p_B|^2 <= 1).

Plantings (each for 4 adversarial queries, which differ by a sign vector over A u B applied to the query and to its own
planted entities; V = 32768, the smallest table the bf16 path takes; 4 ordinary tanh(randn) queries ride in the same call):

  cut, k:   k 'down' entities with exact scores h apart, 2 k 'up' decoys just below them exactly.  In bf16 every decoy is
            above every down entity: s^_(k) is a decoy's, the bf16 top k holds decoys only, and each down entity lies
            between 1.08 delta and 2 delta - 1e-4 below s^_(k).  A cut at s^_(k) - delta, or a delta half as large, loses
            them; the cut at 2 delta keeps and re-scores them.  All at indices = 1 (mod 16), one per 64-entity group and
            query: the stride-16 sample holds background rows only.
  flag, k:  2 rs + 10 'up' decoys at SAMPLED indices (rs = 27: the rank of the sampled threshold), in different threads of
            approx_kth_rows and different groups, their bf16 scores 1e-6 apart: the sampled threshold T is one of them.
            (They lack the pattern's last dimension: the trim alone cannot take an exact score a whole delta down, the
            query's F_p is 0.09.)  k more 'up' decoys (unsampled) sit
            delta + FLAG_MARGIN .. above them in bf16 and make s^_(k); k 'down' entities (unsampled) have the k best exact
            scores and bf16 scores FLAG_MARGIN below every decoy's, so they never enter a candidate list.  delta <=
            s^_(k) - T < 2 delta: the row must be flagged -- a flag without its second delta (or with half a delta) lets
            it pass and the true top k is lost.

What no such table can have: steps of 1e-4 between the exact scores at every k.  The span above the 1.08 delta floor is
0.15 delta = 1.2e-3, and k = 100 entities 1e-4 (or 5e-5) apart span 1e-2 (5e-3).  k = 10 keeps gaps >= 5e-5; k = 100 has
8e-6, which still orders fp32 scores: an fp32 score of these rows is within 1e-6 of float64 (17 roundings of 2^-24 on
|s| <= 0.67 in exact_dot32 at d = 300, 8 more in the normalisation: 1e-6 is also the bound check_topk_against_oracle puts
on every score), so two scores 8e-6 apart cannot swap.  Likewise `flag` has to fit a whole delta between s^_(k) and T
into the span, which leaves 0.23 delta = 1.8e-3 for everything else: its hidden entities are 5e-4, not 1e-3, below the
decoys in bf16 and s^_(k) - delta 5e-4 above T (the bf16 GEMM's fp32 accumulation and the 6 dropped key bits are 5e-6
together), its decoys 1e-6 apart.

Background rows are random unit vectors with their components on A u B u F_p damped by 4 before normalisation: none
comes within 0.1 of the planted scores, nor does another query's planted entity (the sign vectors are made so)."""
import functools

import numpy as np

V = 32768
STRIDE = 16                    # kScoreStride: the sample is every 16th entity
GROUP = 64                     # entities per candidate list
EPS = 2.0 ** -12
DELTA_CONST, DELTA_PER_DIM = 0.00785, 1.2e-7          # bf16_delta(d), csrc/kernels_score_bf16.h
FLOOR = 1.08                   # every reversed entity is at least FLOOR * delta below s^_(k)
NUM_ADV = 4                    # adversarial queries per planting
NUM_ORDINARY = 4
GAP = 1e-4                     # exact score of the lowest top-k entity above the best decoy's
STEP = {10: 6e-5, 100: 8e-6}   # exact scores of neighbouring top-k entities (see above)
STEP_FLOOR = {10: 5e-5, 100: 6e-6}     # what the CPU proof asserts of them
DECOY_STEP = 1e-6              # exact scores of neighbouring decoys
FLAG_MARGIN = 5e-4             # flag: hidden s^ below every decoy's; s^_(k) - delta above every sampled decoy's
DAMP = 0.25                    # background rows on the pattern's dimensions

# (query exponent, entity exponent) of the nine dimensions of one side
PATTERN = ((-1, -1), (-2, -2), (-3, -3), (-2, -1), (-2, -1), (-3, -2), (-3, -2), (-4, -3), (-4, -3))

# name -> (d, plantings (kind, k)); the adversarial queries of planting i are rows 4 i .. 4 i + 3 of `P_adv`
CASES = {
    'cut_d64_k10': (64, (('cut', 10),)), 'cut_d64_k100': (64, (('cut', 100),)),
    'cut_d36_k10': (36, (('cut', 10),)), 'cut_d36_k100': (36, (('cut', 100),)),
    'cut_d300_k10': (300, (('cut', 10),)), 'cut_d300_k100': (300, (('cut', 100),)),
    'flag_d64': (64, (('flag', 10),)), 'flag_d300': (300, (('flag', 10),)),
    'demote_d64': (64, (('flag', 10), ('cut', 10))),
}
# The seed of each table: the first (from 1) with which no BACKGROUND coincidence sends a row of the case to the fallback
# -- nine of 8 x 512 candidate lists with more than 8 entries happen by chance at 1.2 entries a list -- as
# tests/test_score_bf16_inputs_cpu.py asserts for every row.
SEEDS = {'cut_d64_k10': 1, 'cut_d64_k100': 1, 'cut_d36_k10': 1, 'cut_d36_k100': 2, 'cut_d300_k10': 1, 'cut_d300_k100': 1,
         'flag_d64': 1, 'flag_d300': 1, 'demote_d64': 1}
CUT_CASES = [n for n in CASES if n.startswith('cut_')]
FLAG_CASES = [n for n in CASES if n.startswith('flag_')]


def delta(d):
    """bf16_delta(d) as the device computes it (fp32)."""
    return float(np.float32(DELTA_CONST) + np.float32(DELTA_PER_DIM) * np.float32(d))


def sample_rank(k):
    """rs of scorer_topk_io: the sampled threshold is (about) the rs-th best of the sample."""
    return -(-(2 * k + 400) // STRIDE)


def cand_cap(k):
    """ccap of scorer_topk_fused: candidates a row may have before it is flagged."""
    rs = sample_rank(k)
    cap = 1024
    while cap < 2 * k + 400 + 6 * 16 * int(np.ceil(np.sqrt(np.float32(rs)))) and cap < 4096:
        cap *= 2
    return cap


def group_cap(k):
    return 8 if k <= 128 else 16


def bf16(x):
    """float32 -> the float32 value of its round-to-nearest-even bf16 (to_bf16_rows; tests/test_golden_host.py)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def normalize32(X):
    """l2_normalize_rows in numpy: fp32 sum of squares, fp32 square root, fp32 division."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    nrm = np.sqrt((X * X).sum(axis=1, dtype=np.float32), dtype=np.float32)
    return (X / nrm[:, None]).astype(np.float32)


def midpoint_distance(X):
    """Per element of float32 X: distance to the nearest bf16 rounding midpoint, relative to |x| (inf for 0)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    low = (X.view(np.uint32) & 0xffff).astype(np.int64)
    ulp = np.ldexp(1.0, np.frexp(X.astype(np.float64))[1] - 24)        # 2^(e - 23) for |x| in [2^e, 2^(e+1))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(X == 0, np.inf, np.abs(low - 0x8000) * ulp / np.abs(X.astype(np.float64)))


def dn(e):
    return 2.0 ** e * (1 + 2.0 ** -8 - EPS)


def up(e):
    return 2.0 ** e * (1 + 2.0 ** -8 + EPS)


class Layout(object):
    """Which dimensions of a d-dimensional row hold the pattern: 20 of them spread evenly over the row (d = 300: over all
    five 64-wide K chunks of kp = 320), alternately A and B, then F_p and F_e; the pattern's magnitudes in a drawn order."""

    def __init__(self, d, rng):
        pos = np.unique(np.round(np.linspace(0, d - 1, 2 * len(PATTERN) + 2)).astype(np.int64))
        assert len(pos) == 2 * len(PATTERN) + 2, d
        self.d = d
        self.A, self.B, self.FP, self.FE = pos[0:-2:2], pos[1:-2:2], int(pos[-2]), int(pos[-1])
        self.support = np.concatenate([self.A, self.B, [self.FP]])        # where a query is not 0
        self.order = {'down': rng.permutation(len(PATTERN)), 'up': rng.permutation(len(PATTERN))}

    def dims(self, kind):
        return self.A if kind == 'down' else self.B

    def magnitudes(self, kind, who):
        f = dn if kind == 'down' else up
        return np.array([f(PATTERN[i][who]) for i in self.order[kind]])

    def query(self, sign):
        """(d,) float32, unit norm after normalize32, every component at least 2^-13 from a rounding midpoint."""
        fill = 1.0
        for _ in range(64):
            p = np.zeros(self.d)
            for kind in ('down', 'up'):
                p[self.dims(kind)] = self.magnitudes(kind, 0)
            rest = 1.0 - float((p * p).sum())
            assert rest > 0.004, rest
            p[self.FP] = np.sqrt(rest) * fill
            p32 = normalize32((p * sign)[None, :])[0]
            if midpoint_distance(p32).min() >= 2.0 ** -13:
                return p32
            fill *= 1 + 2.0 ** -9
        raise AssertionError('no filler keeps the query off the rounding midpoints')

    def entities(self, kind, sign, trim, short=False):
        """(len(trim), d) float32 'down' / 'up' entities with the component `trim` on F_p.  short: without the last
        dimension of PATTERN (exact score 2^-7 lower: what the F_p component, 0.09 in the query, could only give with a
        trim that leaves no room for F_e)."""
        trim = np.asarray(trim, dtype=np.float64)
        e = np.zeros((len(trim), self.d))
        e[:, self.dims(kind)] = self.magnitudes(kind, 1) * (self.order[kind] != len(PATTERN) - 1 if short else 1.0)
        e[:, self.FP] = trim
        rest = 1.0 - (e * e).sum(axis=1)
        assert rest.min() > 0.004, rest.min()
        e[:, self.FE] = np.sqrt(rest)
        return normalize32(e * sign[None, :])

    def entities_scoring(self, kind, sign, p32, targets, short=False):
        """Entities of a kind whose exact (float64, after fp32 normalisation) scores against p32 are `targets` to ~1e-8,
        every component that meets a non-zero of the query at least 2^-13 from a rounding midpoint."""
        targets = np.array(targets, dtype=np.float64)
        p64 = p32.astype(np.float64)
        trim = np.zeros(len(targets))
        for _ in range(64):
            for _ in range(3):            # (the score is linear in the trim up to the change of the norm)
                got = self.entities(kind, sign, trim, short).astype(np.float64) @ p64
                trim += (targets - got) / p64[self.FP]
            rows = self.entities(kind, sign, trim, short)
            bad = midpoint_distance(rows[:, self.support]).min(axis=1) < 2.0 ** -13
            if not bad.any():
                return rows
            targets[bad] += 3e-7          # moves the trim by ~2^-12 of itself
        raise AssertionError('no trim keeps the rows off the rounding midpoints')


def scores(P32, E32):
    """(exact, approximate): float64 products of the fp32-normalised rows and of their bf16 images."""
    s = P32.astype(np.float64) @ E32.astype(np.float64).T
    sh = bf16(P32).astype(np.float64) @ bf16(E32).astype(np.float64).T
    return s, sh


class Slots(object):
    """Hands out table rows: unsampled ones (index = 1 mod 16, one per group and query) and sampled ones whose sample
    positions fall into different threads of approx_kth_rows (thread = (position / 4) mod 256, i.e. the group mod 256),
    are distinct mod 256 and lie in different groups."""

    def __init__(self, rng):
        self.rng = rng
        self.used = set()
        self.sampled_residues = list(rng.permutation(256))

    def unsampled(self, q, n, avoid_groups=()):
        out, groups = [], set(avoid_groups)
        for g in self.rng.permutation(V // GROUP):
            idx = int(g) * GROUP + 1 + STRIDE * (q % 4)
            if idx in self.used or int(g) in groups:
                continue
            self.used.add(idx)
            groups.add(int(g))
            out.append(idx)
            if len(out) == n:
                return np.array(out), groups
        raise AssertionError('table too small for the planted rows')

    def sampled(self, n):
        res = [int(self.sampled_residues.pop()) for _ in range(n)]
        groups = [r + 256 * int(self.rng.randint(0, 2)) for r in res]
        idx = [g * GROUP + STRIDE * ((g >> 6) & 3) for g in groups]
        assert not self.used.intersection(idx)
        self.used.update(idx)
        return np.array(idx), set(groups)


def _draw_signs(lay, rng, n):
    """n sign vectors over A u B (1 elsewhere).  Up to 4: every query scores BELOW -0.02 (untrimmed) against every other
    query's planted entities, so those never reach a sampled threshold and no candidate list fills with them (k = 100
    plants 1200 rows in 512 groups).  Up to 8 (k = 10 only: 400 planted rows): at most 0.42."""
    signs = np.ones((n, lay.d))
    if n <= 4:
        for kind in ('down', 'up'):
            prod = lay.magnitudes(kind, 0) * lay.magnitudes(kind, 1)
            sg = rng.randint(0, 2, size=(20000, n, len(PATTERN))) * 2 - 1
            cross = np.einsum('bqi,bri,i->bqr', sg, sg, prod)
            worst = (cross - 10.0 * np.eye(n)).max(axis=(1, 2))
            assert worst.min() <= -0.02, worst.min()
            signs[:, lay.dims(kind)] = sg[int(np.argmax(worst <= -0.02))]
        return signs
    # On a side, the products p_i e_i are 1/4, 1/8, 1/8 (PATTERN rows 0, 3, 4) and six more that sum to 0.156.  Queries
    # of different classes differ in more than a common sign on the big three: at most 1/4 + 0.156 between them.  The
    # two queries of one class agree there and are opposite on the other six: 1/2 - 0.156.
    assert n <= 8
    classes = np.array([(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1)])
    for kind in ('down', 'up'):
        big = np.isin(lay.order[kind], (0, 3, 4))
        rest = rng.randint(0, 2, size=(4, len(PATTERN))) * 2 - 1
        for q in range(n):
            sg = rest[q % 4] * (1 if q < 4 else -1)
            sg[big] = classes[q % 4]
            signs[q, lay.dims(kind)] = sg * (rng.randint(0, 2) * 2 - 1)
        prod = lay.magnitudes(kind, 0) * lay.magnitudes(kind, 1)
        sg = signs[:, lay.dims(kind)]
        cross = np.abs((sg[:, None, :] * sg[None, :, :] * prod).sum(axis=2))
        assert (cross - np.diag(np.diag(cross))).max() <= 0.42, cross
    return signs


def _plant(lay, slots, kind, k, q, sign, p32):
    """The planted rows of one adversarial query: dict(rows (n, d), index (n,), top (k,) table indices best first,
    decoys, sampled (flag: the decoys the sample sees))."""
    base = {}
    for ek in ('down', 'up'):
        s, sh = scores(p32[None, :], lay.entities(ek, sign, [0.0]))
        base[ek] = (float(s[0, 0]), float(sh[0, 0] - s[0, 0]))        # exact score untrimmed, bf16 error
    dlt = delta(lay.d)
    span = base['up'][1] - base['down'][1]
    h = STEP[k]
    s_top = base['down'][0] - 2e-5
    top_scores = s_top - h * np.arange(k)
    decoy_best = top_scores[-1] - GAP
    if kind == 'cut':
        floor = span - (k - 1) * (h + DECOY_STEP) - GAP
        assert floor >= FLOOR * dlt + 2e-5, ('the pattern does not reach the floor', span / dlt, floor / dlt)
        decoy_scores = decoy_best - DECOY_STEP * np.arange(2 * k)
        n_sampled = 0
    else:
        # bf16: hidden (top) < sampled decoys < unsampled decoys, exact: all decoys < hidden
        n_sampled = 2 * sample_rank(k) + 10
        t_min = top_scores[0] + base['down'][1] + FLAG_MARGIN                 # approximate score of the lowest sampled decoy
        t_max = t_min + DECOY_STEP * (n_sampled - 1)
        sk = decoy_best - DECOY_STEP * (k - 1) + base['up'][1]                 # approximate score of the k-th unsampled decoy
        assert sk - dlt >= t_max + FLAG_MARGIN, ('the pattern leaves no room for the flag case', span / dlt)
        decoy_scores = decoy_best - DECOY_STEP * np.arange(k)
        s, sh = scores(p32[None, :], lay.entities('up', sign, [0.0], short=True))
        sampled_scores = t_max - float(sh[0, 0] - s[0, 0]) - DECOY_STEP * np.arange(n_sampled)
    rows = [lay.entities_scoring('down', sign, p32, top_scores), lay.entities_scoring('up', sign, p32, decoy_scores)]
    if n_sampled:
        rows.append(lay.entities_scoring('up', sign, p32, sampled_scores, short=True))
    rows = np.concatenate(rows)
    n_unsampled = len(rows) - n_sampled
    samp_idx, samp_groups = slots.sampled(n_sampled) if n_sampled else (np.zeros(0, np.int64), set())
    uns_idx, _ = slots.unsampled(q, n_unsampled, avoid_groups=samp_groups)
    index = np.concatenate([uns_idx, samp_idx])
    return dict(kind=kind, k=k, rows=rows, index=index, top=index[:k], decoys=index[k:], sampled=samp_idx)


@functools.lru_cache(maxsize=None)
def build(name):
    """dict: E (V, d) float32 table, P_adv (4 per planting, d), P_ord (4, d), plant: per adversarial query its _plant dict
    (plus 'query': its row of P_adv), d.  Deterministic; callers must not modify the arrays."""
    d, plantings = CASES[name]
    rng = np.random.RandomState(SEEDS[name])
    lay = Layout(d, rng)
    E = rng.randn(V, d)
    E[:, lay.support] *= DAMP
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    signs = _draw_signs(lay, rng, NUM_ADV * len(plantings))
    slots = Slots(rng)
    P_adv, plant = [], []
    for i, (kind, k) in enumerate(plantings):
        for j in range(NUM_ADV):
            q = NUM_ADV * i + j
            p32 = lay.query(signs[q])
            pl = _plant(lay, slots, kind, k, q, signs[q], p32)
            pl['query'] = q
            E[pl['index']] = pl['rows']
            P_adv.append(p32)
            plant.append(pl)
    P_ord = np.tanh(rng.randn(NUM_ORDINARY, d)).astype(np.float32)
    E.setflags(write=False)
    return dict(name=name, d=d, E=E, P_adv=np.stack(P_adv), P_ord=P_ord, plant=plant, layout=lay)


def queries(case, planting=0):
    """(8, d): the 4 adversarial queries of one planting, then the 4 ordinary ones -- one call of the GPU test."""
    return np.concatenate([case['P_adv'][NUM_ADV * planting:NUM_ADV * (planting + 1)], case['P_ord']])


@functools.lru_cache(maxsize=None)
def model(name):
    """(exact, approximate) scores (Q_adv + 4, V) of every query of a case against its table AS THE LIBRARY HOLDS IT:
    float64 products of the fp32-normalised rows, and of their bf16 images."""
    case = build(name)
    P = normalize32(np.concatenate([case['P_adv'], case['P_ord']]))
    return scores(P, normalize32(case['E']))
