"""Problems whose only difficulty is HOW OFTEN every word occurs in a batch -- shared by the CPU proof of the inputs
(test_wgrad_inputs_cpu.py) and the GPU test (test_gpu_wgrad_cases.py).

dR_w, the word-table gradient, and dZu, the loglinear per-distinct-word sums of dJ, are formed without atomics by an order-fixed
tree over each word's occurrences (csrc/word_index.h; kernels in csrc/kernels_seg.h; dispatch in word_grad_segsum and dzu_from_dj
of csrc/host/lazy_segsum.inc):

  tree    a word's occurrences are cut into ITEMS of at most 64 entries; a word of more than 64 occurrences leaves one partial row
          per item, summed again at the next level (64^2 occurrences: three levels, 64^3: four).  Level 0 of a vectorspace index
          is sorted by item length and a one-entry item takes its row from the descriptor.  An item is walked in trips of 8, then
          4, then 1-3 entries by a lane group of 32 lanes (d_w / 4 <= 32, or rows that 32-lane column groups cover better), 64
          lanes, or one wave per 64 scalar columns (d_w % 4 != 0); the 32-lane form starts a second trip over the row numbers at
          entry 33.  Levels 1 and 2 of a three-level tree run as one launch (segsum_upper_fused) while no word has more than 32
          level-1 chunk items (131 072 occurrences).
  dense   (d_w % 4 == 0, d_w <= 512; by default where the tree runs its 32-lane forms, SERT_DENSE_HEAVY=0 / 1 forces it) the up
          to 16 words of MORE than 4096 occurrences leave the tree when together they hold at least 1/8 of the batch's tokens:
          count-weighted sums over all batch rows by extra workgroups of the tree's launches (segsum_rows_plus: the stream beside
          level 0 over row blocks of 64, 128 or 256 batch rows, the combine beside level 1 or alone), or -- 64-lane row widths
          under SERT_DENSE_HEAVY=1 -- by two launches in front of the tree.
  dzu     the loglinear model: the same tree over V_e-wide rows, the dense words flagged and skipped (they stay in the tree, so
          a batch with a dense word always has three levels and the combine always rides level 1: dzu_from_dj cannot reach its
          "combine alone" launch), segsum_rows_plus_ll beside levels 0 and 1; V_e % 4 != 0: segsum_rows_scalar<true, true>, which
          also carries the per-word sums of r through its rpart chain.

A case is a COUNT PER WORD for each of its two steps, placed at seeded random positions.  Step 2 is another plan: the words that
are heavy or multi-chunk in step 1 are absent in step 2 and the other way round, the singletons move from the low end of the
vocabulary to the high end (word 0 and word V_w - 1 are each present in one step and absent in the other), so nothing of step
1's partial rows, dense partials or gradient rows may survive into step 2.  Everything else is tame, as util.make_vs_problem /
make_ll_problem make it: Glorot parameters, weights in [0.5, 2], lambda = 0.01, small V_e, z and d_e.

Each case states the plan Engine.wgrad_plan() (sert_debug_wgrad_plan) must report for either step.  EVENTS is the one list of
structures the cases have to produce between them; events_of() finds the ones a step produces from its counts, the constants
64, 4096, 16, 32 and 1/8 quoted from word_index.h, and the stated plan alone."""
import numpy as np

from oracle import sert_oracle as O
from tests import util as U

SEG = 64              # csrc/word_index.h: kSegChunk
HEAVY_MIN = 4096      # kHeavyMinCount (a strict >)
HEAVY_MAX = 16        # kHeavyMax
FUSED_MAX = 32        # kFusedMaxChunks
LAM, STEPS = 0.01, 2
VS_Z, VS_VE, VS_DE = 2, 20, 8     # vectorspace: negatives, entities, entity dimension -- not what these cases are about
LL_D = 8                          # loglinear: word dimension

LENS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 31, 32, 33, 36, 63, 64, 65, 128, 129, 4096)

VS_EVENTS = tuple('count%d_lanes%d' % (k, lanes) for lanes in (32, 64) for k in LENS) + (
    'tree_1_level', 'tree_2_levels', 'upper_fused_2_chunk_items', 'upper_fused_32_chunk_items', 'level2_launch_33_chunk_items',
    'tree_4_levels',
    'count4096_in_tree_beside_dense', 'count4097_dense', 'heavy_under_eighth_in_tree', 'dense16', 'heavy17_lightest_in_tree_combine_alone',
    'dense_no_level1_combine_alone', 'row_of_one_dense_word',
    'heavy_rows64', 'heavy_rows128', 'heavy_rows256', 'dense_B_not_multiple_of_16', 'dense_B_not_multiple_of_64',
    'dense_B_not_multiple_of_256',
    'dw4', 'dw128', 'dw132', 'dw200_default_tree', 'dw200_two_launches', 'dw256_default_tree', 'dw256_two_launches', 'dw260', 'dw300',
    'dw388', 'dw516_dense_off', 'dw6_scalar', 'dw70_scalar_upper_levels',
    'id1', 'id2', 'id4', 'word0_present', 'word0_absent', 'last_word_present', 'last_word_absent',
)
LL_EVENTS = (
    'll_ve24_no_dense', 'll_ve24_dense_level1', 'll_ve260_two_groups_ragged', 'll_ve260_dense', 'll_ve23_scalar', 'll_ve75_scalar_two_groups',
    'll_scalar_count65', 'll_scalar_count4097', 'll_word0_present', 'll_word0_absent', 'll_last_word_present', 'll_last_word_absent',
)
EVENTS = VS_EVENTS + LL_EVENTS


def P(levels, launches, dense=0, heavy='none', rows=0, blocks=0, alone=False, sorted0=True, path='word_grad'):
    """A stated plan, as Engine.wgrad_plan() reports it."""
    return {'path': path, 'levels': levels, 'launches': list(launches), 'dense_cnt': dense, 'heavy': heavy, 'heavy_rows': rows,
            'heavy_blocks': blocks, 'combine_alone': alone, 'slot_is_row': sorted0}


def PL(levels, launches, **kw):
    return P(levels, launches, sorted0=False, path='dzu', **kw)


# counts: per step ([(count, how many words)], count of the filler words).  The named words take ids from the middle of the
# vocabulary (step 0 upwards from V_w / 3, step 1 upwards from 2 V_w / 3), the fillers the lowest (step 0) or highest (step 1) ids.
_SHORT = [(k, 1) for k in LENS if k <= SEG]
_LENS0 = _SHORT + [(65, 1), (128, 1), (129, 1), (4096, 1)]               # 4772 tokens
_LENS1 = _SHORT + [(65, 1), (128, 1), (129, 1), (4096, 1), (4097, 1)]    # 8869 tokens
_W0 = [(4300, 1)]                        # one word above 4096, a hundred singletons
_W1 = [(65, 1), (129, 1), (33, 1), (3, 1)]
_WB = dict(B=1100, n=4, Vw=800)          # 4400 tokens


def _widths(dw, plan0, plan1, knob=None):
    return dict(kind='vs', dw=dw, knob=knob, counts=[(_W0, 1), (_W1, 7)], plan=[plan0, plan1], **_WB)


VS_CASES = {
    # every item length under the 32-lane form; step 1 adds a word of 4097 (dense) beside the one of 4096 (in the tree);
    # B = 1999: no multiple of 16
    'lens_d128': dict(kind='vs', B=1999, n=5, Vw=6000, dw=128, knob=None, counts=[(_LENS0, 1), (_LENS1, 1)],
                      plan=[P(2, [('rows32', 1)] * 2),
                            P(2, [('rows_plus', 1)] * 2, dense=1, heavy='fused', rows=64, blocks=32)]),
    # ... under the 64-lane form, the product default at d_w = 256: the word of 4097 in a three-level tree through upper_fused
    'lens_d256': dict(kind='vs', B=1999, n=5, Vw=6000, dw=256, knob=None, counts=[(_LENS0, 1), (_LENS1, 1)],
                      plan=[P(2, [('rows64', 1)] * 2), P(3, [('rows64', 1), ('upper_fused', 2)])]),
    # ... and with SERT_DENSE_HEAVY=1: segsum_heavy + segsum_heavy_combine in front of segsum_rows<64>
    'lens_d256_dense': dict(kind='vs', B=1999, n=5, Vw=6000, dw=256, knob='1', counts=[(_LENS0, 1), (_LENS1, 1)],
                            plan=[P(2, [('rows64', 1)] * 2),
                                  P(2, [('rows64', 1)] * 2, dense=1, heavy='two_launches', rows=256, blocks=8)]),
    'w_d200': _widths(200, P(3, [('rows64', 1), ('upper_fused', 2)]), P(2, [('rows64', 1)] * 2)),
    'w_d200_dense': _widths(200, P(1, [('rows64', 1)], dense=1, heavy='two_launches', rows=256, blocks=5), P(2, [('rows64', 1)] * 2), knob='1'),
    'w_d260': _widths(260, P(1, [('rows_plus', 3)], dense=1, heavy='fused', rows=64, blocks=18, alone=True), P(2, [('rows32', 3)] * 2)),
    'w_d300': _widths(300, P(1, [('rows_plus', 3)], dense=1, heavy='fused', rows=64, blocks=18, alone=True), P(2, [('rows32', 3)] * 2)),
    'w_d388': _widths(388, P(3, [('rows64', 2), ('upper_fused', 4)]), P(2, [('rows64', 2)] * 2)),
    # above 512 columns the dense pass is off: the heavy word in a three-level tree of 32-lane groups, five column groups
    'w_d516': _widths(516, P(3, [('rows32', 5), ('upper_fused', 5)]), P(2, [('rows32', 5)] * 2)),
    'w_d6': _widths(6, P(3, [('scalar', 1)] * 3), P(2, [('scalar', 1)] * 2)),
    'w_d70': _widths(70, P(3, [('scalar', 2)] * 3), P(2, [('scalar', 2)] * 2)),
    # a four-level tree (262 145 = 64^3 + 1 occurrences) at the product default of d_w = 132; step 1: 64^3 exactly, three levels
    # with 64 level-1 chunk items (above kFusedMaxChunks: three launches)
    'four_levels_d132': dict(kind='vs', B=33000, n=8, Vw=2500, dw=132, knob=None, counts=[([(262145, 1)], 1), ([(262144, 1)], 1)],
                             plan=[P(4, [('rows64', 1)] * 4), P(3, [('rows64', 1)] * 3)]),
    # exactly 32 level-1 chunk items (131 072 occurrences): upper_fused; 33 (131 073): the separate level-2 launch.  The tree
    # alone (SERT_DENSE_HEAVY=0), at d_w = 8
    'upper_bounds_d8': dict(kind='vs', B=33000, n=4, Vw=1200, dw=8, knob='0', counts=[([(131072, 1)], 1), ([(131073, 1)], 1)],
                            plan=[P(3, [('rows32', 1), ('upper_fused', 1)]), P(3, [('rows32', 1)] * 3)]),
    # row blocks of 128 batch rows; six dense words and no word above 64 beside them: no level 1, the combine alone.  n = 1,
    # one-byte ids; step 1: no heavy word
    'rows128_d4': dict(kind='vs', B=32808, n=1, Vw=250, dw=4, knob=None, counts=[([(5000, 6)], 40), ([(3, 1)], 200)],
                       plan=[P(1, [('rows_plus', 1)], dense=6, heavy='fused', rows=128, blocks=257, alone=True), P(2, [('rows32', 1)] * 2)]),
    # row blocks of 256; exactly 16 dense words, one batch row all of one dense word (count byte = n); step 1: 17 heavy words,
    # the lightest (4097) stays in a three-level tree beside rows_plus and upper_fused, the combine alone.  Four-byte ids
    'rows256_d8': dict(kind='vs', B=65536, n=2, Vw=70000, dw=8, knob=None, full_row=True,
                       counts=[([(6000, 16)], 1), ([(7000, 16), (4097, 1)], 1)],
                       plan=[P(1, [('rows_plus', 1)], dense=16, heavy='fused', rows=256, blocks=256, alone=True),
                             P(3, [('rows_plus', 1), ('upper_fused', 1)], dense=16, heavy='fused', rows=256, blocks=256, alone=True)]),
    # a heavy word that holds under 1/8 of the tokens (8 x 4097 < 33000) stays in the tree; step 1: two of them hold 1/8
    'eighth_d4': dict(kind='vs', B=16500, n=2, Vw=1000, dw=4, knob=None, counts=[([(4097, 1)], 50), ([(4097, 2)], 50)],
                      plan=[P(3, [('rows32', 1), ('upper_fused', 1)]),
                            P(1, [('rows_plus', 1)], dense=2, heavy='fused', rows=64, blocks=258, alone=True)]),
}

_LB = dict(B=1100, n=4, Vw=800)
_LL0 = [(4096, 1), (65, 1), (129, 1), (33, 1), (3, 1)]      # no dense word: 4096 is not above the threshold
_LL1 = [(4097, 1), (65, 1), (5, 1)]
_LLD = dict(dense=1, heavy='fused', rows=64, blocks=18)
LL_CASES = {
    'll_v24': dict(kind='ll', Ve=24, counts=[(_LL0, 1), (_LL1, 1)],
                   plan=[PL(2, [('rows64', 1)] * 2), PL(3, [('rows_plus_ll', 1)] * 2 + [('rows64', 1)], **_LLD)], **_LB),
    # 65 float4 columns: two 64-lane column groups, the second of one lane
    'll_v260': dict(kind='ll', Ve=260, counts=[(_LL1, 1), (_LL0, 1)],
                    plan=[PL(3, [('rows_plus_ll', 2)] * 2 + [('rows64', 2)], **_LLD), PL(2, [('rows64', 2)] * 2)], **_LB),
    'll_v23': dict(kind='ll', Ve=23, counts=[(_LL1, 1), (_LL0, 1)],
                   plan=[PL(3, [('scalar_ll', 1)] * 3), PL(2, [('scalar_ll', 1)] * 2)], **_LB),
    'll_v75': dict(kind='ll', Ve=75, counts=[(_LL0, 1), (_LL1, 1)],
                   plan=[PL(2, [('scalar_ll', 2)] * 2), PL(3, [('scalar_ll', 2)] * 3)], **_LB),
}

CASES = dict(VS_CASES)
CASES.update(LL_CASES)
SEEDS = {name: 500 + k for k, name in enumerate(CASES)}


def is_ll(name):
    return CASES[name]['kind'] == 'll'


def dense_cases():
    """The vectorspace cases one of whose steps has a dense word: they also run with SERT_DENSE_HEAVY=0."""
    return [name for name, c in VS_CASES.items() if any(p['dense_cnt'] > 0 for p in c['plan'])]


def stated_counts(c, step):
    """counts (V_w) of a case's step, from its count plan."""
    T, Vw = c['B'] * c['n'], c['Vw']
    named, fill = c['counts'][step]
    out = np.zeros(Vw, dtype=np.int64)
    w = (Vw // 3) * (step + 1)
    reserved = []
    for s in range(STEPS):          # the named words of EITHER step are no filler of any
        w0 = (Vw // 3) * (s + 1)
        reserved.append((w0, w0 + sum(k for _, k in c['counts'][s][0])))
    for count, k in named:
        out[w:w + k] = count
        w += k
    assert w <= (Vw // 3) * (step + 2) and w <= Vw - 1, (w, Vw)
    rest = T - int(out.sum())
    assert rest > 0, rest
    free = np.array([v for v in range(Vw) if not any(lo <= v < hi for lo, hi in reserved)], dtype=np.int64)
    nfill = -(-rest // fill)
    assert nfill < len(free), (nfill, len(free))        # (the far end of the vocabulary stays absent)
    ids = free[:nfill] if step == 0 else free[::-1][:nfill]
    out[ids] = fill
    out[ids[-1]] -= nfill * fill - rest
    assert int(out.sum()) == T and out.min() >= 0
    return out


_cache = {}


def case_problem(name):
    """(case dict, problem) of a case, built once per process; treat both as read-only.  problem: the dict of
    util.make_vs_problem / make_ll_problem over STEPS batches with X (STEPS * B, n) from the case's count plans; vectorspace:
    neg = [neg of step 0, neg of step 1]."""
    if name not in _cache:
        c = CASES[name]
        B, n, Vw = c['B'], c['n'], c['Vw']
        if c['kind'] == 'vs':
            p = U.make_vs_problem(SEEDS[name], B * STEPS, n, VS_Z, Vw, VS_VE, c['dw'], VS_DE)
        else:
            p = U.make_ll_problem(SEEDS[name], B * STEPS, n, Vw, c['Ve'], LL_D, 'int')
        rng = np.random.RandomState(SEEDS[name] + 1000)
        X = np.empty((STEPS, B * n), dtype=p['X'].dtype)
        for s in range(STEPS):
            counts = stated_counts(c, s)
            flat = np.repeat(np.arange(Vw), counts)[rng.permutation(B * n)]
            if c.get('full_row'):        # one batch row all of the heaviest word: swap its first n occurrences into row 0
                w = int(np.argmax(counts))
                at = np.nonzero(flat[n:] == w)[0][:n] + n
                flat[at] = flat[:n].copy()
                flat[:n] = w
            X[s] = flat
        p['X'] = X.reshape(STEPS * B, n)
        if c['kind'] == 'vs':
            p['neg'] = [rng.randint(0, VS_VE, size=(B, VS_Z)).astype(np.int64) for _ in range(STEPS)]
        for a in list(p.values()) + p.get('neg', []):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, p)
    return _cache[name]


def step_tokens(name, step):
    """X (B, n) of a step."""
    c, p = case_problem(name)
    return p['X'][step * c['B']:(step + 1) * c['B']]


def step_counts(name, step):
    c, _ = case_problem(name)
    return np.bincount(step_tokens(name, step).ravel().astype(np.int64), minlength=c['Vw'])


_refs = {}


def case_reference(name, dtype):
    """The oracle's run of a case in `dtype`, computed once per process and shared: ([gradients of step 0, of step 1] in the
    oracle's parameter order, the oracle after the last step)."""
    key = (name, np.dtype(dtype).name)
    if key not in _refs:
        c, p = case_problem(name)
        B = c['B']
        if c['kind'] == 'vs':
            ora = O.VectorSpaceOracle(B, c['n'], VS_Z, p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dtype)
        else:
            ora = O.LogLinearOracle(B, c['n'], p['Rw'], p['W'], p['b'], LAM, dtype=dtype)
        grads = []
        for s in range(STEPS):
            sl = slice(s * B, (s + 1) * B)
            if c['kind'] == 'vs':
                _, g, _ = ora.loss_and_grads(p['X'][sl], p['y'][sl], p['w'][sl], p['neg'][s])
            else:
                _, g, _ = ora.loss_and_grads(p['X'][sl], p['ydense'][sl], p['w'][sl])
            kept = [np.array(a) for a in g]
            for a in kept:
                a.setflags(write=False)
            grads.append(kept)
            ora.opt.update(ora.params(), g)
        _refs[key] = (grads, ora)
    return _refs[key]


def word_grad(name, grads):
    """dR_w (V_w, d) of one step's gradients as case_reference returns them."""
    return grads[0] if is_ll(name) else grads[1]


# --------------------------------------------------------------------------------------------------------------------- #
# what the dispatch makes of a step's counts
# --------------------------------------------------------------------------------------------------------------------- #

def lanes32(dw):
    """api_data_train.inc / lazy_segsum.inc: the tree runs its 32-lane forms."""
    d4 = dw // 4
    return dw % 4 == 0 and (d4 <= 32 or (d4 > 64 and 64 * -(-d4 // 64) > 32 * -(-d4 // 32)))


def dense_enabled(c):
    """sert_upload_dataset: the dense pass of a vectorspace model is built."""
    if c['dw'] % 4 != 0 or c['dw'] > 512 or c['n'] > 255:
        return False
    return lanes32(c['dw']) if c['knob'] is None else c['knob'] != '0'


def dense_words(counts, T, enabled=True):
    """build_word_index: the (at most 16) words above 4096 occurrences, heaviest first (ties: lowest id), if they hold 1/8 of
    the T tokens."""
    counts = np.asarray(counts, dtype=np.int64)
    heavy = [int(w) for w in np.argsort(-counts, kind='stable') if counts[w] > HEAVY_MIN][:HEAVY_MAX]
    if not enabled or not heavy or int(counts[heavy].sum()) * 8 < T:
        return []
    return heavy


def tree_shape(counts):
    """(levels, [items per level], largest number of level-1 chunk items of one word) of the tree over words with these counts."""
    lens = [int(k) for k in counts if k > 0]
    items, most_l1_chunks, level = [], 0, 0
    while lens:
        nxt = []
        n_items = 0
        for k in lens:
            if k <= SEG:
                n_items += 1
            else:
                chunks = -(-k // SEG)
                n_items += chunks
                nxt.append(chunks)
                if level == 1:
                    most_l1_chunks = max(most_l1_chunks, chunks)
        items.append(n_items)
        lens = nxt
        level += 1
    return level, items, most_l1_chunks


def heavy_rows(B):
    """kernels_seg.h: heavy_rows_fused."""
    r = 64
    while r < 256 and B // (2 * r) >= 256:
        r *= 2
    return r


def plan_from_dispatch(c, counts):
    """The plan lazy_segsum.inc makes of a step's counts, restated (the CPU proof holds the stated plans against it and against
    the index sert_debug_word_index_sum builds; the GPU test against what the engine reports)."""
    counts = np.asarray(counts, dtype=np.int64)
    B, T = c['B'], c['B'] * c['n']
    if c['kind'] == 'll':
        V = c['Ve']
        dense = dense_words(counts, T, V % 4 == 0)
        levels, _, _ = tree_shape(counts)                  # (the dense words stay in the tree, flagged)
        if V % 4 != 0:
            return PL(levels, [('scalar_ll', -(-V // 64))] * levels)
        gy = -(-(V // 4) // 64)
        if not dense:
            return PL(levels, [('rows64', gy)] * levels)
        launches = [('rows_plus_ll' if l <= 1 else 'rows64', gy) for l in range(levels)]
        return PL(levels, launches, dense=len(dense), heavy='fused', rows=heavy_rows(B), blocks=-(-B // heavy_rows(B)), alone=levels < 2)
    dw = c['dw']
    dense = dense_words(counts, T, dense_enabled(c))
    tree = counts.copy()
    tree[dense] = 0
    levels, _, most = tree_shape(tree)
    d4 = dw // 4
    if dw % 4 != 0:
        return P(levels, [('scalar', -(-dw // 64))] * levels)
    l32 = lanes32(dw)
    form = ('rows32', 1 if d4 <= 32 else -(-d4 // 32)) if l32 else ('rows64', -(-d4 // 64))
    fused_upper = levels == 3 and most <= FUSED_MAX
    fused_heavy = bool(dense) and l32 and levels >= 1
    launches = []
    for l in range(levels):
        if fused_upper and l == 1:
            launches.append(('upper_fused', -(-d4 // 32)))
            break
        launches.append(('rows_plus', -(-d4 // 32)) if fused_heavy and l <= 1 else form)
    kw = {}
    if dense and fused_heavy:
        kw = dict(dense=len(dense), heavy='fused', rows=heavy_rows(B), blocks=-(-B // heavy_rows(B)),
                  alone=not any(f == 'rows_plus' for f, _ in launches[1:]))
    elif dense:
        kw = dict(dense=len(dense), heavy='two_launches', rows=256, blocks=-(-B // 256))
    return P(levels, launches, **kw)


# --------------------------------------------------------------------------------------------------------------------- #
# the events a step produces
# --------------------------------------------------------------------------------------------------------------------- #

def events_of(name, step, plan=None):
    """The EVENTS step `step` of a case produces -- from its counts (and, for the row of one dense word, its tokens), the
    constants above and the plan: the stated one, or the reported one in its place."""
    c, _ = case_problem(name)
    plan = c['plan'][step] if plan is None else plan
    counts = step_counts(name, step)
    B, T, Vw = c['B'], c['B'] * c['n'], c['Vw']
    forms = [f for f, _ in plan['launches']]
    ev = set()

    def put(ev_name, cond):
        if bool(np.any(cond)):
            ev.add(ev_name)

    heavy = np.nonzero(counts > HEAVY_MIN)[0]
    heavy = heavy[np.argsort(-counts[heavy], kind='stable')]
    ndense = plan['dense_cnt']
    dense = heavy[:ndense]
    tree = counts.copy()
    tree[dense] = 0
    present = counts > 0
    if c['kind'] == 'll':
        V = c['Ve']
        scalar = forms and all(f == 'scalar_ll' for f in forms)
        put('ll_ve24_no_dense', V == 24 and ndense == 0 and forms == ['rows64'] * plan['levels'])
        put('ll_ve24_dense_level1', V == 24 and ndense > 0 and forms[:2] == ['rows_plus_ll'] * 2 and not plan['combine_alone'])
        put('ll_ve260_two_groups_ragged', V == 260 and all(gy == 2 for _, gy in plan['launches']) and (V // 4) % 64 != 0)
        put('ll_ve260_dense', V == 260 and ndense > 0 and forms[:2] == ['rows_plus_ll'] * 2)
        put('ll_ve23_scalar', V == 23 and scalar and plan['launches'][0][1] == 1)
        put('ll_ve75_scalar_two_groups', V == 75 and scalar and plan['launches'][0][1] == 2)
        put('ll_scalar_count65', scalar and np.any(counts == 65) and plan['levels'] >= 2)
        put('ll_scalar_count4097', scalar and np.any(counts == 4097) and plan['levels'] == 3)
        put('ll_word0_present', present[0])
        put('ll_word0_absent', not present[0])
        put('ll_last_word_present', present[-1])
        put('ll_last_word_absent', not present[-1])
        return ev
    dw = c['dw']
    lanes = {'rows32': 32, 'rows_plus': 32, 'rows64': 64}.get(forms[0]) if forms else None
    if lanes:
        for k in LENS:
            put('count%d_lanes%d' % (k, lanes), tree == k)
    chunks1 = -(-(-(-tree // SEG)) // SEG)              # level-1 chunk items of a word (1: its level-1 item is final)
    in_tree_heavy = tree > HEAVY_MIN
    put('tree_1_level', plan['levels'] == 1 and tree.max() <= SEG)
    put('tree_2_levels', plan['levels'] == 2 and SEG < tree.max() <= SEG * SEG)
    put('upper_fused_2_chunk_items', 'upper_fused' in forms and np.any(chunks1 == 2))
    put('upper_fused_32_chunk_items', 'upper_fused' in forms and chunks1.max() == FUSED_MAX)
    put('level2_launch_33_chunk_items', plan['levels'] == 3 and len(forms) == 3 and chunks1.max() == FUSED_MAX + 1
        and tree.max() > FUSED_MAX * SEG * SEG)
    put('tree_4_levels', plan['levels'] == 4 and len(forms) == 4 and tree.max() > SEG ** 3)
    put('count4096_in_tree_beside_dense', ndense > 0 and np.any(tree == HEAVY_MIN))
    put('count4097_dense', ndense > 0 and np.any(counts[dense] == HEAVY_MIN + 1))
    put('heavy_under_eighth_in_tree', dense_enabled(c) and len(heavy) > 0 and ndense == 0 and int(counts[heavy].sum()) * 8 < T)
    put('dense16', ndense == HEAVY_MAX and len(heavy) == HEAVY_MAX)
    put('heavy17_lightest_in_tree_combine_alone', len(heavy) == HEAVY_MAX + 1 and ndense == HEAVY_MAX and in_tree_heavy.sum() == 1
        and forms == ['rows_plus', 'upper_fused'] and plan['combine_alone'])
    put('dense_no_level1_combine_alone', ndense > 0 and plan['levels'] == 1 and forms == ['rows_plus'] and plan['combine_alone'])
    if ndense > 0:
        X = step_tokens(name, step)
        same = np.all(X == X[:, :1], axis=1) & np.isin(X[:, 0], dense)
        put('row_of_one_dense_word', same & (c['n'] >= 2))
    fused = plan['heavy'] == 'fused'
    for r in (64, 128, 256):
        put('heavy_rows%d' % r, fused and plan['heavy_rows'] == r and plan['heavy_blocks'] == -(-B // r))
    for k in (16, 64, 256):
        put('dense_B_not_multiple_of_%d' % k, fused and B % k != 0)
    put('dw4', dw == 4)
    put('dw128', dw == 128)
    put('dw132', dw == 132)
    for k in (200, 256):
        put('dw%d_default_tree' % k, dw == k and c['knob'] is None and forms == ['rows64', 'upper_fused'] and np.any(in_tree_heavy))
        put('dw%d_two_launches' % k, dw == k and c['knob'] == '1' and plan['heavy'] == 'two_launches' and forms[0] == 'rows64')
    put('dw260', dw == 260)
    put('dw300', dw == 300)
    put('dw388', dw == 388)
    put('dw516_dense_off', dw == 516 and ndense == 0 and int(counts[heavy].sum()) * 8 >= T and len(heavy) > 0)
    put('dw6_scalar', dw == 6 and forms[0] == 'scalar')
    put('dw70_scalar_upper_levels', dw == 70 and forms == ['scalar'] * 3 and plan['launches'][0][1] == 2 and np.any(in_tree_heavy))
    put('id%d' % U.id_dtype(Vw).itemsize, True)
    put('word0_present', present[0])
    put('word0_absent', not present[0])
    put('last_word_present', present[-1])
    put('last_word_absent', not present[-1])
    return ev
