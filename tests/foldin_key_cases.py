"""Fold-in steps whose only difficulty is the STRUCTURE of their keys, the kernel instance they take or the way their
instances were uploaded -- shared by the CPU proof of the inputs (test_foldin_keys_inputs_cpu.py) and the GPU test
(test_gpu_foldin_keys.py).  Patterned on tests/egrad_key_cases.py.

A fold-in step (csrc/kernels_foldin.h; the loss dispatch in csrc/host/api_foldin.inc, the sort / reduce / fix-up dispatch the
model's own, csrc/host/lazy_segsum.inc: EntityChain) runs the vectorspace step's kernels, changed
where it matters: foldin_nce<K> / foldin_nce_scalar<K> -- the row body of the step's loss kernel (csrc/kernels_vs.h,
nce_rows16 / nce_rows_wave) under another candidate policy -- score a two-part table and write a KEY per pair (the new row,
or the sentinel N for a pair on a frozen row); csort_pass sorts the B (z + 1) keys over the smallest b bits with 2^b > N;
foldin_chunk_reduce<VEC, NCH> reduces chunks of CHUNK = 16 sorted pairs and stops at the sentinel run, which is the END of the
order; egrad_fixup<VEC> (N >= 256) or egrad_fixup_wg<VEC> adds the carries of the runs that cross chunks.  The sort is stable
and the pairs are pair-major, so a step is fully described by a COUNT PER KEY: how many pairs hit each new row 0 .. N - 1 and
how many hit frozen rows.  y and the explicit negatives are built from such a count plan; every instance's positive is on a
new row, so the live total L satisfies B <= L <= B (z + 1) and a row's count is at least its number of positives.

Every case has TWO steps with different plans (step 2: the counts reversed over the rows and the sentinel count changed), so
that nothing of step 1's run bounds, carries or keys may survive into step 2, and states the plan FoldIn.plan()
(sert_debug_foldin_plan) must report.  EVENTS is the one list of structures the cases have to produce between them;
events_of() finds the ones a case produces from its keys, the constants 16 and 2048 and the stated plan alone.

chunked_gradient() restates the reduce and the fix-up on the CPU in float64, chunk by chunk -- not as a reference (the twin of
tests/foldin_cases.py is the reference, and the restatement is proved against it) but so that the CPU test can make it wrong
on purpose, one carry or one bound at a time, and show that the GPU test's bounds notice."""
import numpy as np

from oracle import sert_oracle as O
from tests import foldin_cases as FC

CHUNK = 16            # csrc/kernels_egrad.h: kEChunk
SORT_TILE = 2048      # csrc/kernels_sort.h: kSortTile
SORT_MAX_BITS = 11    # csrc/kernels_sort.h: kSortMaxBits
SLAB = 65536          # csrc/host/foldin_common.inc, fold_project_slabs: rows projected per slab of sert_foldin_upload
STEPS = 2
VW, VE, DW, NWIN = 50, 7, 12, 3       # the base case of tests/foldin_cases.py: the forward is not what these cases are about
LAM, LR = 0.01, 0.01

RUN_EVENTS = (
    'run1_first_slot', 'run1_last_slot', 'run15', 'run16_aligned', 'run16_unaligned', 'run17', 'run31', 'run32_aligned', 'run33',
    'run17_from_last_slot', 'run_ends_at_chunk_end_from_earlier_chunk', 'run_over_3_chunks',
    'fixup_wave_6_chunks', 'fixup_wave_70_chunks', 'fixup_wg_6_chunks', 'fixup_wg_70_chunks',
    'one_row_takes_all', 'row0_absent', 'last_row_absent', 'last_row_present', 'absent_stretch_5',
)
SENTINEL_EVENTS = (
    'sentinel_at_chunk_start', 'sentinel_in_slot1', 'sentinel_in_last_slot', 'sentinel_run1_is_last_pair',
    'sentinel_longer_than_tile', 'no_sentinel_total_mod16_zero', 'no_sentinel_total_mod16_nonzero',
    'last_live_run_3_chunks_ends_in_sentinel_chunk', 'last_row_absent_before_sentinel',
)
SIZE_EVENTS = (
    'total_2048', 'total_2049', 'total_above_two_tiles',
    'N1', 'N4_3bits', 'N255', 'N256', 'N2047_11bits_1pass', 'N2048_12bits_2passes', 'N_17bits_unequal_passes', 'N_mod4_nonzero',
    'reduce_4_1', 'reduce_4_2', 'reduce_4_5_de300', 'reduce_4_5_de320', 'reduce_4_8_de384', 'reduce_4_8_de512',
    'reduce_1_4_one_column_pass', 'reduce_1_4_two_column_passes', 'reduce_1_4_eight_column_passes',
    'fixup_wave_vec4', 'fixup_wave_vec1', 'fixup_wg_vec4', 'fixup_wg_vec1', 'fixup_wg_vec4_de512',
)
LOSS_EVENTS = tuple('%s_K%d_%s' % (f, k, t) for f in ('nce', 'nce_scalar') for k in range(1, 9) for t in ('train', 'eval'))
UPLOAD_EVENTS = ('upload_batch_straddles_slab', 'upload_batch_behind_slab', 'upload_slab_bf16_pipe', 'upload_dw_mod4_nonzero',
                 'upload_w_none')
EVENTS = RUN_EVENTS + SENTINEL_EVENTS + SIZE_EVENTS + LOSS_EVENTS + UPLOAD_EVENTS


def plan_of(loss, k, bits, passes, vec, nch, cols, fixup, tiles):
    """FoldIn.plan() after a training step."""
    return dict(loss=loss, k=k, train=True, sort_bits=bits, passes=passes, vec=vec, nch=nch, col_passes=cols, fixup=fixup,
                tiles=tiles)


def _spread(N, head, rest, over, tail_zeros=0):
    """counts (N): `head` on the first rows, `rest` pairs spread as evenly as they go over the `over` rows that end `tail_zeros`
    short of the last row, every row between absent."""
    c = np.zeros(N, dtype=np.int64)
    c[:len(head)] = head
    assert rest >= over > 0 and len(head) + over + tail_zeros <= N, (rest, over)
    hi = N - tail_zeros
    c[hi - over:hi] = rest // over
    c[hi - over:hi - over + rest % over] += 1
    return c


def _scatter(N, live, seed, runs):
    """counts (N): the `runs` and, for the rest of the `live` pairs, runs of 1, on rows drawn without replacement over the whole
    range (in a seeded order), N - 1 among them."""
    rng = np.random.RandomState(seed)
    m = len(runs) + live - sum(runs)
    ids = rng.choice(N - 1, m - 1, replace=False)
    ids = rng.permutation(np.concatenate([ids, [N - 1]]))
    c = np.zeros(N, dtype=np.int64)
    c[ids] = 1
    c[ids[:len(runs)]] = runs
    return c


# the runs of `runs_wave_v1`, by sorted position (start .. end), as tests/egrad_key_cases.py has them:
#   1 (0..1: first slot)  15 (1..16)  16 (16..32: aligned, sole owner of chunk 1)  32 (32..64: aligned, one tail + one head)
#   15 (64..79)  1 (79..80: last slot)  17 (80..97)  16 (97..113: not aligned)  31 (113..144: ends at a chunk's end, began
#   two chunks earlier)  33 (144..177)  14 (177..191)  17 (191..208: starts in the last slot of chunk 11)
#   100 (208..308: 7 chunks)  1125 (308..1433: 71 chunks)  then seven absent rows
_RUNS_A = [1, 15, 16, 32, 15, 1, 17, 16, 31, 33, 14, 17, 100, 1125, 0, 0, 0, 0, 0, 0, 0]

# name -> B, z, N, de; counts (N): the live pairs per new row of step 1 (the pairs left over are the sentinel run); sent2: the
# sentinel count of step 2, whose live counts are step 1's reversed over the rows, the difference taken by the largest run.
STRUCTURE_CASES = {
    # N >= 256, d_e % 4 != 0: egrad_fixup<1>; 70 columns: the second column pass of foldin_chunk_reduce<1, 4>; 2049 pairs: two
    # sort tiles, the second of one key; L = 1616: the sentinel run starts at a chunk start
    'runs_wave_v1': dict(B=683, z=2, N=300, de=70, counts=_spread(300, _RUNS_A, 183, 40), sent2=300,
                         plan=plan_of('scalar', 2, 9, 1, 1, 4, 2, 'wave', 2)),
    # N < 256, d_e % 4 != 0: egrad_fixup_wg<1>; 510 columns: eight column passes; 2048 pairs, 2047 of them live: a sentinel run of
    # one pair in the last slot of the last chunk, the last three rows absent in front of it; runs of 19 and 71 chunks
    'runs_wg_v1_d510': dict(B=512, z=3, N=40, de=510, counts=_spread(40, [0, 300, 0, 0, 0, 0, 0, 1130, 17, 33, 1, 31], 535, 12, 3),
                            sent2=500, plan=plan_of('scalar', 8, 6, 1, 1, 4, 8, 'workgroup', 1)),
    # d_e = 512: foldin_chunk_reduce<4, 8> and egrad_fixup_wg<4> with its LDS slab full; 1500 pairs, all live: no sentinel and a
    # ragged last chunk
    'runs_wg_v4_d512': dict(B=300, z=4, N=20, de=512, counts=_spread(20, [5, 1130, 300, 33, 0, 0, 1], 31, 4, 2), sent2=170,
                            plan=plan_of('vector', 8, 5, 1, 4, 8, 1, 'workgroup', 1)),
    # one row takes every pair (260 chunks under egrad_fixup<4>), its neighbours absent, no sentinel, 4160 pairs: more than two
    # sort tiles and a multiple of 16; d_e = 384: <4, 8>
    'one_row_d384': dict(B=1040, z=3, N=300, de=384, counts=_spread(300, [0] * 150, 4160, 1, 149), sent2=100,
                         plan=plan_of('vector', 6, 9, 1, 4, 8, 1, 'wave', 3)),
    # d_e = 320: <4, 5> at its largest width; the last row's run of 59 starts at 308 and ends at L = 367: four chunks, the last of
    # them the one the sentinel run begins in, in its last slot
    'runs_wave_d320': dict(B=200, z=4, N=260, de=320, counts=_spread(260, _RUNS_A[:13], 59, 1), sent2=700,
                           plan=plan_of('vector', 5, 9, 1, 4, 5, 1, 'wave', 1)),
    # N = 256: the first N of egrad_fixup<4>; d_e = 300 (the README's C4 dimension): <4, 5> and foldin_nce<5> with a lane group
    # that holds three float4 of its fifth chunk; L = 113: the chunk the sentinel begins in holds one live pair
    'n256_d300': dict(B=100, z=4, N=256, de=300, counts=_scatter(256, 113, 21, [33, 17, 16, 2, 3]), sent2=380,
                      plan=plan_of('vector', 5, 9, 1, 4, 5, 1, 'wave', 1)),
    # N = 255: the last N of egrad_fixup_wg<4>, N % 4 != 0 (the bounds array is 256 long); d_e = 128: <4, 2>; a run of 100
    'n255_d128': dict(B=200, z=4, N=255, de=128, counts=_scatter(255, 400, 22, [100, 33, 17, 16, 65, 2, 3]), sent2=500,
                      plan=plan_of('vector', 2, 8, 1, 4, 2, 1, 'workgroup', 1)),
    # N = 2047: 11 key bits, one pass, the sentinel the largest key of the digit; d_e = 64: <4, 1>
    'n2047_d64': dict(B=300, z=5, N=2047, de=64, counts=_scatter(2047, 900, 23, [33, 17, 16, 65, 2, 3, 100]), sent2=800,
                      plan=plan_of('vector', 1, 11, 1, 4, 1, 1, 'wave', 1)),
    # N = 2048: 12 key bits, two passes of 6 -- an off-by-one in sort_bits would sort the sentinel 2048 as key 0; 3000 pairs in
    # two tiles, 2300 of them the sentinel run: longer than a tile
    'n2048_d8': dict(B=600, z=4, N=2048, de=8, counts=_scatter(2048, 700, 24, [33, 17, 16, 65, 2, 3, 100]), sent2=1900,
                     plan=plan_of('vector', 1, 12, 2, 4, 1, 1, 'wave', 2)),
    # N = 4: 3 key bits, the sentinel 4 = 100b
    'n4_d8': dict(B=32, z=4, N=4, de=8, counts=np.array([40, 0, 33, 17]), sent2=40,
                  plan=plan_of('vector', 1, 3, 1, 4, 1, 1, 'workgroup', 1)),
    # N = 1: one key bit
    'n1_d8': dict(B=32, z=4, N=1, de=8, counts=np.array([50]), sent2=95,
                  plan=plan_of('vector', 1, 1, 1, 4, 1, 1, 'workgroup', 1)),
    # N = 70000: 17 key bits, passes of 9 and 8, nearly all rows absent
    'n70000_d8': dict(B=500, z=4, N=70000, de=8, counts=_scatter(70000, 1200, 25, [33, 17, 16, 65, 2, 3, 100, 300]), sent2=1000,
                      plan=plan_of('vector', 1, 17, 2, 4, 1, 1, 'wave', 2)),
}

# one tiny case per loss-kernel instance that no structure case has the d_e of: B = 24 (a ragged last workgroup), z = 4
_LOSS_DE = {'vector': (68, 132, 256, 260, 448), 'scalar': (63, 65, 130, 250, 301, 382, 446)}


def _loss_case(form, de):
    k = -(-(de // 4) // 16) if form == 'vector' else -(-de // 64)
    vec, nch = (4, next(n for n in (1, 2, 5, 8) if k <= n)) if form == 'vector' else (1, 4)
    cols = -(-(de // vec) // (16 * nch))
    return dict(B=24, z=4, N=5, de=de, counts=np.array([9, 0, 21, 1, 17]), sent2=50,
                plan=plan_of(form, k, 3, 1, vec, nch, cols, 'workgroup', 1))


LOSS_CASES = {'loss_%s_d%d' % (form, de): _loss_case(form, de) for form in ('vector', 'scalar') for de in _LOSS_DE[form]}
# ... and the structure cases whose d_e completes the sixteen instances: 64 (K = 1), 384 (6), 512 (8), 510 (scalar, 8), 300 (5)
LOSS_INSTANCE_CASES = tuple(LOSS_CASES) + ('n2047_d64', 'one_row_d384', 'runs_wg_v4_d512', 'runs_wg_v1_d510', 'n256_d300')

# how the instances were uploaded.  batches: the batch each step trains; M instances
UPLOAD_CASES = {
    # M = 65536 + 70, B = 40: batch 1638 is rows 65520 .. 65559 (straddles the slab boundary), batch 1639 lies behind it; the
    # first slab's projection is a 65536 x 8 x 12 product: the bf16-pipe GEMM
    'upload_two_slabs': dict(B=40, z=4, N=5, de=8, M=SLAB + 70, batches=(1638, 1639), counts=np.array([30, 0, 21, 40, 17]),
                             sent2=60, plan=plan_of('vector', 1, 3, 1, 4, 1, 1, 'workgroup', 1)),
    # d_w = 10: vs_gather_mean<uint32_t, 1>
    'upload_dw10': dict(B=40, z=4, N=5, de=8, dw=10, counts=np.array([30, 0, 21, 40, 17]), sent2=60,
                        plan=plan_of('vector', 1, 3, 1, 4, 1, 1, 'workgroup', 1)),
    # w = None: the ones vector
    'upload_w_none': dict(B=40, z=4, N=5, de=8, w_none=True, counts=np.array([30, 0, 21, 40, 17]), sent2=60,
                          plan=plan_of('vector', 1, 3, 1, 4, 1, 1, 'workgroup', 1)),
}

CASES = dict(STRUCTURE_CASES)
CASES.update(LOSS_CASES)
CASES.update(UPLOAD_CASES)
SEEDS = {name: 700 + k for k, name in enumerate(CASES)}
# the case run also at lambda = 0 (absent rows exactly untouched) and the multi-tile, two-pass case run twice
EXACT_CASE, REPRO_CASE = 'runs_wave_v1', 'n2048_d8'


def step_counts(c, s):
    """(live counts (N), sentinel count) of step s: the stated ones; then the live counts reversed over the rows with the
    difference to the stated sentinel count of step 2 taken by the largest run."""
    total = c['B'] * (c['z'] + 1)
    counts = np.asarray(c['counts'], dtype=np.int64)
    if s == 0:
        return counts, total - int(counts.sum())
    rev = counts[::-1].copy()
    rev[int(np.argmax(rev))] += (total - c['sent2']) - int(rev.sum())
    return rev, c['sent2']


def _build_step(rng, c, s):
    """(y (B) int32, neg (B, z) int64) of a step from its count plan: the B positives dealt over the present rows in
    proportion to their counts (never more than a row's count), the other live pairs and the sentinel pairs -- frozen rows
    drawn uniformly -- permuted over the B z negative slots."""
    B, z, N = c['B'], c['z'], c['N']
    counts, sent = step_counts(c, s)
    L = int(counts.sum())
    assert counts.min() >= 0 and sent >= 0 and B <= L <= B * (z + 1), (c['B'], L, sent)
    pos = counts * B // L
    room = np.nonzero(pos < counts)[0]
    short = B - int(pos.sum())
    assert 0 <= short <= len(room)
    pos[room[:short]] += 1
    y = rng.permutation(np.repeat(np.arange(N, dtype=np.int64), pos))
    live = VE + np.repeat(np.arange(N, dtype=np.int64), counts - pos)
    frozen = rng.randint(0, VE, size=sent).astype(np.int64)
    neg = rng.permutation(np.concatenate([live, frozen])).reshape(B, z)
    return y.astype(np.int32), neg


_cache = {}


def case_problem(name):
    """The case as tests/foldin_cases.FoldInTwin and the GPU test take it, built once per process; read-only.  Beyond the keys
    of foldin_cases.make_case: 'batches' (the batch step s trains), 'neg' [neg of step 0, of step 1], 'eval_neg', 'w_upload'
    (None for the ones vector), 'plan'."""
    if name not in _cache:
        spec = CASES[name]
        rng = np.random.RandomState(SEEDS[name])
        c = dict(name=name, Vw=VW, Ve=VE, n=NWIN, dw=spec.get('dw', DW), lam=LAM, lr=LR)
        c.update(spec)
        B, z, N, de, dw = c['B'], c['z'], c['N'], c['de'], c['dw']
        c['batches'] = tuple(spec.get('batches', (0, 1)))
        M = c['M'] = spec.get('M', STEPS * B + 5)           # (a trailing M mod B instances are never visited)
        c['Rw'] = O.glorot_uniform(rng, (VW, dw))
        c['Re'] = O.glorot_uniform(rng, (VE, de))
        c['W'] = O.glorot_uniform(rng, (dw, de))
        c['b'] = (0.1 * rng.randn(de)).astype(np.float32)
        # (Glorot's scale of at most 256 rows: with lr = 0.01 Adam moves every element by about 0.002 a step, absent rows
        #  included -- the L2 term -- and rows of a 70000-row Glorot table are that small themselves: they would cancel)
        lim = np.sqrt(6.0 / (min(N, 256) + de))
        c['E0'] = rng.uniform(-lim, lim, size=(N, de)).astype(np.float32)
        c['X'] = rng.randint(0, VW, size=(M, NWIN)).astype(np.int32)
        y = rng.randint(0, N, size=M).astype(np.int32)
        negs = []
        for s, b in enumerate(c['batches']):
            y[b * B:(b + 1) * B], neg = _build_step(rng, c, s)
            negs.append(neg)
        c['y'], c['neg'] = y, negs
        c['w_upload'] = None if spec.get('w_none') else rng.uniform(0.5, 2.0, M).astype(np.float32)
        c['w'] = np.ones(M, np.float32) if c['w_upload'] is None else c['w_upload']
        c['eval_neg'] = rng.randint(0, VE + N, size=(B, z)).astype(np.int64)
        for a in list(c.values()) + negs:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def step_keys(name, s):
    """The (B (z + 1)) keys the loss kernel writes for step s, pair-major: the new row, or the sentinel N for a frozen row."""
    c = case_problem(name)
    B, b = c['B'], c['batches'][s]
    cand = np.concatenate([(VE + c['y'][b * B:(b + 1) * B].astype(np.int64))[:, None], c['neg'][s]], axis=1).ravel()
    return np.where(cand >= VE, cand - VE, c['N'])


# --------------------------------------------------------------------------------------------------------------------- #
# the twin's run of a case, computed once and shared
# --------------------------------------------------------------------------------------------------------------------- #

_refs = {}


def case_reference(name, dtype, lam=None):
    """The twin's two steps of a case in `dtype`: a list, per step, of dict(loss, E, m, v) -- copies of the twin's state after
    the step, read-only -- and after them the twin itself.  lam: in place of the case's lambda."""
    key = (name, np.dtype(dtype).name, lam)
    if key not in _refs:
        c = case_problem(name)
        if lam is not None:
            c = dict(c, lam=lam)
        tw = FC.FoldInTwin(c, dtype)
        out = []
        for s, b in enumerate(c['batches']):
            loss = tw.train_step(b, c['neg'][s])
            st = dict(loss=loss, E=tw.E.copy(), m=tw.m.copy(), v=tw.v.copy())
            for a in st.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out.append(st)
        _refs[key] = (out, tw)
    return _refs[key]


def pair_terms(c, E, s):
    """What the gradient kernels read in step s with the new rows at E, from the oracle on the extended table in float64:
    (keys (B (z + 1)), coef (B (z + 1)) = d loss / d u of every pair, P (B, d_e) = clip(t) of the batch's instances, the
    oracle's own data term of dE (N, d_e), and the oracle's forward record: t, sig, ...)."""
    B, b = c['B'], c['batches'][s]
    sl = slice(b * B, (b + 1) * B)
    ext = np.concatenate([np.asarray(c['Re'], np.float64), np.asarray(E, np.float64)], axis=0)
    ora = O.VectorSpaceOracle(B, c['n'], c['z'], c['Rw'], ext, c['W'], c['b'], 0.0, dtype=np.float64)
    _, grads, f = ora.loss_and_grads(c['X'][sl], c['Ve'] + c['y'][sl].astype(np.int64), c['w'][sl], c['neg'][s])
    cand = f['cand'].ravel()
    keys = np.where(cand >= c['Ve'], cand - c['Ve'], c['N'])
    return keys, f['du'].ravel(), f['p'], grads[0][c['Ve']:], f


class ChunkedGradient(object):
    """foldin_chunk_reduce + egrad_fixup on the CPU in float64, with the buffers a handle keeps from step to step (G, the head
    and tail carries, the run bounds).  `wrong`: None, or the one thing this instance gets wrong --
      ('drop_head', row) / ('drop_tail', row)   the fix-up of `row` leaves out its head carry / its first tail carry
      ('second_column_pass',)                   the columns of the second column pass (64 and up) are never written
      ('drop_last_live_pair',)                  the live pair in front of the sentinel is not reduced
      ('sentinel_into_row0',)                   the sentinel run is added into row 0
      ('stale_bounds',)                         the run bounds are not cleared between steps."""

    def __init__(self, N, de, total, wrong=None):
        self.N, self.de, self.wrong = N, de, wrong or ('none',)
        chunks = -(-total // CHUNK)
        self.G = np.zeros((N, de))
        self.head, self.tail = np.zeros((chunks, de)), np.zeros((chunks, de))
        self.run_start, self.run_end = np.zeros(N, np.int64), np.zeros(N, np.int64)

    def step(self, keys, coef, P, zp1):
        """-> dE (N, d_e), the data term, of one step."""
        N, wrong = self.N, self.wrong[0]
        total = len(keys)
        order = np.argsort(keys, kind='stable')
        sk = keys[order]
        L = int(np.count_nonzero(sk < N))
        assert np.all(sk[L:] == N)
        C = coef[order][:, None] * P[order // zp1]
        if wrong == 'drop_last_live_pair':
            C[L - 1] = 0
        if wrong != 'stale_bounds':
            self.run_start[:] = 0
            self.run_end[:] = 0
        G, head, tail = self.G, self.head, self.tail
        for chunk in range(-(-L // CHUNK)):
            cb = chunk * CHUNK
            ce = min(total, cb + CHUNK)
            cnt = min(L, ce) - cb
            k = sk[cb:cb + cnt]
            cuts = np.concatenate([[0], np.nonzero(np.diff(k))[0] + 1, [cnt]])
            for jb, je in zip(cuts[:-1], cuts[1:]):
                e = int(k[jb])
                touches_begin = jb == 0 and cb > 0 and sk[cb - 1] == e
                touches_end = je == cnt and cnt == ce - cb and ce < total and sk[ce] == e
                if not touches_begin:
                    self.run_start[e] = cb + jb
                if not touches_end:
                    self.run_end[e] = cb + je
                acc = C[cb + jb:cb + je].sum(axis=0)
                if touches_end:
                    tail[chunk] = acc
                elif touches_begin:
                    head[chunk] = acc
                else:
                    G[e] = acc
        s, t = self.run_start, self.run_end
        G[t <= s] = 0
        for e in np.nonzero(t > s)[0]:
            cs, cl = s[e] // CHUNK, (t[e] - 1) // CHUNK
            if cs == cl:
                continue
            carries = tail[cs:cl].sum(axis=0) - (tail[cs] if self.wrong == ('drop_tail', e) else 0)
            G[e] = carries + (0 if self.wrong == ('drop_head', e) else head[cl])
        out = G.copy()
        if wrong == 'second_column_pass':
            out[:, 64:] = 0
        if wrong == 'sentinel_into_row0':
            out[0] += C[L:].sum(axis=0)
        return out


def chunked_run(name, wrong=None, X=None):
    """Both steps of a case in float64 with the gradient's data term from ChunkedGradient (made `wrong`), Adam and the L2 term
    from the oracle: a list, per step, of dict(E, m, v, g).  X: other instances than the case's (the upload mutant)."""
    c = case_problem(name)
    if X is not None:
        c = dict(c, X=X)
    B, zp1 = c['B'], c['z'] + 1
    E = np.array(c['E0'], dtype=np.float64)
    opt = O.Adam([E], lr=c['lr'])
    cg = ChunkedGradient(c['N'], c['de'], B * zp1, wrong)
    out = []
    for s in range(STEPS):
        keys, coef, P, _, _ = pair_terms(c, E, s)
        g = cg.step(keys, coef, P, zp1)
        opt.update([E], [g + (c['lam'] / B) * E])
        out.append(dict(E=E.copy(), m=opt.m[0].copy(), v=opt.v[0].copy(), g=g))
    return out


# --------------------------------------------------------------------------------------------------------------------- #
# the events a case produces
# --------------------------------------------------------------------------------------------------------------------- #

def key_events(counts, sent, N, de, plan):
    """The RUN, SENTINEL and SIZE events one step with these live counts per row and this sentinel count produces under the
    stated plan -- from the counts, CHUNK, SORT_TILE and the plan alone: the sort is stable, so row e's run is
    [sum(counts[:e]), sum(counts[:e + 1])) and the sentinel run is [L, total)."""
    counts = np.asarray(counts, dtype=np.int64)
    L = int(counts.sum())
    total = L + sent
    end = np.cumsum(counts)
    start = end - counts
    here = counts > 0
    s, t, ln = start[here], end[here], counts[here]
    slot = s % CHUNK
    nchunks = (t - 1) // CHUNK - s // CHUNK + 1
    ev = set()

    def put(name, cond):
        if bool(np.any(cond)):
            ev.add(name)

    put('run1_first_slot', (ln == 1) & (slot == 0))
    put('run1_last_slot', (ln == 1) & (slot == CHUNK - 1))
    put('run16_aligned', (ln == 16) & (slot == 0))
    put('run16_unaligned', (ln == 16) & (slot != 0))
    put('run32_aligned', (ln == 32) & (slot == 0))
    for k in (15, 17, 31, 33):
        put('run%d' % k, ln == k)
    put('run17_from_last_slot', (ln == 17) & (slot == CHUNK - 1))
    put('run_ends_at_chunk_end_from_earlier_chunk', (t % CHUNK == 0) & (nchunks >= 2))
    put('run_over_3_chunks', nchunks >= 3)
    kind = 'wave' if plan['fixup'] == 'wave' else 'wg'
    put('fixup_%s_6_chunks' % kind, (nchunks >= 6) & (nchunks < 70))
    put('fixup_%s_70_chunks' % kind, nchunks >= 70)
    e = np.nonzero(here)[0]
    put('one_row_takes_all', len(e) == 1 and sent == 0 and N > 1)
    put('row0_absent', counts[0] == 0)
    put('last_row_absent', counts[-1] == 0)
    put('last_row_present', counts[-1] > 0)
    put('absent_stretch_5', np.diff(np.concatenate([[-1], e, [N]])) - 1 >= 5)

    put('sentinel_at_chunk_start', sent > 0 and L % CHUNK == 0)
    put('sentinel_in_slot1', sent > 0 and L % CHUNK == 1)
    put('sentinel_in_last_slot', sent > 0 and L % CHUNK == CHUNK - 1)
    put('sentinel_run1_is_last_pair', sent == 1 and total % CHUNK == 0)
    put('sentinel_longer_than_tile', sent > SORT_TILE)
    put('no_sentinel_total_mod16_zero', sent == 0 and total % CHUNK == 0)
    put('no_sentinel_total_mod16_nonzero', sent == 0 and total % CHUNK != 0)
    put('last_live_run_3_chunks_ends_in_sentinel_chunk', sent > 0 and L % CHUNK != 0 and nchunks[-1] >= 3)
    put('last_row_absent_before_sentinel', sent > 0 and counts[-1] == 0)

    put('total_2048', total == SORT_TILE and plan['tiles'] == 1)
    put('total_2049', total == SORT_TILE + 1 and plan['tiles'] == 2)
    put('total_above_two_tiles', total > 2 * SORT_TILE and plan['tiles'] >= 3)
    bits, passes = plan['sort_bits'], plan['passes']
    put('N1', N == 1 and bits == 1)
    put('N4_3bits', N == 4 and bits == 3)
    put('N255', N == 255 and plan['fixup'] == 'workgroup')
    put('N256', N == 256 and plan['fixup'] == 'wave')
    put('N2047_11bits_1pass', N == 2047 and (bits, passes) == (11, 1) and sent > 0)
    put('N2048_12bits_2passes', N == 2048 and (bits, passes) == (12, 2) and sent > 0)
    put('N_17bits_unequal_passes', bits == 17 and passes == 2 and N > (1 << 16) and e[-1] >= (1 << 16))
    put('N_mod4_nonzero', N % 4 != 0 and N > 4)
    vn, cols = (plan['vec'], plan['nch']), plan['col_passes']
    put('reduce_4_1', vn == (4, 1) and de % 4 == 0 and de <= 64)
    put('reduce_4_2', vn == (4, 2) and de % 4 == 0 and 64 < de <= 128)
    put('reduce_4_5_de300', vn == (4, 5) and de == 300)
    put('reduce_4_5_de320', vn == (4, 5) and de == 320)
    put('reduce_4_8_de384', vn == (4, 8) and de == 384)
    put('reduce_4_8_de512', vn == (4, 8) and de == 512)
    put('reduce_1_4_one_column_pass', vn == (1, 4) and cols == 1 and de % 4 != 0 and de <= 64)
    put('reduce_1_4_two_column_passes', vn == (1, 4) and cols == 2 and de == 70)
    put('reduce_1_4_eight_column_passes', vn == (1, 4) and cols == 8 and de == 510)
    put('fixup_%s_vec%d' % (kind, plan['vec']), True)
    put('fixup_wg_vec4_de512', plan['fixup'] == 'workgroup' and plan['vec'] == 4 and de == 512)
    return ev


def events_of(name, plan=None):
    """The events both steps of a case (and, for a loss-instance case, its evaluation) produce; `plan`: the reported one in
    place of the stated one."""
    c = case_problem(name)
    plan = c['plan'] if plan is None else plan
    ev = set()
    for s in range(STEPS):
        keys = step_keys(name, s)
        counts = np.bincount(keys, minlength=c['N'] + 1)
        ev |= key_events(counts[:c['N']], int(counts[c['N']]), c['N'], c['de'], plan)
    form = 'nce' if plan['loss'] == 'vector' else 'nce_scalar'
    ev.add('%s_K%d_train' % (form, plan['k']))
    if name in LOSS_INSTANCE_CASES:
        ev.add('%s_K%d_eval' % (form, plan['k']))
    B = c['B']
    for b in c['batches']:
        if b * B < SLAB < (b + 1) * B and c['M'] > SLAB:
            ev.add('upload_batch_straddles_slab')
        if b * B >= SLAB:
            ev.add('upload_batch_behind_slab')
    if c['M'] >= SLAB and c['de'] <= 128 and c['dw'] % 4 == 0:
        ev.add('upload_slab_bf16_pipe')          # (both tests assert the route itself: sert_debug_gemm_route)
    if c['dw'] % 4 != 0:
        ev.add('upload_dw_mod4_nonzero')
    if c['w_upload'] is None:
        ev.add('upload_w_none')
    return ev
