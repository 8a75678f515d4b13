"""Vectorspace problems whose only difficulty is the STRUCTURE of their (entity, pair) keys -- shared by the CPU proof of the
inputs (test_egrad_keys_inputs_cpu.py) and the GPU test (test_gpu_egrad_keys.py).

dR_e, the entity-table gradient of the NCE loss, is formed without atomics by one of two mechanisms (csrc/kernels_egrad.h,
csrc/kernels_sort.h; the choice of path in csrc/host/step_vectorspace.inc and api_model.inc, the sorted chain's dispatch --
shared with the fold-in step, tests/foldin_key_cases.py -- in csrc/host/lazy_segsum.inc: EntityChain):

  sorted   entity_key_sort -> egrad_chunk_reduce<VEC, NCH> -> egrad_fixup<VEC> / egrad_fixup_wg<VEC>: the keys counting-sorted
           by entity (stable), reduced in chunks of CHUNK = 16 sorted pairs; a run that crosses a chunk boundary leaves a tail
           carry in every chunk but its last and a head carry in its last, and the chunk that holds a run's first / last pair
           records run_start / run_end.  Whether that is right depends on where every run starts and ends relative to a chunk:
           a sorted case is a COUNT PER ENTITY (the sort is stable, so the counts alone fix every run's position).
  bucket   (V_e <= 2048, d_e % 4 == 0, d_e <= 128) egrad_bucket -> egrad_acc<2>: the batch cut into sub-groups of rows, each
           sub-group's pairs into one list per range of 16 entities; lists walked 64 entries at a time, their T rows 16 at a
           time.  Here placement matters: a bucket case names, per sub-group of the geometry it states, how many pairs fall in
           which range.

Everything else is kept tame, as util.make_vs_problem makes it: Glorot-scale parameters, weights in [0.5, 2], lambda = 0.01.
Every case has TWO steps with different plans (step 2: the counts reversed over the entities / the sub-group plans rotated
and the ranges mirrored), so that nothing of step 1's run bounds, carries or lists may survive into step 2.

Each case states the plan Engine.egrad_plan() (sert_debug_egrad_plan) must report.  EVENTS is the one list of key
structures the cases have to produce between them; events_of() finds the ones a case produces, from its keys, the constant
16 and the stated plan alone."""
import numpy as np

from oracle import sert_oracle as O
from tests import util as U

CHUNK = 16            # csrc/kernels_egrad.h: kEChunk
SORT_TILE = 2048      # csrc/kernels_sort.h: kSortTile
RANGE = 16            # entities per range of the bucket path
LAM, STEPS = 0.01, 2
N, VW, DW = 2, 200, 8     # window, word vocabulary, word dimension: the forward is not what these cases are about

SORTED_EVENTS = (
    'run1_first_slot', 'run1_last_slot', 'run16_aligned', 'run16_unaligned', 'run32_aligned', 'run15', 'run17', 'run31', 'run33',
    'run17_from_last_slot', 'run_ends_at_chunk_end_from_earlier_chunk', 'run_over_3_chunks',
    'fixup_wave_6_chunks', 'fixup_wave_70_chunks', 'fixup_wg_18_chunks', 'fixup_wg_70_chunks',
    'one_entity_takes_all', 'entity0_absent', 'last_entity_absent', 'last_entity_present', 'absent_stretch_5',
    'total_mod16_zero', 'total_mod16_nonzero', 'total_below_tile', 'total_2048', 'total_2049', 'total_above_tile',
    'Ve2048_11bits_1pass', 'Ve2049_12bits_2passes', 'Ve_17bits_unequal_passes',
    'reduce_4_1', 'reduce_4_2', 'reduce_4_5', 'reduce_4_8_de384', 'reduce_4_8_de512', 'reduce_1_4_second_column_pass',
    'fixup_wave_vec4', 'fixup_wave_vec1', 'fixup_wg_vec4', 'fixup_wg_vec1', 'fixup_wg_vec4_de512',
)
BUCKET_EVENTS = (
    'list0', 'list1', 'list16', 'list17', 'list63', 'list64', 'list65', 'list129',
    'sub_group_in_one_range', 'sub_group_in_last_range', 'Ve_le_16', 'Ve_ragged_last_range', 'Ve2048_128_ranges',
    'ragged_last_sub_group', 'ragged_last_group', 'fewer_sub_groups_than_16', 'z0', 'sub_pairs_not_power_of_two',
    'subs_per_group_gt_32', 'de4', 'de128',
)
EVENTS = SORTED_EVENTS + BUCKET_EVENTS


# --------------------------------------------------------------------------------------------------------------------- #
# count plans of the sorted cases
# --------------------------------------------------------------------------------------------------------------------- #

def _spread(V, total, head, over, tail_zeros=0):
    """counts (V): `head` on the first entities, the remaining pairs spread as evenly as they go over the `over` entities that end
    `tail_zeros` short of the table's end, every entity between absent."""
    c = np.zeros(V, dtype=np.int64)
    c[:len(head)] = head
    rest = total - int(c.sum())
    assert rest >= over > 0 and len(head) + over + tail_zeros <= V, (rest, over)
    hi = V - tail_zeros
    c[hi - over:hi] = rest // over
    c[hi - over:hi - over + rest % over] += 1
    return c


def _scatter(V, total, seed, runs):
    """counts (V): the `runs` and, for the rest of the pairs, runs of 1, on entities drawn without replacement over the whole
    id range (in a seeded order), V - 1 among them."""
    rng = np.random.RandomState(seed)
    m = len(runs) + total - sum(runs)
    ids = rng.choice(V - 1, m - 1, replace=False)
    ids = rng.permutation(np.concatenate([ids, [V - 1]]))
    c = np.zeros(V, dtype=np.int64)
    c[ids] = 1
    c[ids[:len(runs)]] = runs
    return c


# the runs of `runs_wave_v1`, by sorted position (start .. end):
#   1 (0..1: first slot)  15 (1..16)  16 (16..32: aligned, sole owner of chunk 1)  32 (32..64: aligned, one tail + one head)
#   15 (64..79)  1 (79..80: last slot)  17 (80..97)  16 (97..113: not aligned)  31 (113..144: ends at a chunk's end, began
#   two chunks earlier)  33 (144..177)  14 (177..191)  17 (191..208: starts in the last slot of chunk 11)
#   100 (208..308: 7 chunks)  1125 (308..1433: 71 chunks)  then seven absent entities
_RUNS_A = [1, 15, 16, 32, 15, 1, 17, 16, 31, 33, 14, 17, 100, 1125, 0, 0, 0, 0, 0, 0, 0]

SORTED_CASES = {
    # V_e >= 256, d_e % 4 != 0: egrad_fixup<1>; 70 columns: the second column pass of egrad_chunk_reduce<1, 4>; 2049 pairs
    'runs_wave_v1': dict(B=683, z=2, Ve=300, de=70, counts=_spread(300, 2049, _RUNS_A, 40),
                         plan=dict(path='sorted', sort_bits=9, passes=1, vec=1, nch=4, fixup='wave')),
    # V_e < 256, d_e % 4 != 0: egrad_fixup_wg<1>; runs of 19 and 71 chunks; entity 0 and the last entity absent; 2048 pairs
    'runs_wg_v1': dict(B=512, z=3, Ve=40, de=70, counts=_spread(40, 2048, [0, 300, 0, 0, 0, 0, 0, 1130, 17, 33, 1, 31], 12, 3),
                       plan=dict(path='sorted', sort_bits=6, passes=1, vec=1, nch=4, fixup='workgroup')),
    # d_e = 512: egrad_chunk_reduce<4, 8> and egrad_fixup_wg<4> with its LDS slab full; 1500 pairs (ragged last chunk)
    'runs_wg_v4_d512': dict(B=300, z=4, Ve=20, de=512, counts=_spread(20, 1500, [5, 1130, 300, 33, 0, 0, 1], 4, 2),
                            plan=dict(path='sorted', sort_bits=5, passes=1, vec=4, nch=8, fixup='workgroup')),
    # one entity takes every pair of the batch (250 chunks under egrad_fixup<4>), its neighbours absent; d_e = 384: <4, 8>
    'one_entity_d384': dict(B=1000, z=3, Ve=300, de=384, counts=_spread(300, 4000, [0] * 150, 1, 149),
                            plan=dict(path='sorted', sort_bits=9, passes=1, vec=4, nch=8, fixup='wave')),
    # d_e = 320: egrad_chunk_reduce<4, 5>
    'runs_wave_d320': dict(B=200, z=4, Ve=260, de=320, counts=_spread(260, 1000, _RUNS_A[:13], 60, 1),
                           plan=dict(path='sorted', sort_bits=9, passes=1, vec=4, nch=5, fixup='wave')),
    # V_e = 2048 forced onto the sort: 11 key bits, one pass; d_e = 64: <4, 1>
    'v2048_d64': dict(B=300, z=5, Ve=2048, de=64, counts=_scatter(2048, 1800, 11, [33, 17, 16, 65, 2, 3, 100]),
                      plan=dict(path='sorted', sort_bits=11, passes=1, vec=4, nch=1, fixup='wave')),
    # V_e = 2049: 12 key bits, two passes of 6; d_e = 128: <4, 2>
    'v2049_d128': dict(B=400, z=4, Ve=2049, de=128, counts=_scatter(2049, 2000, 12, [33, 17, 16, 65, 2, 3, 100]),
                       plan=dict(path='sorted', sort_bits=12, passes=2, vec=4, nch=2, fixup='wave')),
    # V_e = 70000: 17 key bits, passes of 9 and 8; d_e = 8
    'v70000_d8': dict(B=500, z=4, Ve=70000, de=8, counts=_scatter(70000, 2500, 13, [33, 17, 16, 65, 2, 3, 100, 300]),
                      plan=dict(path='sorted', sort_bits=17, passes=2, vec=4, nch=1, fixup='wave')),
}

# --------------------------------------------------------------------------------------------------------------------- #
# placement plans of the bucket cases
# --------------------------------------------------------------------------------------------------------------------- #
# plan: the geometry api_model.inc derives for the shape, as the hook must report it (group_sum False: a single GPU leaves the
# sum of the group tables to the optimiser, with either keep_grads).  lists: {sub-group: {range: pairs}}, the pairs of a
# sub-group that `lists` does not place fall in ranges drawn uniformly.  sorted_plan: what the same shape reports under
# SERT_EGRAD_SORT=1.
BUCKET_CASES = {
    # 32 rows x 4 pairs per sub-group; 7 ranges, the last of 4 entities; 10 sub-groups (fewer than 16, the last of 12 rows)
    'lists_v100_d128': dict(
        B=300, z=3, Ve=100, de=128,
        plan=dict(path='bucket', sub_rows=32, num_sub=10, subs_per_group=1, groups=10, ranges=7, group_sum=False),
        lists={0: {0: 128}, 1: {6: 128}, 2: {0: 1, 1: 16, 2: 17, 3: 63, 4: 31}, 3: {0: 64, 1: 64}, 4: {0: 65, 1: 63}, 9: {6: 48}},
        sorted_plan=dict(path='sorted', sort_bits=7, passes=1, vec=4, nch=2, fixup='workgroup')),
    # z = 0, one range (no match bits), d_e = 4: one lane of 64 holds columns
    'z0_v16_d4': dict(
        B=1000, z=0, Ve=16, de=4,
        plan=dict(path='bucket', sub_rows=32, num_sub=32, subs_per_group=2, groups=16, ranges=1, group_sum=False),
        lists={}, sorted_plan=dict(path='sorted', sort_bits=4, passes=1, vec=4, nch=1, fixup='workgroup')),
    # z = 20: 4096 / 21 = 195 rows, halved to 48: 1008 pairs per sub-group; 128 ranges; 65 sub-groups in 17 groups of 4 (the last
    # of one sub-group, itself of 28 rows)
    'z20_v2048_d32': dict(
        B=3100, z=20, Ve=2048, de=32,
        plan=dict(path='bucket', sub_rows=48, num_sub=65, subs_per_group=4, groups=17, ranges=128, group_sum=False),
        lists={0: {127: 129, 64: 65, 63: 64, 0: 17}, 5: {127: 1008}, 64: {100: 129}},
        sorted_plan=dict(path='sorted', sort_bits=11, passes=1, vec=4, nch=1, fixup='wave')),
    # 528 sub-groups of 256 rows in 16 groups of 33: the second trip of egrad_acc's list loop (sub-group 32 of every group)
    'deep_groups_d4': dict(
        B=135000, z=1, Ve=40, de=4,
        plan=dict(path='bucket', sub_rows=256, num_sub=528, subs_per_group=33, groups=16, ranges=3, group_sum=False),
        lists={}, sorted_plan=dict(path='sorted', sort_bits=6, passes=1, vec=4, nch=1, fixup='workgroup')),
}

CASES = dict(SORTED_CASES)
CASES.update(BUCKET_CASES)
SEEDS = {name: 300 + k for k, name in enumerate(CASES)}


def is_bucket(name):
    return name in BUCKET_CASES


def _place(rng, keys, B, c1):
    """(y (B) int32, neg (B, z) int64) holding `keys` in a seeded permutation of the B (z + 1) slots; slot (i, j) is the key of
    pair i (z + 1) + j, as the loss kernel writes cand (csrc/kernels_vs.h)."""
    assert len(keys) == B * c1, (len(keys), B, c1)
    cand = np.empty(B * c1, dtype=np.int64)
    cand[rng.permutation(B * c1)] = keys
    cand = cand.reshape(B, c1)
    return cand[:, 0].astype(np.int32), np.ascontiguousarray(cand[:, 1:])


def sorted_step_counts(c, step):
    """counts per entity of a sorted case's step: the stated ones, then the same reversed over the entities."""
    counts = np.asarray(c['counts'], dtype=np.int64)
    return counts if step == 0 else counts[::-1].copy()


def bucket_step_lists(c, step):
    """{sub-group: {range: pairs}} of a bucket case's step: the stated ones, then rotated by one sub-group (the ragged last
    sub-group keeps its own) and mirrored over the ranges."""
    if step == 0:
        return c['lists']
    g = c['plan']
    last = g['num_sub'] - 1
    ragged = c['B'] % g['sub_rows'] != 0
    out = {}
    for sg, l in c['lists'].items():
        to = sg if (ragged and sg == last) else (sg + 1) % (last if ragged else last + 1)
        out[to] = {g['ranges'] - 1 - r: k for r, k in l.items()}
    return out


def _bucket_keys(rng, c, step):
    """cand (B, z + 1) of a bucket case's step: per sub-group the placed pairs in entities drawn inside their range, the others
    in ranges drawn uniformly, permuted over the sub-group's slots."""
    g, V, c1 = c['plan'], c['Ve'], c['z'] + 1
    lists = bucket_step_lists(c, step)
    cand = np.empty((c['B'], c1), dtype=np.int64)
    for sg in range(g['num_sub']):
        lo, hi = sg * g['sub_rows'], min(c['B'], (sg + 1) * g['sub_rows'])
        npairs = (hi - lo) * c1
        placed = lists.get(sg, {})
        rid = np.concatenate([np.full(k, r, dtype=np.int64) for r, k in sorted(placed.items())] + [np.zeros(0, np.int64)])
        assert len(rid) <= npairs, (sg, len(rid), npairs)
        if len(rid) < npairs:        # the pairs the plan does not place: ranges drawn uniformly among those it does not name
            free = np.setdiff1d(np.arange(g['ranges']), list(placed))
            rid = np.concatenate([rid, free[rng.randint(0, len(free), size=npairs - len(rid))]])
        width = np.minimum(RANGE, V - rid * RANGE)
        keys = rid * RANGE + (rng.randint(0, 1 << 30, size=npairs) % width)
        cand[lo:hi] = keys[rng.permutation(npairs)].reshape(hi - lo, c1)
    return cand


_cache = {}


def case_problem(name):
    """(case dict, problem) of a case, built once per process; treat both as read-only.  problem: the dict of
    util.make_vs_problem over STEPS batches, with y (STEPS * B) and neg = [neg of step 0, neg of step 1] from the case's plans."""
    if name not in _cache:
        c = CASES[name]
        B, z, c1 = c['B'], c['z'], c['z'] + 1
        p = U.make_vs_problem(SEEDS[name], B * STEPS, N, max(z, 1), VW, c['Ve'], DW, c['de'])
        rng = np.random.RandomState(SEEDS[name] + 1000)
        ys, negs = [], []
        for s in range(STEPS):
            if is_bucket(name):
                cand = _bucket_keys(rng, c, s)
                y, neg = cand[:, 0].astype(np.int32), np.ascontiguousarray(cand[:, 1:])
            else:
                counts = sorted_step_counts(c, s)
                y, neg = _place(rng, np.repeat(np.arange(c['Ve'], dtype=np.int64), counts), B, c1)
            ys.append(y)
            negs.append(neg)
        p['y'] = np.concatenate(ys)
        p['neg'] = negs
        for a in list(p.values()) + negs:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, p)
    return _cache[name]


def step_keys(name, step):
    """cand (B, z + 1) int64 of a step: column 0 the labels, the others the negatives."""
    c, p = case_problem(name)
    B = c['B']
    return np.concatenate([p['y'][step * B:(step + 1) * B, None].astype(np.int64), p['neg'][step]], axis=1)


def step_counts(name, step):
    c, _ = case_problem(name)
    return np.bincount(step_keys(name, step).ravel(), minlength=c['Ve'])


_refs = {}


def case_reference(name, dtype):
    """The oracle's run of a case in `dtype`, computed once per process and shared: ([dR_e of step 0, dR_e of step 1], the oracle
    after the last step)."""
    key = (name, np.dtype(dtype).name)
    if key not in _refs:
        c, p = case_problem(name)
        B = c['B']
        ora = O.VectorSpaceOracle(B, N, c['z'], p['Rw'], p['Re'], p['W'], p['b'], LAM, dtype=dtype)
        grads = []
        for s in range(STEPS):
            sl = slice(s * B, (s + 1) * B)
            _, g, _ = ora.loss_and_grads(p['X'][sl], p['y'][sl], p['w'][sl], p['neg'][s])
            g[0].setflags(write=False)
            grads.append(g[0])
            ora.opt.update(ora.params(), g)
        _refs[key] = (grads, ora)
    return _refs[key]


# --------------------------------------------------------------------------------------------------------------------- #
# the events a case produces
# --------------------------------------------------------------------------------------------------------------------- #

def sorted_events(counts, Ve, de, plan):
    """The SORTED_EVENTS that one step with these counts per entity produces under the stated plan -- from the counts, CHUNK and
    the plan alone: the sort is stable, so entity e's run is [sum(counts[:e]), sum(counts[:e + 1]))."""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    end = np.cumsum(counts)
    start = end - counts
    here = counts > 0
    s, t, L = start[here], end[here], counts[here]
    slot = s % CHUNK
    nchunks = (t - 1) // CHUNK - s // CHUNK + 1
    ev = set()

    def put(name, cond):
        if bool(np.any(cond)):
            ev.add(name)

    put('run1_first_slot', (L == 1) & (slot == 0))
    put('run1_last_slot', (L == 1) & (slot == CHUNK - 1))
    put('run16_aligned', (L == 16) & (slot == 0))
    put('run16_unaligned', (L == 16) & (slot != 0))
    put('run32_aligned', (L == 32) & (slot == 0))
    for k in (15, 17, 31, 33):
        put('run%d' % k, L == k)
    put('run17_from_last_slot', (L == 17) & (slot == CHUNK - 1))
    put('run_ends_at_chunk_end_from_earlier_chunk', (t % CHUNK == 0) & (nchunks >= 2))
    put('run_over_3_chunks', nchunks >= 3)
    if plan['fixup'] == 'wave':
        put('fixup_wave_6_chunks', nchunks >= 6)
        put('fixup_wave_70_chunks', nchunks >= 70)
    else:
        put('fixup_wg_18_chunks', nchunks >= 18)
        put('fixup_wg_70_chunks', nchunks >= 70)
    e = np.nonzero(here)[0]
    put('one_entity_takes_all', len(e) == 1 and 0 < e[0] < Ve - 1)
    put('entity0_absent', counts[0] == 0)
    put('last_entity_absent', counts[-1] == 0)
    put('last_entity_present', counts[-1] > 0)
    gaps = np.diff(np.concatenate([[-1], e, [Ve]])) - 1
    put('absent_stretch_5', gaps >= 5)
    put('total_mod16_zero', total % CHUNK == 0)
    put('total_mod16_nonzero', total % CHUNK != 0)
    put('total_below_tile', total < SORT_TILE)
    put('total_2048', total == SORT_TILE)
    put('total_2049', total == SORT_TILE + 1)
    put('total_above_tile', total > SORT_TILE + 1)
    bits, passes = plan['sort_bits'], plan['passes']
    put('Ve2048_11bits_1pass', Ve == 2048 and (bits, passes) == (11, 1))
    put('Ve2049_12bits_2passes', Ve == 2049 and (bits, passes) == (12, 2))
    put('Ve_17bits_unequal_passes', bits == 17 and passes == 2 and (1 << 16) < Ve and e[-1] >= (1 << 16))
    vn = (plan['vec'], plan['nch'])
    put('reduce_4_1', vn == (4, 1) and de % 4 == 0 and de <= 64)
    put('reduce_4_2', vn == (4, 2) and de % 4 == 0 and 64 < de <= 128)
    put('reduce_4_5', vn == (4, 5) and de % 4 == 0 and 128 < de <= 320)
    put('reduce_4_8_de384', vn == (4, 8) and de == 384)
    put('reduce_4_8_de512', vn == (4, 8) and de == 512)
    put('reduce_1_4_second_column_pass', vn == (1, 4) and de % 4 != 0 and de > 64)
    put('fixup_%s_vec%d' % ('wave' if plan['fixup'] == 'wave' else 'wg', plan['vec']), True)
    put('fixup_wg_vec4_de512', plan['fixup'] == 'workgroup' and plan['vec'] == 4 and de == 512)
    return ev


def bucket_list_lengths(cand, sub_rows, ranges):
    """(sub-groups, ranges): how many pairs of each sub-group of `sub_rows` rows of cand (B, z + 1) fall in each range of 16
    entities -- the lengths of the lists egrad_bucket leaves and egrad_acc walks."""
    B, c1 = cand.shape
    num_sub = -(-B // sub_rows)
    sg = np.repeat(np.arange(B) // sub_rows, c1)
    flat = sg * ranges + (cand.ravel() // RANGE)
    return np.bincount(flat, minlength=num_sub * ranges).reshape(num_sub, ranges)


def bucket_events(cand, Ve, de, plan):
    """The BUCKET_EVENTS that one step with these keys produces under the geometry of `plan` (stated or reported)."""
    B, c1 = cand.shape
    g = plan
    ln = bucket_list_lengths(cand, g['sub_rows'], g['ranges'])
    ev = set()

    def put(name, cond):
        if bool(np.any(cond)):
            ev.add(name)

    for k in (0, 1, 16, 17, 63, 64, 65):
        put('list%d' % k, ln == k)
    put('list129', ln >= 129)
    pairs = ln.sum(axis=1)
    put('sub_group_in_one_range', (ln.max(axis=1) == pairs) & (g['ranges'] > 1))
    put('sub_group_in_last_range', (ln[:, -1] == pairs) & (g['ranges'] > 1))
    put('Ve_le_16', Ve <= RANGE and g['ranges'] == 1)
    put('Ve_ragged_last_range', Ve % RANGE != 0 and ln[:, -1].sum() > 0)
    put('Ve2048_128_ranges', Ve == 2048 and g['ranges'] == 128 and ln[:, 64:].sum() > 0)
    put('ragged_last_sub_group', B % g['sub_rows'] != 0)
    put('ragged_last_group', g['num_sub'] % g['subs_per_group'] != 0)
    put('fewer_sub_groups_than_16', g['num_sub'] < 16)
    put('z0', c1 == 1)
    full = g['sub_rows'] * c1
    put('sub_pairs_not_power_of_two', (4096 // c1) * c1 != 4096 and 4096 // c1 < 256 and full & (full - 1) != 0)
    put('subs_per_group_gt_32', g['subs_per_group'] > 32)
    put('de4', de == 4)
    put('de128', de == 128)
    return ev


def events_of(name, step=0, plan=None):
    """The events step `step` of a case produces; `plan`: the reported one in place of the stated one."""
    c, _ = case_problem(name)
    plan = c['plan'] if plan is None else plan
    if is_bucket(name):
        return bucket_events(step_keys(name, step), c['Ve'], c['de'], plan)
    return sorted_events(step_counts(name, step), c['Ve'], c['de'], plan)
