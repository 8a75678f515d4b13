"""-m gpu: the step's streaming outputs at the edges of every store that may be written through (common.h: store16).

The gather's H, the loss kernel's DA, the word-gradient tree's final, partial and heavy-word rows, the word-table update's
p, m and v and the entity gradient's partial tables go out through one helper whose flavour -- plain, nt or the 16-byte
write-through buffer store -- is a compile-time choice per kernel family (SERT_WT_STORES).  A buffer store takes a
wave-uniform base and a 32-bit lane offset and its descriptor guards nothing, so what can go wrong is a lane that stores
where it did not before (ragged row blocks, column groups past d) or an offset formed from the wrong base.  Every case
below is a few vectorspace steps against the oracle: per-step loss to 1e-5, every parameter and both moments with the
bounds of tests/util.py (check_state), and the host counters say which kernel forms ran.  The library under test is
whatever mask the build chose; a variants build (tools/build_variant.sh NAME -DSERT_WT_STORES=0x3f, SERT_LIB=...) runs
the same file over every write-through store at once."""
import numpy as np
import pytest

from oracle import philox
from oracle import sert_oracle as O
from sert_amd import _capi as C
from tests import util as U

pytestmark = pytest.mark.gpu

SEED = 4321
LOSS_TOL = 1e-5


def run_steps(p, B, n, z, lam, plan, reads=()):
    """Train plan = [(batch, hint or None), ...] in the product configuration (keep_grads = 0); reads: steps behind which
    the word table is read (a flush of the rows that are behind).  Returns losses, the state dict and the counters."""
    eng = U.vs_engine(p, B, n, z, lam, keep_grads=0, seed=SEED)
    eng.upload_dataset(C.SPLIT_TRAIN, p['X'], y_int=p['y'], w=p['w'])
    losses = []
    for s, (b, hint) in enumerate(plan):
        if hint is not None:
            eng.hint_next_batch(hint)
        losses.append(eng.train_batch(b))
        if s in reads:
            assert np.all(np.isfinite(eng.get_tensor(C.T_RW)))
    state = U.engine_state(eng)
    counts = (eng.tail_counts(), eng.update_counts())
    eng.close()
    return losses, state, counts


def oracle_run(p, B, n, z, lam, plan):
    Ve = p['Re'].shape[0]
    ora = O.VectorSpaceOracle(B, n, z, p['Rw'], p['Re'], p['W'], p['b'], lam)
    refs = []
    for s, (b, _) in enumerate(plan):
        sl = slice(b * B, (b + 1) * B)
        refs.append(ora.train_step(p['X'][sl], p['y'][sl], p['w'][sl], philox.training_negatives(SEED, s, B, z, Ve)))
    return refs, ora


def oracle_steps(p, B, n, z, lam, plan):
    """Per-step losses and the final state of the oracle, as copies that nothing shares with the oracle object."""
    refs, ora = oracle_run(p, B, n, z, lam, plan)
    return tuple(refs), {k: np.array(v, copy=True) for k, v in U.oracle_state(ora).items()}


def check(losses, state, refs, ref_state):
    for s, (got, ref) in enumerate(zip(losses, refs)):
        assert abs(got - ref) <= LOSS_TOL * abs(ref), (s, got, ref)
    print('\n'.join(U.check_state(state, ref_state)))


# ---- small tables: the plain gather and the one that carries the tail, the loss kernel's rows, adam_l2 -----------------
# B = 17: one ragged 16-row block of the loss kernel and a last wave of the gather that is mostly idle; 130: nine blocks,
# the last with two rows.  d_w = 4: one 16-byte piece per row (sixteen rows per wave-instruction of the gather); 36: rows
# that straddle the waves of the gather; 128: C2's; 300: three column groups in the tree, the last ragged.  d_e = 4 / 128:
# one lane of sixteen / every lane stores a piece of DA.
PLAN3 = [(0, 1), (1, 2), (2, None)]
_ref_cache = {}


@pytest.mark.parametrize('hinted', [False, True], ids=['unhinted', 'hinted'])
@pytest.mark.parametrize('de', [4, 128])
@pytest.mark.parametrize('dw', [4, 36, 128, 300])
@pytest.mark.parametrize('B', [17, 130])
def test_three_steps_at_the_edges_of_the_row_stores(hip_lib, B, dw, de, hinted):
    n, z, Vw, Ve, lam = 3, 3, 400, 50, 0.05
    key = (B, dw, de)
    p = U.make_vs_problem(61, B * 3, n, z, Vw, Ve, dw, de, zipf=True)
    plan = PLAN3 if hinted else [(b, None) for b, _ in PLAN3]
    losses, state, (tails, upd) = run_steps(p, B, n, z, lam, plan)
    if hinted:      # every hinted step's tail leads the next gather launch; the last step's is launched alone
        assert tails == {'alone': 1, 'in_gather': 2}, tails
    else:
        assert tails == {'alone': 3, 'in_gather': 0}, tails
    assert upd['dense'] == 3 and sum(v for k, v in upd.items() if k != 'dense') == 0, upd      # (a small table: adam_l2)
    if key not in _ref_cache:       # (one oracle run serves both schedules: losses and copies of its arrays, read only)
        _ref_cache[key] = oracle_steps(p, B, n, z, lam, PLAN3)
    check(losses, state, *_ref_cache[key])


# ---- a table just above 2^22 elements: dense_update_skip (full and sparse passes) and the flush (dense_update_lazy) -----
def test_lazy_update_full_sparse_and_flush_above_the_table_threshold(hip_lib):
    B, n, z, Vw, Ve, dw, de, lam = 130, 3, 3, 32769, 50, 128, 128, 0.05
    assert Vw * dw > 1 << 22 and (Vw - 1) * dw <= 1 << 22
    p = U.make_vs_problem(62, B * 4, n, z, Vw, Ve, dw, de, zipf=True)
    p['X'][-1, -1] = Vw - 1            # (the table's last row is touched: the last piece of p, m and v is written)
    plan = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 1), (1, None), (2, 3), (3, None)]
    losses, state, (tails, upd) = run_steps(p, B, n, z, lam, plan, reads=(2,))
    assert upd['skip_32_1'] == len(plan) and upd['dense'] == 0, upd
    assert upd['skip_sparse'] >= 3 and upd['skip_full'] >= 2, upd
    # (the flush -- dense_update_lazy with update = 0, not among the counters -- runs in front of the table read behind step 2,
    #  a sparse pass that left rows behind, and in front of the state reads at the end)
    check(losses, state, *oracle_steps(p, B, n, z, lam, plan))


# ---- the tree's partial rows: a word in more than one 64-entry chunk, a heavy word, ragged last row blocks --------------
@pytest.mark.parametrize('case', ['chunked', 'heavy'])
def test_words_with_many_occurrences_and_a_ragged_last_row_block(hip_lib, case):
    # chunked: 200 of a batch's 390 tokens are one word (four chunk items -> partial rows, summed by level 1), 70 another
    # (two).  heavy: 4300 of 4500 tokens are one word (>= 4096: the dense heavy-word pass and its per-block partial rows;
    # 1500 rows = five 256-row blocks and 220 rows).  d_w = 300: three column groups, the last 11 pieces wide.
    B, n = (130, 3) if case == 'chunked' else (1500, 3)
    z, Vw, Ve, dw, de, lam = 3, 500, 50, 300, 4, 0.05
    p = U.make_vs_problem(63, B * 2, n, z, Vw, Ve, dw, de)
    rng = np.random.RandomState(64)
    for b in range(2):
        flat = p['X'][b * B:(b + 1) * B].reshape(-1)
        pos = rng.permutation(flat.size)
        if case == 'chunked':
            flat[pos[:200]] = 7
            flat[pos[200:270]] = 399
        else:
            flat[pos[:4300]] = 7
            flat[pos[4300:4400]] = 399
    plan = [(0, 1), (1, 0), (0, None)]
    losses, state, _ = run_steps(p, B, n, z, lam, plan)
    check(losses, state, *oracle_steps(p, B, n, z, lam, plan))
