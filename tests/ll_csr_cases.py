"""Loglinear problems whose only difficulty is the STRUCTURE of their CSR label rows -- shared by the CPU proof of the
inputs (test_ll_csr_inputs_cpu.py) and the GPU test (test_gpu_ll_csr.py).

The loss kernels of the loglinear step handle a row's label entries in four ways (csrc/kernels_ll.h): ll_row_wave serially on
the entry's owner lane; ll_row_from_table and ll_fused_row in per-thread registers, kLlFusedLabels / NT entries a thread;
the streaming kernels through memory (ll_s_rowloss -> labfix -> ll_s_labfix), which is also where a split goes whose
longest row exceeds kLlFusedLabels.  The count plans below stand on the edges of those mechanisms: 0 (an empty row) and
V_e (a full one), 128 / 129 (a thread of a 128-thread row takes its second label), 512 / 513 (the fifth), 1024 / 1025
(the host's bound), and 4097 labels over three 4096-element segments.

Everything else is kept tame on purpose: Glorot-scale parameters, no probability anywhere near a clip bound (the CPU test
proves it), so engine and oracle cannot differ by an fp32 mask decision."""
import numpy as np

from oracle import sert_oracle as O
from tests import util as U

B, VW, D, STEPS, LAM = 8, 120, 16, 2, 0.01
LABEL_LIMIT = 1024          # csrc/kernels_ll.h: kLlFusedLabels

# id -> n, V_e, label counts of the rows of one batch (repeated for every batch), the form the TRAINING step must reach as
# Engine.ll_loss_form() reports it, the forms of eval_batch on the training split (distinct-word table) and on the
# validation split (per token), and the standard deviation of the bias.
# b_std: make_ll_problem's 0.1 everywhere but in `fusedrow` -- J_e sums n = 65 log-probabilities, 65 b_e among them, and
# Q = softmax(J) over a 0.1-wide bias is a softmax over N(0, 6.5^2): some Q_e above 0.5 and most below 1e-7, i.e.
# clipped.  0.1 * 3 / 65 gives its J the spread the n = 3 cases have.  b_mean: a bias that narrow would be a tensor of
# magnitude 0.014 with a gradient of magnitude 0.4, and the parameter bound (relative to max |b|) would ask 30 times
# more of db than the gradient bound does; the common offset 0.3 -- which every softmax ignores -- gives b the magnitude
# it has in the other cases (max |0.1 randn| over a few hundred entities).
CASES = {
    'wave1': dict(n=3, Ve=256, counts=(0, 1, 2, 64, 65, 255, 256, 3),
                  train=('wave', 1), ev_train=('fused_row', 512), ev_valid=('fused_row', 512)),
    'wave8': dict(n=3, Ve=1028, counts=(1024, 1000, 513, 512, 0, 1, 700, 4),
                  train=('wave', 8), ev_train=('fused_row', 512), ev_valid=('fused_row', 512)),
    'table128_small': dict(n=3, Ve=601, counts=(601, 600, 513, 512, 0, 1, 5, 300),
                           train=('table', 128), ev_train=('fused_row', 512), ev_valid=('fused_row', 512)),
    'table128_limit': dict(n=3, Ve=1026, counts=(4, 128, 129, 512, 513, 640, 1023, 1024),
                           train=('table', 128), ev_train=('fused_row', 512), ev_valid=('fused_row', 512)),
    'table512': dict(n=3, Ve=2050, counts=(1024, 1023, 513, 512, 1, 0, 3, 800),
                     train=('table', 512), ev_train=('fused_row', 512), ev_valid=('fused_row', 512)),
    'fusedrow': dict(n=65, Ve=300, counts=(0, 1, 4, 5, 128, 299, 300, 17), b_std=0.1 * 3 / 65, b_mean=0.3,
                     train=('fused_row', 512), ev_train=('fused_row', 512), ev_valid=('fused_row', 512)),
    'fallback_scalar': dict(n=3, Ve=1026, counts=(1025, 1, 0, 4, 513, 2, 3, 5),
                            train=('stream', 0), ev_train=('stream', 0), ev_valid=('stream', 0), segments=1),
    'fallback_v4': dict(n=3, Ve=1028, counts=(1025, 1, 0, 4, 513, 2, 3, 5),
                        train=('stream', 1), ev_train=('stream', 1), ev_valid=('stream', 1), segments=1),
    'stream': dict(n=4, Ve=9001, counts=(4097, 1025, 0, 1),
                   train=('stream', 0), ev_train=('stream', 0), ev_valid=('stream', 0), segments=3),
}
SEEDS = {name: 100 + k for k, name in enumerate(CASES)}


def make_ll_csr_problem(seed, counts, n, Vw, Ve, d, steps=STEPS, b_std=0.1, b_mean=0.0, unnormalised_row=None, zero_entry=True):
    """The dict of util.make_ll_problem for rows with the given label counts, the plan repeated `steps` times.
    Columns: np.sort(rng.choice(Ve, k, replace=False)); values: uniform in [0.5, 1.5), the row normalised to sum 1.
    Two deliberate exceptions, in the first batch: the row `unnormalised_row` (default: the first with at least two labels)
    is scaled to sum 2.5, and -- zero_entry -- the middle entry of the LAST row with at least two labels other than that one
    is a stored 0.0 (the row is not renormalised).  Also returned: `counts` per row, `zero_at` = (row, column)."""
    import scipy.sparse as sp
    rng = np.random.RandomState(seed)
    Bc = len(counts)
    N = Bc * steps
    Rw = O.glorot_uniform(rng, (Vw, d))
    W = O.glorot_uniform(rng, (d, Ve))
    b = (b_mean + b_std * rng.randn(Ve)).astype(np.float32)
    X = rng.randint(0, Vw, size=(N, n)).astype(U.id_dtype(Vw))
    w = rng.uniform(0.5, 2.0, N).astype(np.float32)
    multi = [i for i, k in enumerate(counts) if k >= 2]
    if unnormalised_row is None and multi:
        unnormalised_row = multi[0]
    zero_row = next((i for i in reversed(multi) if i != unnormalised_row), None) if zero_entry else None
    indptr, indices, data, zero_at = [0], [], [], None
    for r in range(N):
        k = int(counts[r % Bc])
        cols = np.sort(rng.choice(Ve, k, replace=False))
        vals = rng.uniform(0.5, 1.5, k)
        if k:
            vals = vals / vals.sum()
        if r == unnormalised_row:
            vals = vals * 2.5
        if r == zero_row:
            vals[k // 2] = 0.0
            zero_at = (r, int(cols[k // 2]))
        indices += cols.tolist()
        data += vals.tolist()
        indptr.append(len(indices))
    # (built from the three arrays: nothing is summed, sorted or pruned -- the stored zero stays stored)
    y = sp.csr_matrix((np.array(data, dtype=np.float32), np.array(indices, dtype=np.int32),
                       np.array(indptr, dtype=np.int64)), shape=(N, Ve))
    ydense = np.asarray(y.todense(), dtype=np.float32)
    return dict(Rw=Rw, W=W, b=b, X=X, y=y, ydense=ydense, w=w, rng=rng, counts=np.diff(y.indptr),
                unnormalised_row=unnormalised_row, zero_at=zero_at)


_cache = {}


def case_problem(name):
    """(case dict, problem) of a case, built once per process; treat both as read-only."""
    if name not in _cache:
        c = CASES[name]
        p = make_ll_csr_problem(SEEDS[name], c['counts'], c['n'], VW, c['Ve'], D, b_std=c.get('b_std', 0.1),
                                b_mean=c.get('b_mean', 0.0))
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, p)
    return _cache[name]


_refs = {}


def case_reference(name, dtype):
    """The oracle's run of a case in `dtype`, computed once per process and shared: a list with, per step, dict(loss,
    grads = [dR_w, dW, db], f = the forward's intermediates and dJ) and the oracle after the last step."""
    key = (name, np.dtype(dtype).name)
    if key not in _refs:
        c, p = case_problem(name)
        Bc = len(c['counts'])
        ora = O.LogLinearOracle(Bc, c['n'], p['Rw'], p['W'], p['b'], LAM, dtype=dtype)
        steps = []
        for s in range(STEPS):
            sl = slice(s * Bc, (s + 1) * Bc)
            loss, grads, f = ora.loss_and_grads(p['X'][sl], p['ydense'][sl], p['w'][sl])
            steps.append(dict(loss=loss, grads=[np.array(g, copy=True) for g in grads], f=f))
            ora.opt.update(ora.params(), grads)
        _refs[key] = (steps, ora)
    return _refs[key]
