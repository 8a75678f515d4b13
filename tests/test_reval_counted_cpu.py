"""CPU: the host half of the evaluator by rank counting (sert_reval_create_counted) -- evaluation.metrics_from_ranks, the
definition the device kernel restates, against evaluation.host_metrics on explicit rankings; which handle
RetrievalEvaluator picks; the new header against the binding; bin/train.py --eval_top above 1024."""
import os
import re

import numpy as np
import pytest

from sert_amd import _capi, evaluation
from tests import test_gpu_reval as R          # (its helpers, as a module: _judgements)
from tests import test_reval_cpu as RC         # (_train_cli)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9          # the evaluator's bound (tests/test_gpu_reval.py): float64 sums of <= 1e5 terms, every metric <= 1
SIZES = (1, 2, 3, 5, 6, 7, 9, 64, 257, 400)


@pytest.mark.parametrize('V', SIZES)
def test_metrics_from_ranks_equal_host_metrics_on_the_ranking(V):
    """Random permutations of V entities as rankings, the eight judgement patterns of _judgements (unknown entities, zero
    and negative gains, lists longer than the depth, the entity at the last rank) built around each depth's cut; depths 1,
    4, 5, 6, V - 1, V (those above V evaluate every entity, as the evaluator clips them; V - 1 = 0 is no depth)."""
    rng = np.random.RandomState(100 + V)
    ranking = np.stack([rng.permutation(V) for _ in range(16)])           # (two rounds of the eight patterns)
    rank_of = np.empty_like(ranking)
    rank_of[np.arange(16)[:, None], ranking] = np.arange(1, V + 1)[None, :]
    worst, seen = 0.0, 0
    for depth in sorted(set(min(d, V) for d in (1, 4, 5, 6, V - 1, V) if d >= 1)):
        rels = R._judgements(rng, ranking[:, :depth], V)
        for q, rel in enumerate(rels):
            known = sorted((e, g) for e, g in rel.items() if e < V)
            ranks = [int(rank_of[q, e]) for e, _ in known]
            gains = [g for _, g in known]
            got = evaluation.metrics_from_ranks(ranks, gains, depth, evaluation.ideal_dcg(rel, depth),
                                                sum(1 for g in rel.values() if g > 0))
            want = evaluation.host_metrics([int(e) for e in ranking[q]], rel, depth)
            assert sorted(got) == sorted(evaluation.METRICS)
            for name in evaluation.METRICS:
                worst = max(worst, abs(got[name] - want[name]))
                assert abs(got[name] - want[name]) <= TOL, (V, depth, q, name, got[name], want[name])
            seen += 1
    assert seen >= 16
    print('V=%d: %d topic evaluations, largest difference %.3g' % (V, seen, worst))


def test_metrics_from_ranks_by_hand():
    # ranks 2 (gain 1), 3 (gain 0), 5 (gain 2), 9 (gain -1), depth 5: the entity at rank 9 is outside
    got = evaluation.metrics_from_ranks([3, 2, 9, 5], [0.0, 1.0, -1.0, 2.0], 5, 2.5, 4)
    assert abs(got['ndcg'] - (1.0 / np.log2(3) + 2.0 / np.log2(6)) / 2.5) < 1e-15
    assert abs(got['map'] - (1.0 / 2 + 2.0 / 5) / 4) < 1e-15
    assert got['recip_rank'] == 0.5 and got['P_5'] == 2.0 / 5 and got['num_rel_ret'] == 2.0
    # a negative gain inside the depth is added to the DCG and is no hit; no ideal DCG, no relevant entity: zeros
    got = evaluation.metrics_from_ranks([1], [-1.0], 3, 1.0, 1)
    assert got['ndcg'] == -1.0 and got['map'] == 0.0 and got['recip_rank'] == 0.0 and got['num_rel_ret'] == 0.0
    assert evaluation.metrics_from_ranks([1], [1.0], 3, 0.0, 0) == dict(evaluation.ZERO, num_rel_ret=1.0, P_5=0.2, recip_rank=1.0)
    assert evaluation.metrics_from_ranks([], [], 3, 1.0, 2) == evaluation.ZERO


def test_which_handle_the_evaluator_makes():
    """Counted exactly where sert_reval_create refuses a vectorspace model; every other case keeps its handle."""
    vs, fs, ll = _capi.KIND_VECTORSPACE, _capi.KIND_VECTORSPACE_SOFTMAX, _capi.KIND_LOGLINEAR
    for kind in (vs, fs):
        assert evaluation.uses_counting(kind, None, 500) and evaluation.uses_counting(kind, 1025, 5000)
        assert evaluation.uses_counting(kind, 501, 500) and evaluation.uses_counting(kind, 5000, 338)
        assert not evaluation.uses_counting(kind, 1024, 5000) and not evaluation.uses_counting(kind, 500, 500)
        assert not evaluation.uses_counting(kind, 100, 5000) and not evaluation.uses_counting(kind, 1, 1)
    for k in (None, 1, 100, 1025, 10 ** 6):
        assert not evaluation.uses_counting(ll, k, 500)


def test_header_and_binding_agree_on_the_counted_entry_points(hip_lib):
    with open(os.path.join(ROOT, 'include', 'sert_hip_reval_counted.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(sert_[a-z_0-9]+)\s*\(', src)))
    assert declared == sorted(_capi.EXPORTS_REVAL_COUNTED) == ['sert_reval_create_counted', 'sert_reval_judged_ranks']
    assert not [s for s in declared if not hasattr(hip_lib, s)]
    with open(os.path.join(ROOT, 'include', 'sert_hip.h')) as f:
        assert '#include "sert_hip_reval_counted.h"' in f.read()          # (one boundary: sert_hip.h brings it in)
    with open(os.path.join(ROOT, 'include', 'sert_hip_debug.h')) as f:
        assert 'sert_debug_count_ranks' in f.read() and 'sert_debug_count_ranks' in _capi.EXPORTS


def test_eval_top_above_1024_parses(tmp_path):
    cli = RC._train_cli()
    for name in ('data', 'meta', 'topics', 'qv'):
        (tmp_path / name).write_text('x')
    args = cli.build_parser().parse_args(['--data', str(tmp_path / 'data'), '--meta', str(tmp_path / 'meta'), '--type',
                                          'vectorspace', '--model_output', 'm', '--eval_topics', str(tmp_path / 'topics'),
                                          '--eval_qrels', 'validation=' + str(tmp_path / 'qv'), '--eval_top', '5000'])
    assert args.eval_top == 5000
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--data', str(tmp_path / 'data'), '--meta', str(tmp_path / 'meta'), '--type',
                                       'vectorspace', '--model_output', 'm', '--eval_top', '0'])
