"""The schedules of the vectorspace training step, pinned: facts (sert_amd._capi.VS_FACTS) and the plan csrc/step_plan.h must
decide for them (sert_amd._capi.vs_plan_for's dict).  tests/test_step_plan_cpu.py evaluates every case without a GPU,
tests/test_gpu_step_plan.py runs steps at small shapes and asserts that the engine issued the plan of its case.

The expectations are stated by hand, case by case, from the schedule each case is meant to take (DESIGN.md section 3 and the
comments of csrc/step_plan.h) -- never copied from the plan function's output."""

KIND_LOGLINEAR, KIND_VECTORSPACE, KIND_SOFTMAX = 0, 1, 2


def facts(**over):
    """Case A: single GPU, two queues, V_e = 1000, d = 128 (the sort-free entity chain), batch 8192, this step's negatives
    drawn during the previous step, the next step's not yet."""
    f = dict(kind=KIND_VECTORSPACE, nstreams=2, n_re=1000 * 128, batch=8192, word_dim=128, entity_dim=128, num_negatives=10,
             has_entities=1, sort_free=1, cand_early=1, neg_side_ready=1, has_labels=1, next_neg_drawn=0)
    f.update(over)
    return f


def plan(base, **over):
    p = dict(base)
    unknown = set(over) - set(p)
    assert not unknown, unknown
    p.update(over)
    return p


# everything on the main queue, nothing carried, no join: a loglinear step, and what the struct holds before the first step
DEFAULT = dict(fork_at='none', fork_carried=False, fork_recorded=False, dh_event='none', dh_carried=False,
               order=('entity', 'dense', 'dh', 'word_sum'), entity_queue='main', dense_queue='main', side_meets_fork=False,
               entity_waits_fork=False, dense_event='none', bwd_fused=False, bucket_early=False, sort_early=False,
               draw_next_neg=False, lazy_join=False, end_join=False, dp_late_join=False, combine_in_tail=False,
               re_in_parts=False, side_small=False, small_order='none', split_small=False, defer_re=False, defer_small=False,
               re_on_side=False)

# A: the late fork -- the dh GEMM's own completion is the step's one fork; dW / db first on the side queue (marked by ev_dense, which
# the tail waits for), the entity chain behind them with no event of its own; the next negatives in front of the fork wait; the
# main queue never joins; R_e alone on the side queue, not joined by the tail
A = plan(DEFAULT, fork_at='dh', fork_carried=True, dh_event='ev_fork', dh_carried=True, order=('dh', 'dense', 'entity', 'word_sum'),
         entity_queue='side', dense_queue='side', dense_event='ev_dense', draw_next_neg=True, lazy_join=True,
         combine_in_tail=True, re_in_parts=True, side_small=True, defer_small=True)
# ... with dW / db on the main queue behind the entity chain (dh above 24 MB, SERT_DW_FIRST=0)
A_DW_MAIN = plan(A, order=('dh', 'entity', 'dense', 'word_sum'), dense_queue='main', dense_event='none')
# B: side-heavy -- forked on the loss kernel's completion; the dh GEMM's completion is ev_dense, which the update waits for
B = plan(A, fork_at='loss', dh_event='ev_dense', order=('entity', 'dh', 'word_sum', 'dense'), entity_waits_fork=True,
         dense_event='none', draw_next_neg=False, small_order='ev_dense', defer_small=False)
# C: one queue -- ev_fork is still recorded at the head of the entity chain, nobody waits for it
C = plan(DEFAULT, fork_recorded=True, combine_in_tail=True, re_in_parts=True)
# D: R_e above 2^22 elements -- side-heavy with the sorted chain, its sort beside the forward, R_e streaming behind the tail
D_FACTS = dict(n_re=40000 * 128, big_re=1, sort_free=0)
D = plan(B, sort_early=True, re_in_parts=False, defer_re=True, re_on_side=True)
# ... SERT_SIDE_HEAVY=0: forked on the loss kernel, dW beside the sort on the main queue, joined at the end of the backward, the
# update forked and joined around the small tensors
D_PLAIN = plan(DEFAULT, fork_at='loss', fork_carried=True, entity_queue='side', entity_waits_fork=True, sort_early=True, end_join=True,
               combine_in_tail=True, side_small=True, small_order='ev_opt_fork')
# F: the product-search shape -- late fork, the sorted chain alone on the side queue, dW on the main queue
F_FACTS = dict(batch=4096, word_dim=300, entity_dim=128, n_re=32768 * 128, sort_free=0)
F = plan(A_DW_MAIN, sort_early=True, draw_next_neg=False, re_in_parts=False)
# G: three queues -- dW on the third, which meets ev_fork and records ev_join3; both side queues joined at the end
G = plan(DEFAULT, fork_at='loss', fork_carried=True, entity_queue='side', dense_queue='third', entity_waits_fork=True,
         dense_event='ev_join3', end_join=True, re_in_parts=True, side_small=True, small_order='ev_opt_fork')
# SERT_FORK_LATE=0: forked on the loss kernel, dW on the main queue, the dh GEMM's completion is ev_dense
EARLY_FORK = plan(A, fork_at='loss', dh_event='ev_dense', order=('entity', 'dense', 'dh', 'word_sum'), dense_queue='main',
                  entity_waits_fork=True, dense_event='none', draw_next_neg=False, small_order='ev_dense', defer_small=False)
# data parallel: the word-table gradient in front of dW; the main queue joins (host transport) ...
DP_HOST = plan(DEFAULT, fork_at='loss', fork_carried=True, order=('entity', 'dh', 'word_sum', 'dense'), entity_queue='side',
               entity_waits_fork=True, end_join=True)
# ... or the communication queue does (a communicator): dW first on the side queue, which meets the fork in front of it
DP_COMM = plan(DP_HOST, order=('dh', 'dense', 'entity', 'word_sum'), dense_queue='side', side_meets_fork=True, end_join=False,
               dp_late_join=True)

CASES = {
    'A': (facts(), A),
    'A_batch_32768': (facts(batch=32768), plan(A, bucket_early=True)),
    'A_batch_32768_first_step': (facts(batch=32768, neg_side_ready=0), A),
    'A_next_negatives_drawn': (facts(next_neg_drawn=1), plan(A, draw_next_neg=False)),
    'A_dh_above_24MB': (facts(word_dim=1024), A_DW_MAIN),
    'A_dh_above_24MB_batch_32768': (facts(word_dim=256, batch=32768), plan(A, bucket_early=True)),
    'B_side_heavy_2': (facts(k_side_heavy=2), B),
    'C_one_queue': (facts(nstreams=1), C),
    'D_big_entity_table': (facts(**D_FACTS), D),
    'D_first_step': (facts(neg_side_ready=0, **D_FACTS), plan(D, sort_early=False)),
    'D_dh_63MB': (facts(word_dim=2016, **D_FACTS), D),
    'D_dh_64MB': (facts(word_dim=2048, **D_FACTS), plan(D, sort_early=False)),
    'D_side_heavy_0': (facts(k_side_heavy=0, **D_FACTS), D_PLAIN),
    'D_re_defer_0': (facts(k_re_defer=0, **D_FACTS), plan(D, defer_re=False)),
    'E_timing': (facts(timing=1), C),
    'F_product_search': (facts(**F_FACTS), F),
    'F_first_step': (facts(neg_side_ready=0, **F_FACTS), plan(F, sort_early=False)),
    'G_three_queues': (facts(nstreams=3), G),
    'keep_grads': (facts(keep_grads=1), plan(A, defer_small=False)),
    'keep_grads_big_entity_table': (facts(keep_grads=1, **D_FACTS), D_PLAIN),
    'full_softmax': (facts(kind=KIND_SOFTMAX), plan(DEFAULT, side_small=True, small_order='ev_opt_fork')),
    'full_softmax_one_queue': (facts(kind=KIND_SOFTMAX, nstreams=1), DEFAULT),
    'loglinear': (facts(kind=KIND_LOGLINEAR), DEFAULT),
    'dp_host_transport': (facts(host_ar=1), DP_HOST),
    'dp_communicator': (facts(comm=1), DP_COMM),
    'dp_communicator_dp_late_0': (facts(comm=1, k_dp_late=0), DP_HOST),
    'dp_communicator_timing': (facts(comm=1, timing=1), plan(C, order=('entity', 'dh', 'word_sum', 'dense'), combine_in_tail=False, re_in_parts=False)),
    # a variants build's knobs
    'fork_late_0': (facts(k_fork_late=0), EARLY_FORK),
    'ext_events_0': (facts(k_ext_events=0), plan(EARLY_FORK, fork_carried=False, fork_recorded=True, dh_carried=False)),
    'fork_at_nce': (facts(k_fork_at=1), plan(A, fork_at='loss', dh_event='none', dh_carried=False, order=('entity', 'dh', 'dense', 'word_sum'),
                                             dense_queue='main', entity_waits_fork=True, dense_event='none', draw_next_neg=False)),
    'fork_at_nce_dw': (facts(k_fork_at=2), plan(A, fork_at='loss', dh_event='none', dh_carried=False, side_meets_fork=True,
                                                draw_next_neg=False)),
    'dw_first_0': (facts(k_dw_first=0), A_DW_MAIN),
    'dw_first_2': (facts(word_dim=1024, k_dw_first=2), A),
    'dw_first_2_sorted_chain': (facts(k_dw_first=2, **F_FACTS), plan(F, order=('dh', 'dense', 'entity', 'word_sum'), dense_queue='side',
                                                                    dense_event='ev_dense')),
    'no_early_bucket': (facts(batch=32768, k_no_early_bucket=1), A),
    'early_bucket_0': (facts(batch=32768, k_early_bucket=0), A),
    'early_bucket_1': (facts(k_early_bucket=1), plan(A, bucket_early=True)),
    'no_early_sort': (facts(k_no_early_sort=1, **F_FACTS), plan(F, sort_early=False)),
    'early_sort_1': (facts(word_dim=2048, k_early_sort=1, **D_FACTS), D),
    'no_tail': (facts(k_no_tail=1), plan(A, combine_in_tail=False, split_small=True, defer_small=False)),
    'egrad_group_sum': (facts(k_egrad_group_sum=1), plan(A, re_in_parts=False)),
    'bwd_fused': (facts(k_bwd_fused=1, bwd_fused_shape=1), plan(A_DW_MAIN, bwd_fused=True)),
    'bwd_fused_other_shape': (facts(k_bwd_fused=1, bwd_fused_shape=0), A),
    'bwd_fused_fork_late_0': (facts(k_bwd_fused=1, bwd_fused_shape=1, k_fork_late=0),
                              plan(EARLY_FORK, bwd_fused=True, order=('entity', 'dh', 'dense', 'word_sum'))),
    'dh_strip': (facts(dh_strip=1), plan(A, fork_carried=False, dh_carried=False)),
}
