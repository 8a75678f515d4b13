"""ctypes binding of include/sert_hip.h (libsert_hip.so).

There is deliberately no fallback: if the HIP library is missing or a call
fails, an exception is raised.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SERT_LIB: load another build of the library (A/B experiments with tools/build_variant.sh)
LIB_PATH = os.environ.get('SERT_LIB') or os.path.join(_HERE, 'libsert_hip.so')

KIND_LOGLINEAR, KIND_VECTORSPACE, KIND_VECTORSPACE_SOFTMAX = 0, 1, 2
SPLIT_TRAIN, SPLIT_VALIDATE = 0, 1
LL_STATUS_DEVICE, LL_STATUS_HOST = 0, 1      # sert_ll_rank_queries' per-query status
# columns of sert_reval_run's metrics
REVAL_NDCG, REVAL_MAP, REVAL_RECIP_RANK, REVAL_P5, REVAL_NUM_REL_RET, REVAL_NUM_METRICS = 0, 1, 2, 3, 4, 5

T_RW, T_RE, T_W, T_B = 0, 1, 2, 3
T_STATE0_RW, T_STATE0_RE, T_STATE0_W, T_STATE0_B = 4, 5, 6, 7
T_STATE1_RW, T_STATE1_RE, T_STATE1_W, T_STATE1_B = 8, 9, 10, 11
T_GRAD_RW, T_GRAD_RE, T_GRAD_W, T_GRAD_B = 12, 13, 14, 15
T_ACT_H, T_ACT_T, T_ACT_DA, T_ACT_DH, T_ACT_ROWLOSS = 16, 17, 18, 19, 20

COMM_ID_BYTES = 128
# SERT_LL_FORM_* of include/sert_hip_debug.h, by value
# sert_debug_state_counts, by position
STATE_COUNTS = ('run_ahead_discarded', 'run_ahead_consumed', 'lazy_flushes', 're_settled', 're_sq_handed', 're_sq_small',
                're_sq_adam')
LL_FORMS = ('none', 'wave', 'table', 'fused_row', 'stream', 'rowwise')
# SERT_EGRAD_PATH_* / SERT_EGRAD_FIXUP_*, by value
EGRAD_PATHS = ('none', 'bucket', 'sorted')
EGRAD_FIXUPS = ('none', 'wave', 'workgroup')
NCE_FORMS = ('none', 'regs', 'per_candidate', 'scalar')                  # SERT_NCE_FORM_*
WGRAD_PATHS = ('none', 'word_grad', 'dzu')                               # SERT_WGRAD_PATH_*
WGRAD_HEAVY = ('none', 'fused', 'two_launches', 'wide')                  # SERT_WGRAD_HEAVY_*
WGRAD_FORMS = ('none', 'rows32', 'rows64', 'scalar', 'rows_plus', 'rows_plus_ll', 'upper_fused', 'scalar_ll', 'bundled')   # SERT_WGRAD_FORM_*
# SERT_VS_FACT_* / SERT_VS_PLAN_* (the schedule of the vectorspace step, csrc/step_plan.h), by index; the enums the plan's
# entries take, by value
VS_FACTS = ('kind', 'host_ar', 'comm', 'timing', 'nstreams', 'n_re', 'big_re', 'big_w', 'keep_grads', 'batch', 'word_dim',
            'entity_dim', 'num_negatives', 'has_entities', 'sort_free', 'cand_early', 'neg_side_ready', 'has_labels',
            'next_neg_drawn', 'dh_strip', 'bwd_fused_shape',
            'k_ext_events', 'k_fork_late', 'k_fork_at', 'k_side_heavy', 'k_re_defer', 'k_early_bucket', 'k_no_early_bucket',
            'k_early_sort', 'k_no_early_sort', 'k_dw_first', 'k_dp_late', 'k_no_tail', 'k_egrad_group_sum', 'k_bwd_fused')
VS_KNOB_DEFAULTS = dict(k_ext_events=1, k_fork_late=1, k_fork_at=0, k_side_heavy=1, k_re_defer=1, k_early_bucket=-1,
                        k_no_early_bucket=0, k_early_sort=0, k_no_early_sort=0, k_dw_first=-1, k_dp_late=1, k_no_tail=0,
                        k_egrad_group_sum=0, k_bwd_fused=0)
VS_PLAN = ('fork_at', 'fork_carried', 'fork_recorded', 'dh_event', 'dh_carried', 'order', 'order', 'order', 'order',
           'entity_queue', 'dense_queue', 'side_meets_fork', 'entity_waits_fork', 'dense_event', 'bwd_fused', 'bucket_early',
           'sort_early', 'draw_next_neg', 'lazy_join', 'end_join', 'dp_late_join', 'combine_in_tail', 're_in_parts', 'side_small',
           'small_order', 'split_small', 'defer_re', 'defer_small', 're_on_side')
VS_FORKS = ('none', 'loss', 'dh')
VS_PIECES = ('entity', 'dh', 'dense', 'word_sum')
VS_QUEUES = ('main', 'side', 'third')
VS_EVENTS = ('none', 'ev_fork', 'ev_dense', 'ev_join3', 'ev_opt_fork')

# every symbol include/sert_hip.h declares
EXPORTS = [
    'sert_create', 'sert_destroy', 'sert_last_error', 'sert_device_info', 'sert_device_count',
    'sert_set_tensor', 'sert_get_tensor', 'sert_tensor_size', 'sert_set_step', 'sert_get_step',
    'sert_set_eval_draws', 'sert_get_eval_draws', 'sert_negatives_of_step',
    'sert_upload_dataset', 'sert_train_batch', 'sert_hint_next_batch', 'sert_train_batches',
    'sert_eval_batch', 'sert_eval_batches',
    'sert_predict_project', 'sert_predict_tokens', 'sert_ll_rank_queries', 'sert_ll_rank_candidates', 'sert_score_topk',
    'sert_reval_create', 'sert_reval_run', 'sert_reval_destroy',
    'sert_scorer_create', 'sert_scorer_destroy', 'sert_scorer_topk', 'sert_scorer_rank', 'sert_scorer_scores', 'sert_scorer_cosines',
    'sert_scorer_pairs', 'sert_scorer_rank_candidates',
    'sert_host_alloc', 'sert_host_free',
    'sert_comm_unique_id', 'sert_comm_init', 'sert_comm_init_host', 'sert_comm_destroy', 'sert_comm_stats',
    'sert_synchronize', 'sert_timing_enable', 'sert_timing_reset', 'sert_timing_count',
    'sert_timing_name', 'sert_timing_avg_us', 'sert_timing_launches', 'sert_bench_gemm', 'sert_debug_gemm', 'sert_debug_gemm_splitk', 'sert_debug_gemm_longk', 'sert_debug_gemm_route', 'sert_bench_memory', 'sert_debug_row_lists', 'sert_debug_word_index_sum',
    'sert_debug_update_counts', 'sert_debug_tail_counts', 'sert_debug_state_counts', 'sert_debug_ll_loss_form', 'sert_debug_egrad_plan', 'sert_debug_nce_form', 'sert_debug_foldin_plan', 'sert_debug_foldin_table', 'sert_debug_ll_foldin_layout', 'sert_debug_wfold_plan', 'sert_debug_wfold_index', 'sert_debug_ll_wfold_plan', 'sert_debug_wgrad_plan', 'sert_debug_vs_plan', 'sert_debug_vs_facts', 'sert_debug_vs_plan_for', 'sert_debug_poison_scratch', 'sert_debug_ll_rank_distributions', 'sert_debug_reval_chunks', 'sert_debug_scorer_counts', 'sert_debug_scorer_select', 'sert_debug_scorer_rank_counts', 'sert_debug_scorer_rank_select', 'sert_debug_scorer_rerank_counts',
    'sert_debug_count_ranks', 'sert_debug_ll_rank_candidates_distributions', 'sert_debug_ll_rerank_counts',
    'sert_profile_range_push', 'sert_profile_range_pop',
]
# ... and include/sert_hip_reval_counted.h, which sert_hip.h includes (the evaluator by rank counting)
EXPORTS_REVAL_COUNTED = ['sert_reval_create_counted', 'sert_reval_judged_ranks']
# ... and include/sert_hip_foldin.h, which sert_hip.h includes too (folding unseen entities into a trained model)
EXPORTS_FOLDIN = [
    'sert_foldin_create', 'sert_foldin_create_refresh', 'sert_foldin_destroy', 'sert_foldin_upload', 'sert_foldin_num_batches',
    'sert_foldin_train_batch', 'sert_foldin_train_batches', 'sert_foldin_eval_batch', 'sert_foldin_negatives_of_step',
    'sert_foldin_get_rows', 'sert_foldin_set_rows', 'sert_foldin_set_step', 'sert_foldin_get_step',
    'sert_foldin_set_eval_draws', 'sert_foldin_get_eval_draws',
]
FOLDIN_ROWS, FOLDIN_M, FOLDIN_V = 0, 1, 2
# ... and include/sert_hip_ll_foldin.h, which sert_hip.h includes as well (the same for a trained loglinear model)
EXPORTS_LL_FOLDIN = [
    'sert_ll_foldin_create', 'sert_ll_foldin_create_refresh', 'sert_ll_foldin_destroy', 'sert_ll_foldin_upload', 'sert_ll_foldin_upload_csr',
    'sert_ll_foldin_num_batches', 'sert_ll_foldin_train_batch', 'sert_ll_foldin_train_batches', 'sert_ll_foldin_eval_batch',
    'sert_ll_foldin_get_tensor', 'sert_ll_foldin_set_tensor',
]
LL_FOLDIN_W, LL_FOLDIN_B, LL_FOLDIN_ACCU_W, LL_FOLDIN_ACCU_B, LL_FOLDIN_DELTA_W, LL_FOLDIN_DELTA_B = 0, 1, 2, 3, 4, 5
# ... and include/sert_hip_wfold.h, which sert_hip.h includes as well (folding unseen WORDS into a trained vectorspace model)
EXPORTS_WFOLD = [
    'sert_wfold_create', 'sert_wfold_destroy', 'sert_wfold_upload', 'sert_wfold_num_batches',
    'sert_wfold_train_batch', 'sert_wfold_train_batches', 'sert_wfold_eval_batch', 'sert_wfold_negatives_of_step',
    'sert_wfold_get_rows', 'sert_wfold_set_rows', 'sert_wfold_set_step', 'sert_wfold_get_step',
    'sert_wfold_set_eval_draws', 'sert_wfold_get_eval_draws',
]
WFOLD_ROWS, WFOLD_M, WFOLD_V = 0, 1, 2
# ... and include/sert_hip_ll_wfold.h, which sert_hip.h includes as well (folding unseen WORDS into a trained loglinear model)
EXPORTS_LL_WFOLD = [
    'sert_ll_wfold_create', 'sert_ll_wfold_destroy', 'sert_ll_wfold_upload', 'sert_ll_wfold_upload_csr', 'sert_ll_wfold_num_batches',
    'sert_ll_wfold_train_batch', 'sert_ll_wfold_train_batches', 'sert_ll_wfold_eval_batch',
    'sert_ll_wfold_get_rows', 'sert_ll_wfold_set_rows',
]
LL_WFOLD_ROWS, LL_WFOLD_ACCU, LL_WFOLD_DELTA = 0, 1, 2
LL_WFOLD_FORMS = ('none', 'reg', 'stream')             # SERT_LL_WFOLD_FORM_* (include/sert_hip_debug.h)
LL_WFOLD_LABELS = ('int', 'rows')                      # SERT_LL_WFOLD_LABELS_* (include/sert_hip_debug.h)
WFOLD_PROJECT_FORMS = ('none', 'vector', 'scalar')     # SERT_WFOLD_PROJECT_* (include/sert_hip_debug.h)
FOLDIN_LOSS_FORMS = ('none', 'vector', 'scalar')       # SERT_FOLDIN_LOSS_* (include/sert_hip_debug.h)


# int (*sert_alltoall_fn)(void* user, const float* send, const int64_t* send_offsets, const int64_t* send_counts,
#                         float* recv, const int64_t* recv_offsets, const int64_t* recv_counts)
_F32P, _I64P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
ALLTOALL_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, _F32P, _I64P, _I64P, _F32P, _I64P, _I64P)


class SertConfig(ctypes.Structure):
    _fields_ = [
        ('struct_size', ctypes.c_uint32),
        ('kind', ctypes.c_int32),
        ('batch_size', ctypes.c_int32),
        ('global_batch_size', ctypes.c_int32),
        ('window_size', ctypes.c_int32),
        ('vocab_size', ctypes.c_int32),
        ('num_entities', ctypes.c_int32),
        ('word_dim', ctypes.c_int32),
        ('entity_dim', ctypes.c_int32),
        ('num_negatives', ctypes.c_int32),
        ('id_bytes', ctypes.c_int32),
        ('device', ctypes.c_int32),
        ('keep_grads', ctypes.c_int32),
        ('deterministic', ctypes.c_int32),
        ('inference_only', ctypes.c_int32),
        ('lambda_', ctypes.c_float),
        ('lr', ctypes.c_float),
        ('beta1', ctypes.c_float),
        ('beta2', ctypes.c_float),
        ('eps', ctypes.c_float),
        ('seed', ctypes.c_uint64),
    ]


class SertFoldInConfig(ctypes.Structure):
    """sert_foldin_config (include/sert_hip_foldin.h)."""
    _fields_ = [
        ('struct_size', ctypes.c_uint32),
        ('batch_size', ctypes.c_int32),
        ('num_negatives', ctypes.c_int32),
        ('lambda_', ctypes.c_float),
        ('lr', ctypes.c_float),
        ('beta1', ctypes.c_float),
        ('beta2', ctypes.c_float),
        ('eps', ctypes.c_float),
        ('seed', ctypes.c_uint64),
    ]


class SertWFoldConfig(ctypes.Structure):
    """sert_wfold_config (include/sert_hip_wfold.h)."""
    _fields_ = list(SertFoldInConfig._fields_)


class SertLlFoldInConfig(ctypes.Structure):
    """sert_ll_foldin_config (include/sert_hip_ll_foldin.h)."""
    _fields_ = [
        ('struct_size', ctypes.c_uint32),
        ('batch_size', ctypes.c_int32),
        ('lambda_', ctypes.c_float),
        ('lr', ctypes.c_float),
        ('rho', ctypes.c_float),
        ('eps', ctypes.c_float),
        ('max_cache_bytes', ctypes.c_uint64),
    ]


class SertLlWFoldConfig(ctypes.Structure):
    """sert_ll_wfold_config (include/sert_hip_ll_wfold.h)."""
    _fields_ = list(SertLlFoldInConfig._fields_)


class SertError(RuntimeError):
    pass


_lib = None


def load():
    """Load libsert_hip.so (once) and declare the signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SertError(
            'libsert_hip.so not found at %s; build it with '
            '`python -m sert_amd._build` (hipcc --offload-arch=gfx950). '
            'There is no CPU fallback.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    fp = ctypes.c_void_p  # host float*/int* passed as raw addresses
    lib.sert_create.argtypes = [ctypes.POINTER(SertConfig), ctypes.POINTER(vp)]
    lib.sert_destroy.argtypes = [vp]
    lib.sert_last_error.restype = ctypes.c_char_p
    lib.sert_device_info.argtypes = [ctypes.c_int, ctypes.c_char_p, sz]
    lib.sert_device_count.argtypes = []
    lib.sert_set_tensor.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_get_tensor.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_tensor_size.argtypes = [vp, ctypes.c_int]
    lib.sert_tensor_size.restype = sz
    lib.sert_set_step.argtypes = [vp, i64]
    lib.sert_get_step.argtypes = [vp]
    lib.sert_get_step.restype = i64
    lib.sert_set_eval_draws.argtypes = [vp, i64]
    lib.sert_get_eval_draws.argtypes = [vp]
    lib.sert_get_eval_draws.restype = i64
    lib.sert_negatives_of_step.argtypes = [vp, i64, ctypes.c_int, vp]
    lib.sert_upload_dataset.argtypes = [vp, ctypes.c_int, fp, fp, fp, fp, fp, fp, i64]
    lib.sert_train_batch.argtypes = [vp, i64, fp, ctypes.POINTER(ctypes.c_float)]
    lib.sert_train_batches.argtypes = [vp, fp, i64, fp]
    lib.sert_hint_next_batch.argtypes = [vp, i64]
    lib.sert_eval_batch.argtypes = [vp, ctypes.c_int, i64, fp, ctypes.POINTER(ctypes.c_float)]
    lib.sert_eval_batches.argtypes = [vp, ctypes.c_int, ctypes.c_void_p, i64, ctypes.c_void_p]
    lib.sert_predict_project.argtypes = [vp, fp, i64, fp]
    lib.sert_predict_tokens.argtypes = [vp, fp, i64, fp]
    lib.sert_ll_rank_queries.argtypes = [vp, fp, fp, i64, i32, fp, fp, fp, fp, fp]
    lib.sert_ll_rank_candidates.argtypes = [vp, fp, fp, i64, fp, fp, i32, fp, fp, fp, fp, fp]
    lib.sert_debug_ll_rank_candidates_distributions.argtypes = [ctypes.c_int, fp, fp, i64, i32, fp, fp, i32, fp, fp, fp, fp, fp]
    lib.sert_debug_ll_rerank_counts.argtypes = [ctypes.POINTER(i64)]
    lib.sert_reval_create.argtypes = [vp, fp, fp, i64, fp, fp, fp, fp, fp, i32, ctypes.POINTER(vp)]
    lib.sert_reval_create_counted.argtypes = lib.sert_reval_create.argtypes
    lib.sert_reval_judged_ranks.argtypes = [vp, fp]
    lib.sert_reval_run.argtypes = [vp, fp, fp, fp, fp]
    lib.sert_reval_destroy.argtypes = [vp]
    lib.sert_foldin_create.argtypes = [vp, i32, fp, ctypes.POINTER(SertFoldInConfig), ctypes.POINTER(vp)]
    lib.sert_foldin_create_refresh.argtypes = [vp, fp, i32, i32, fp, ctypes.POINTER(SertFoldInConfig), ctypes.POINTER(vp)]
    lib.sert_foldin_destroy.argtypes = [vp]
    lib.sert_foldin_upload.argtypes = [vp, fp, fp, fp, i64]
    lib.sert_foldin_num_batches.argtypes = [vp]
    lib.sert_foldin_num_batches.restype = i64
    lib.sert_foldin_train_batch.argtypes = [vp, i64, fp, ctypes.POINTER(ctypes.c_float)]
    lib.sert_foldin_train_batches.argtypes = [vp, fp, i64, fp]
    lib.sert_foldin_eval_batch.argtypes = [vp, i64, fp, ctypes.POINTER(ctypes.c_float)]
    lib.sert_foldin_negatives_of_step.argtypes = [vp, i64, ctypes.c_int, fp]
    lib.sert_foldin_get_rows.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_foldin_set_rows.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_foldin_set_step.argtypes = [vp, i64]
    lib.sert_foldin_get_step.argtypes = [vp]
    lib.sert_foldin_get_step.restype = i64
    lib.sert_foldin_set_eval_draws.argtypes = [vp, i64]
    lib.sert_foldin_get_eval_draws.argtypes = [vp]
    lib.sert_foldin_get_eval_draws.restype = i64
    lib.sert_ll_foldin_create.argtypes = [vp, i32, fp, fp, ctypes.POINTER(SertLlFoldInConfig), ctypes.POINTER(vp)]
    lib.sert_ll_foldin_create_refresh.argtypes = [vp, fp, i32, i32, fp, fp, ctypes.POINTER(SertLlFoldInConfig), ctypes.POINTER(vp)]
    lib.sert_ll_foldin_destroy.argtypes = [vp]
    lib.sert_ll_foldin_upload.argtypes = [vp, fp, fp, fp, i64]
    lib.sert_ll_foldin_upload_csr.argtypes = [vp, fp, fp, fp, fp, fp, i64]
    lib.sert_ll_foldin_num_batches.argtypes = [vp]
    lib.sert_ll_foldin_num_batches.restype = i64
    lib.sert_ll_foldin_train_batch.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_float)]
    lib.sert_ll_foldin_train_batches.argtypes = [vp, fp, i64, fp]
    lib.sert_ll_foldin_eval_batch.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_float)]
    lib.sert_ll_foldin_get_tensor.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_ll_foldin_set_tensor.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_wfold_create.argtypes = [vp, i32, fp, ctypes.POINTER(SertWFoldConfig), ctypes.POINTER(vp)]
    lib.sert_wfold_destroy.argtypes = [vp]
    lib.sert_wfold_upload.argtypes = [vp, fp, fp, fp, i64]
    lib.sert_wfold_num_batches.argtypes = [vp]
    lib.sert_wfold_num_batches.restype = i64
    lib.sert_wfold_train_batch.argtypes = [vp, i64, fp, ctypes.POINTER(ctypes.c_float)]
    lib.sert_wfold_train_batches.argtypes = [vp, fp, i64, fp]
    lib.sert_wfold_eval_batch.argtypes = [vp, i64, fp, ctypes.POINTER(ctypes.c_float)]
    lib.sert_wfold_negatives_of_step.argtypes = [vp, i64, ctypes.c_int, fp]
    lib.sert_wfold_get_rows.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_wfold_set_rows.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_wfold_set_step.argtypes = [vp, i64]
    lib.sert_wfold_get_step.argtypes = [vp]
    lib.sert_wfold_get_step.restype = i64
    lib.sert_wfold_set_eval_draws.argtypes = [vp, i64]
    lib.sert_wfold_get_eval_draws.argtypes = [vp]
    lib.sert_wfold_get_eval_draws.restype = i64
    lib.sert_ll_wfold_create.argtypes = [vp, i32, fp, ctypes.POINTER(SertLlWFoldConfig), ctypes.POINTER(vp)]
    lib.sert_ll_wfold_destroy.argtypes = [vp]
    lib.sert_ll_wfold_upload.argtypes = [vp, fp, fp, fp, i64]
    lib.sert_ll_wfold_upload_csr.argtypes = [vp, fp, fp, fp, fp, fp, i64]
    lib.sert_ll_wfold_num_batches.argtypes = [vp]
    lib.sert_ll_wfold_num_batches.restype = i64
    lib.sert_ll_wfold_train_batch.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_float)]
    lib.sert_ll_wfold_train_batches.argtypes = [vp, fp, i64, fp]
    lib.sert_ll_wfold_eval_batch.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_float)]
    lib.sert_ll_wfold_get_rows.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_ll_wfold_set_rows.argtypes = [vp, ctypes.c_int, fp, sz]
    lib.sert_debug_ll_wfold_plan.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    lib.sert_debug_wfold_plan.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    lib.sert_debug_wfold_index.argtypes = [fp, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, i64, fp, fp, i64, fp, i64,
                                           ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.sert_score_topk.argtypes = [ctypes.c_int, fp, i64, i32, fp, i64, i32, fp, fp]
    lib.sert_scorer_create.argtypes = [ctypes.c_int, fp, i64, i32, ctypes.POINTER(vp)]
    lib.sert_scorer_destroy.argtypes = [vp]
    lib.sert_scorer_topk.argtypes = [vp, fp, i64, i32, fp, fp]
    lib.sert_scorer_rank.argtypes = [vp, fp, i64, i32, fp, fp]
    lib.sert_scorer_scores.argtypes = [vp, fp, i64, fp]
    lib.sert_scorer_cosines.argtypes = [vp, fp, i64, fp]
    lib.sert_scorer_pairs.argtypes = [vp, fp, i64, fp, fp, ctypes.c_int, fp]
    lib.sert_scorer_rank_candidates.argtypes = [vp, fp, i64, fp, fp, i32, fp, fp]
    lib.sert_host_alloc.argtypes = [ctypes.POINTER(vp), sz]
    lib.sert_host_free.argtypes = [vp]
    lib.sert_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.sert_comm_init.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.sert_comm_destroy.argtypes = [vp]
    lib.sert_comm_init_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, ALLTOALL_FN, vp]
    lib.sert_comm_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.sert_debug_row_lists.argtypes = [fp, ctypes.c_int, ctypes.c_int, i64, i64, i64, i64, i64] + [fp] * 7 + [i64, fp]
    lib.sert_synchronize.argtypes = [vp]
    lib.sert_profile_range_push.argtypes = [ctypes.c_char_p]
    lib.sert_profile_range_pop.argtypes = []
    lib.sert_timing_enable.argtypes = [vp, ctypes.c_int]
    lib.sert_timing_reset.argtypes = [vp]
    lib.sert_timing_count.argtypes = [vp]
    lib.sert_timing_name.argtypes = [vp, ctypes.c_int]
    lib.sert_timing_name.restype = ctypes.c_char_p
    lib.sert_timing_avg_us.argtypes = [vp, ctypes.c_int]
    lib.sert_timing_avg_us.restype = ctypes.c_double
    lib.sert_timing_launches.argtypes = [vp, ctypes.c_int]
    lib.sert_timing_launches.restype = ctypes.c_double
    lib.sert_bench_gemm.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_double)]
    lib.sert_bench_memory.argtypes = [ctypes.c_int, ctypes.c_int, sz, sz, ctypes.c_int, ctypes.c_int, sz, ctypes.c_int,
                                      ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise SertError(load().sert_last_error().decode('utf-8', 'replace'))


def _addr(a):
    return None if a is None else a.ctypes.data


def device_count():
    return load().sert_device_count()


def device_info(device=0):
    buf = ctypes.create_string_buffer(512)
    n = load().sert_device_info(device, buf, 512)
    if n < 0:
        raise SertError(load().sert_last_error().decode())
    return buf.value.decode()


def require_gpu():
    """Raise unless a HIP device is visible (the product has no CPU path)."""
    n = device_count()
    if n is None or n <= 0:
        raise SertError('no HIP device visible: sert_amd runs on MI355X (gfx950) only; '
                        'there is no CPU fallback.')
    return n


class Engine(object):
    """Thin owner of one sert_model handle."""

    def __init__(self, **cfg):
        lib = load()
        c = SertConfig()
        c.struct_size = ctypes.sizeof(SertConfig)
        for k, v in cfg.items():
            if not hasattr(c, k):
                raise TypeError('unknown sert_config field %r' % k)
            setattr(c, k, v)
        self.cfg = c
        self._h = ctypes.c_void_p()
        self._lib = lib
        check(lib.sert_create(ctypes.byref(c), ctypes.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.sert_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # tensors
    def tensor_size(self, which):
        return int(self._lib.sert_tensor_size(self._h, which))

    def set_tensor(self, which, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        check(self._lib.sert_set_tensor(self._h, which, a.ctypes.data, a.size))

    def get_tensor(self, which, shape=None, out=None):
        n = self.tensor_size(which)
        if out is None:
            out = np.empty(n, dtype=np.float32)
        assert out.dtype == np.float32 and out.size == n and out.flags['C_CONTIGUOUS']
        check(self._lib.sert_get_tensor(self._h, which, out.ctypes.data, n))
        return out.reshape(shape) if shape is not None else out

    def set_step(self, t):
        check(self._lib.sert_set_step(self._h, int(t)))

    def get_step(self):
        return int(self._lib.sert_get_step(self._h))

    def set_eval_draws(self, n):
        check(self._lib.sert_set_eval_draws(self._h, int(n)))

    def get_eval_draws(self):
        return int(self._lib.sert_get_eval_draws(self._h))

    def negatives_of_step(self, position, evaluation=False):
        """(B, z) int64: the negatives the device sampler draws at training position `position` (= get_step() before the
        step) or for the `position`-th evaluated batch."""
        out = np.empty((self.cfg.batch_size, self.cfg.num_negatives), dtype=np.int64)
        check(self._lib.sert_negatives_of_step(self._h, int(position), int(bool(evaluation)), out.ctypes.data))
        return out

    # data
    def upload_dataset(self, split, x, y_int=None, csr=None, w=None):
        x = np.ascontiguousarray(x)
        n = x.shape[0]
        keep = [x]
        y_addr = ip = ix = da = None
        if y_int is not None:
            y_int = np.ascontiguousarray(y_int, dtype=np.int32)
            keep.append(y_int)
            y_addr = y_int.ctypes.data
        if csr is not None:
            # the C ABI takes canonical CSR only (strictly increasing columns per row, include/sert_hip.h): rows that scipy
            # knows to be unsorted are sorted here; duplicate columns are the caller's to sum (sum_duplicates)
            if not getattr(csr, 'has_sorted_indices', True):
                csr = csr.sorted_indices()
            indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
            data = np.ascontiguousarray(csr.data, dtype=np.float32)
            keep += [indptr, indices, data]
            ip, ix, da = indptr.ctypes.data, indices.ctypes.data, data.ctypes.data
        w_addr = None
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            keep.append(w)
            w_addr = w.ctypes.data
        check(self._lib.sert_upload_dataset(self._h, split, x.ctypes.data if n else None,
                                            y_addr, ip, ix, da, w_addr, n))
        del keep

    # hot path
    def train_batch(self, batch_index, negatives=None):
        loss = ctypes.c_float()
        if negatives is not None:
            negatives = np.ascontiguousarray(negatives, dtype=np.int64)
        check(self._lib.sert_train_batch(self._h, int(batch_index), _addr(negatives),
                                         ctypes.byref(loss)))
        return np.float32(loss.value)

    def hint_next_batch(self, next_batch_index):
        """The batch that will be trained after the next train_batch call (or None):
        its parameter-only forward part is enqueued before that call waits for its loss."""
        check(self._lib.sert_hint_next_batch(
            self._h, -1 if next_batch_index is None else int(next_batch_index)))

    def train_batches(self, batch_indices):
        idx = np.ascontiguousarray(batch_indices, dtype=np.int64)
        out = np.empty(idx.size, dtype=np.float32)
        check(self._lib.sert_train_batches(self._h, idx.ctypes.data, idx.size, out.ctypes.data))
        return out

    def eval_batch(self, split, batch_index, negatives=None):
        loss = ctypes.c_float()
        if negatives is not None:
            negatives = np.ascontiguousarray(negatives, dtype=np.int64)
        check(self._lib.sert_eval_batch(self._h, split, int(batch_index), _addr(negatives),
                                        ctypes.byref(loss)))
        return np.float32(loss.value)

    def eval_batches(self, split, batch_indices):
        """Unweighted batch-mean losses of several batches, one host synchronisation."""
        idx = np.ascontiguousarray(batch_indices, dtype=np.int64)
        out = np.empty(idx.shape[0], dtype=np.float32)
        if idx.shape[0]:
            check(self._lib.sert_eval_batches(self._h, split, idx.ctypes.data, idx.shape[0], out.ctypes.data))
        return out

    def predict_project(self, avg):
        avg = np.ascontiguousarray(avg, dtype=np.float32)
        q = avg.shape[0]
        out = np.empty((q, self.cfg.entity_dim), dtype=np.float32)
        check(self._lib.sert_predict_project(self._h, avg.ctypes.data, q, out.ctypes.data))
        return out

    def predict_tokens(self, ids):
        ids = np.ascontiguousarray(ids)
        assert ids.dtype.itemsize == self.cfg.id_bytes
        rows = ids.shape[0]
        out = np.empty((rows, self.cfg.window_size, self.cfg.num_entities), dtype=np.float32)
        check(self._lib.sert_predict_tokens(self._h, ids.ctypes.data, rows, out.ctypes.data))
        return out

    def ll_rank_queries(self, token_lists, k=None):
        """sert_ll_rank_queries: (idx (Q, kk) int32, score (Q, kk) f32, joint_entropy (Q,), token_entropy (T,),
        status (Q,) int32, offsets (Q + 1,) int64); kk = V_e for k None or k >= V_e."""
        tokens, offsets = _concat_queries(token_lists)
        return _ll_rank_call(self.cfg.num_entities, offsets, k, lambda kk, outs: self._lib.sert_ll_rank_queries(
            self._h, tokens.ctypes.data, offsets.ctypes.data, offsets.size - 1, kk, *outs), tokens.size)

    def ll_rank_candidates(self, token_lists, candidates, k=None):
        """sert_ll_rank_candidates: every query's candidate list (one integer array per query; any order, duplicates allowed:
        sorted and de-duplicated here, as Scorer.rank_candidates does) ranked under the loglinear model, scores normalised
        over all entities.  (out_indptr (Q + 1,) int64, idx int32, score f32 -- query q's result is
        idx / score[out_indptr[q]:out_indptr[q + 1]], its best min(k, length), k None: the whole list --, joint_entropy (Q,),
        token_entropy (T,), status (Q,) int32, offsets (Q + 1,) int64)."""
        tokens, offsets = _concat_queries(token_lists)
        return _ll_rank_candidates_call(self.cfg.num_entities, offsets, candidates, k, tokens.size,
                                        lambda indptr, ents, kk, outs: self._lib.sert_ll_rank_candidates(
                                            self._h, tokens.ctypes.data, offsets.ctypes.data, offsets.size - 1,
                                            indptr.ctypes.data, ents.ctypes.data, kk, *outs))

    # data parallel
    def comm_init(self, unique_id, rank, world):
        assert len(unique_id) == COMM_ID_BYTES
        check(self._lib.sert_comm_init(self._h, unique_id, rank, world))

    def comm_init_host(self, rank, world, alltoall):
        """Host-mediated exchange (verification transport, sert_comm_init_host):
        ``alltoall(send, send_offsets, send_counts, recv, recv_offsets, recv_counts)`` moves float32
        segments between the ranks (numpy views of the engine's pinned buffers; offsets and counts are
        int64 arrays of length world, in floats) -- see sert_amd.distributed.host_alltoall."""
        def trampoline(_user, send, soff, scnt, recv, roff, rcnt):
            try:
                so = np.ctypeslib.as_array(soff, shape=(world,))
                sc = np.ctypeslib.as_array(scnt, shape=(world,))
                ro = np.ctypeslib.as_array(roff, shape=(world,))
                rc = np.ctypeslib.as_array(rcnt, shape=(world,))
                ns = int((so + sc).max()) if world else 0
                nr = int((ro + rc).max()) if world else 0
                sbuf = np.ctypeslib.as_array(send, shape=(max(ns, 1),))
                rbuf = np.ctypeslib.as_array(recv, shape=(max(nr, 1),))
                alltoall(sbuf, so, sc, rbuf, ro, rc)
                return 0
            except Exception:  # noqa: BLE001 - reported through the C error path
                import traceback
                traceback.print_exc()
                return 1
        self._host_alltoall = ALLTOALL_FN(trampoline)   # keep the thunk alive
        check(self._lib.sert_comm_init_host(self._h, rank, world, self._host_alltoall, None))

    def comm_stats(self):
        """sert_comm_stats as a dict (world 1 / no communicator: exchange 'none')."""
        v = (ctypes.c_double * 8)()
        check(self._lib.sert_comm_stats(self._h, v, 8))
        return {'world': int(v[0]), 'exchange': {0: 'none', 1: 'zero1', 2: 'rows'}[int(v[1])],
                'bytes_per_step': float(v[2]), 'zero1_bytes_per_step': float(v[3]),
                'transport': {0: 'none', 1: 'rccl', 2: 'host'}[int(v[4])], 'steps': int(v[5]),
                'rows_fetched_per_batch': float(v[6]), 'rows_served_per_batch': float(v[7])}

    # diagnostics
    def synchronize(self):
        check(self._lib.sert_synchronize(self._h))

    def timing_enable(self, on=True):
        """False / 0: off; True / 1: every kernel group alone on one queue; 2: in the step (see sert_hip.h)."""
        check(self._lib.sert_timing_enable(self._h, int(on)))

    def timing_launches(self):
        """In-step mode: timed launches per training step and group."""
        n = self._lib.sert_timing_count(self._h)
        return {self._lib.sert_timing_name(self._h, i).decode():
                self._lib.sert_timing_launches(self._h, i) for i in range(n)}

    def timing_reset(self):
        check(self._lib.sert_timing_reset(self._h))

    def poison_scratch(self):
        """sert_debug_poison_scratch (test hook): NaNs into the gradient scratch, wrong run bounds behind it."""
        self._lib.sert_debug_poison_scratch.argtypes = [ctypes.c_void_p]
        check(self._lib.sert_debug_poison_scratch(self._h))

    def update_counts(self):
        """sert_debug_update_counts (test hook): launches of the word-table update by kernel form since creation."""
        v = (ctypes.c_int64 * 10)()
        self._lib.sert_debug_update_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
        check(self._lib.sert_debug_update_counts(self._h, v, 10))
        names = ('dense', 'lazy', 'skip_32_1', 'skip_64_1', 'skip_32_3', 'skip_64_2', 'skip_64_3', 'skip_64_4', 'skip_full', 'skip_sparse')
        return dict(zip(names, (int(x) for x in v)))

    def tail_counts(self):
        """sert_debug_tail_counts (test hook): the vectorspace step's tail launches since creation, alone and inside a gather."""
        v = (ctypes.c_int64 * 2)()
        self._lib.sert_debug_tail_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
        check(self._lib.sert_debug_tail_counts(self._h, v, 2))
        return {'alone': int(v[0]), 'in_gather': int(v[1])}

    def state_counts(self):
        """sert_debug_state_counts (test hook): transitions of the state a step leaves for the next call, since creation."""
        v = (ctypes.c_int64 * len(STATE_COUNTS))()
        self._lib.sert_debug_state_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
        check(self._lib.sert_debug_state_counts(self._h, v, len(STATE_COUNTS)))
        return dict(zip(STATE_COUNTS, (int(x) for x in v)))

    def ll_loss_form(self):
        """sert_debug_ll_loss_form (test hook): the loss form the last loglinear forward launched."""
        v = (ctypes.c_int32 * 5)()
        self._lib.sert_debug_ll_loss_form.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_ll_loss_form(self._h, v, 5))
        return {'form': LL_FORMS[int(v[0])], 'param': int(v[1]), 'train': bool(v[2]), 'slots': bool(v[3]), 'segments': int(v[4])}

    def egrad_plan(self):
        """sert_debug_egrad_plan (test hook): what the last vectorspace backward launched for the entity-table gradient.
        {'path': 'none'} before the first backward; the keys of the path taken otherwise."""
        v = (ctypes.c_int32 * 12)()
        self._lib.sert_debug_egrad_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_egrad_plan(self._h, v, 12))
        v = [int(x) for x in v]
        path = EGRAD_PATHS[v[0]]
        if path == 'bucket':
            return {'path': path, 'sub_rows': v[1], 'num_sub': v[2], 'subs_per_group': v[3], 'groups': v[4], 'ranges': v[5],
                    'group_sum': bool(v[6])}
        if path == 'sorted':
            return {'path': path, 'sort_bits': v[7], 'passes': v[8], 'vec': v[9], 'nch': v[10], 'fixup': EGRAD_FIXUPS[v[11]]}
        assert not any(v), v
        return {'path': path}

    def nce_form(self):
        """sert_debug_nce_form (test hook): the NCE loss kernel the last vectorspace forward launched -- 'form' (none / regs /
        per_candidate / scalar), 'param' (NCH or NPL), 'maxc' (regs only, else 0: 6 for z + 1 <= 6, 11 for z + 1 == 11, else 12), 'train', 'workgroups' and 'loss_partials'.
        All zero before the first forward and for a model without an NCE loss."""
        v = (ctypes.c_int32 * 6)()
        self._lib.sert_debug_nce_form.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_nce_form(self._h, v, 6))
        v = [int(x) for x in v]
        return {'form': NCE_FORMS[v[0]], 'param': v[1], 'maxc': v[2], 'train': bool(v[3]), 'workgroups': v[4],
                'loss_partials': v[5]}

    def wgrad_plan(self):
        """sert_debug_wgrad_plan (test hook): what the last backward launched for the per-word sums (the word-table gradient of a
        vectorspace model, dZu of a loglinear one).  {'path': 'none'} before the first backward; otherwise 'levels' of the
        batch's tree, 'launches' [(form, gridDim.y)] of the tree in order, 'dense_cnt', 'heavy' (none / fused / two_launches /
        wide) with 'heavy_rows' per workgroup and 'heavy_blocks', 'combine_alone', 'slot_is_row'."""
        v = (ctypes.c_int32 * 24)()
        self._lib.sert_debug_wgrad_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_wgrad_plan(self._h, v, 24))
        v = [int(x) for x in v]
        path = WGRAD_PATHS[v[0]]
        if path == 'none':
            assert not any(v), v
            return {'path': path}
        assert v[2] <= 6, v
        return {'path': path, 'levels': v[1], 'launches': [(WGRAD_FORMS[v[10 + 2 * k]], v[11 + 2 * k]) for k in range(v[2])],
                'dense_cnt': v[3], 'heavy': WGRAD_HEAVY[v[4]], 'heavy_rows': v[5], 'heavy_blocks': v[6],
                'combine_alone': bool(v[7]), 'slot_is_row': bool(v[8])}

    def vs_plan(self):
        """sert_debug_vs_plan (test hook): the schedule of the step this model issued last, as vs_plan_for returns it."""
        v = (ctypes.c_int32 * len(VS_PLAN))()
        self._lib.sert_debug_vs_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_vs_plan(self._h, v, len(VS_PLAN)))
        return _vs_plan_dict(v)

    def vs_facts(self):
        """sert_debug_vs_facts (test hook): the facts the last step's schedule was decided from, by name (VS_FACTS)."""
        v = (ctypes.c_int32 * len(VS_FACTS))()
        self._lib.sert_debug_vs_facts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_vs_facts(self._h, v, len(VS_FACTS)))
        return dict(zip(VS_FACTS, (int(x) for x in v)))

    def timings(self):
        n = self._lib.sert_timing_count(self._h)
        return {self._lib.sert_timing_name(self._h, i).decode():
                self._lib.sert_timing_avg_us(self._h, i) for i in range(n)}


def _vs_plan_dict(v):
    v = [int(x) for x in v]
    p = {name: bool(v[i]) for i, name in enumerate(VS_PLAN) if name != 'order'}
    p['fork_at'] = VS_FORKS[v[VS_PLAN.index('fork_at')]]
    p['order'] = tuple(VS_PIECES[x] for x in v[VS_PLAN.index('order'):][:4])
    for name in ('entity_queue', 'dense_queue'):
        p[name] = VS_QUEUES[v[VS_PLAN.index(name)]]
    for name in ('dh_event', 'dense_event', 'small_order'):
        p[name] = VS_EVENTS[v[VS_PLAN.index(name)]]
    return p


def vs_plan_for(**facts):
    """sert_debug_vs_plan_for (test hook, no device): the schedule csrc/step_plan.h decides for the given facts (VS_FACTS by
    name; a fact not given is 0 -- nstreams 2 -- and a knob not given unset), as a dict: flags as bool, 'fork_at', the queues
    and the events by name, 'order' as a tuple of piece names."""
    vals = dict({name: 0 for name in VS_FACTS}, nstreams=2, **VS_KNOB_DEFAULTS)
    unknown = set(facts) - set(vals)
    assert not unknown, unknown
    vals.update(facts)
    f = (ctypes.c_int32 * len(VS_FACTS))(*[int(vals[name]) for name in VS_FACTS])
    v = (ctypes.c_int32 * len(VS_PLAN))()
    lib = load()
    lib.sert_debug_vs_plan_for.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    check(lib.sert_debug_vs_plan_for(f, len(VS_FACTS), v, len(VS_PLAN)))
    return _vs_plan_dict(v)


def comm_unique_id():
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    check(load().sert_comm_unique_id(buf))
    return buf.raw


def _concat_queries(token_lists):
    lengths = np.fromiter((len(t) for t in token_lists), dtype=np.int64, count=len(token_lists))
    offsets = np.zeros(len(token_lists) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    tokens = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int64) for t in token_lists])
                                  if len(token_lists) else np.zeros(0, np.int64), dtype=np.int32)
    return tokens, offsets


def _ll_rank_call(num_entities, offsets, k, call, num_tokens):
    q = offsets.size - 1
    kk = num_entities if k is None or k >= num_entities else int(k)
    idx = np.empty((q, kk), dtype=np.int32)
    score = np.empty((q, kk), dtype=np.float32)
    joint_h = np.empty(q, dtype=np.float32)
    token_h = np.empty(num_tokens, dtype=np.float32)
    status = np.empty(q, dtype=np.int32)
    outs = [a.ctypes.data for a in (idx, score, joint_h, token_h, status)]
    check(call(-1 if k is None else int(k), outs))
    return idx, score, joint_h, token_h, status, offsets


def debug_ll_rank_distributions(distributions, offsets, k=None, device=0):
    """sert_debug_ll_rank_distributions: the ranking kernels of sert_ll_rank_queries on per-token distributions
    (offsets[-1], V_e) given here; same outputs as Engine.ll_rank_queries."""
    lib = load()
    P = np.ascontiguousarray(distributions, dtype=np.float32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    assert P.ndim == 2 and P.shape[0] == offsets[-1]
    lib.sert_debug_ll_rank_distributions.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                     ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 5
    return _ll_rank_call(P.shape[1], offsets, k, lambda kk, outs: lib.sert_debug_ll_rank_distributions(
        device, P.ctypes.data, offsets.ctypes.data, offsets.size - 1, P.shape[1], kk, *outs), P.shape[0])


def _ll_rank_candidates_call(num_entities, offsets, candidates, k, num_tokens, call):
    q = offsets.size - 1
    if k is not None and k <= 0:
        raise SertError('ll_rank_candidates: k must be None (the whole list) or positive')
    if len(candidates) != q:
        raise SertError('ll_rank_candidates: %d candidate lists for %d queries' % (len(candidates), q))
    indptr, ents = candidates_csr(candidates, unique=True)
    out_indptr = ranked_indptr(indptr, k)
    n = int(out_indptr[-1])
    idx = np.empty(max(n, 1), dtype=np.int32)
    score = np.empty(max(n, 1), dtype=np.float32)
    joint_h = np.empty(q, dtype=np.float32)
    token_h = np.empty(max(num_tokens, 1), dtype=np.float32)
    status = np.empty(q, dtype=np.int32)
    # (the library refuses a null pointer: an empty array still has an address to give)
    e = ents if len(ents) else np.zeros(1, np.int32)
    outs = [a.ctypes.data for a in (idx, score, joint_h, token_h, status)]
    check(call(indptr, e, -1 if k is None else min(int(k), 2 ** 31 - 1), outs))
    return out_indptr, idx[:n], score[:n], joint_h, token_h[:num_tokens], status, offsets


def debug_ll_rank_candidates_distributions(distributions, offsets, candidates, k=None, device=0):
    """sert_debug_ll_rank_candidates_distributions: the aggregate and the candidate-ranking kernels of
    sert_ll_rank_candidates on per-token distributions (offsets[-1], V_e) given here; same outputs as
    Engine.ll_rank_candidates."""
    lib = load()
    P = np.ascontiguousarray(distributions, dtype=np.float32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    assert P.ndim == 2 and P.shape[0] == offsets[-1]
    return _ll_rank_candidates_call(P.shape[1], offsets, candidates, k, P.shape[0],
                                    lambda indptr, ents, kk, outs: lib.sert_debug_ll_rank_candidates_distributions(
                                        device, P.ctypes.data, offsets.ctypes.data, offsets.size - 1, P.shape[1],
                                        indptr.ctypes.data, ents.ctypes.data, kk, *outs))


def debug_ll_rerank_counts():
    """sert_debug_ll_rerank_counts (test hook): what the loglinear candidate calls of this process did so far -- [calls, their
    chunks, lists ranked by the LDS kernel, by the slab and the counting-sort passes, empty lists]."""
    v = (ctypes.c_int64 * 5)()
    check(load().sert_debug_ll_rerank_counts(v))
    return [int(x) for x in v]


def score_topk(entities, projections, k, device=0):
    """Batched VectorSpaceCallback scoring (bin/query.py:239-370)."""
    e = np.ascontiguousarray(entities, dtype=np.float32)
    p = np.ascontiguousarray(projections, dtype=np.float32)
    assert e.ndim == 2 and p.ndim == 2 and e.shape[1] == p.shape[1]
    q = p.shape[0]
    idx = np.empty((q, k), dtype=np.int32)
    val = np.empty((q, k), dtype=np.float32)
    check(load().sert_score_topk(device, e.ctypes.data, e.shape[0], e.shape[1], p.ctypes.data, q,
                                 k, idx.ctypes.data, val.ctypes.data))
    return idx, val


class PinnedBuffer(object):
    """Page-locked host memory (sert_host_alloc) viewed as a numpy array; grows on demand."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        self._ptr = ctypes.c_void_p()
        self._bytes = 0
        self._lib = load()

    def view(self, shape):
        if os.environ.get('SERT_NO_PINNED'):     # cross-check knob: ordinary pageable arrays
            return np.empty(shape, dtype=self.dtype)
        need = int(np.prod(shape)) * self.dtype.itemsize
        if need > self._bytes:
            self.free()
            cap = max(need, 1 << 16)
            check(self._lib.sert_host_alloc(ctypes.byref(self._ptr), cap))
            self._bytes = cap
        raw = (ctypes.c_char * max(need, 1)).from_address(self._ptr.value)
        return np.frombuffer(raw, dtype=self.dtype, count=int(np.prod(shape))).reshape(shape)

    def holds(self, array):
        """Is `array` a view of this buffer (so that no staging copy is needed)?"""
        if not self._ptr.value or not isinstance(array, np.ndarray) or not array.flags['C_CONTIGUOUS']:
            return False
        addr = array.ctypes.data
        return self._ptr.value <= addr and addr + array.nbytes <= self._ptr.value + self._bytes

    def free(self):
        if self._ptr.value:
            self._lib.sert_host_free(self._ptr)
            self._ptr = ctypes.c_void_p()
            self._bytes = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def debug_scorer_select(cosines, k, mode, thr=-np.inf, device=0):
    """sert_debug_scorer_select (test hook): the scorer's selection kernels on caller-provided cosines (Q, V); mode 0
    topk_rows, mode 1 topk_from_groups on the lists of the elements >= thr.  (idx, score)."""
    s = np.ascontiguousarray(cosines, dtype=np.float32)
    assert s.ndim == 2
    idx = np.empty((s.shape[0], k), dtype=np.int32)
    val = np.empty((s.shape[0], k), dtype=np.float32)
    lib = load()
    lib.sert_debug_scorer_select.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                             ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    check(lib.sert_debug_scorer_select(device, mode, s.ctypes.data, s.shape[0], s.shape[1], k, float(thr), idx.ctypes.data,
                                       val.ctypes.data))
    return idx, val


def debug_scorer_rank_select(cosines, k=None, device=0):
    """sert_debug_scorer_rank_select (test hook): the ranking kernels of sert_scorer_rank on caller-provided cosines (Q, V) --
    the LDS sort for V <= 8192, the counting-sort passes above.  (idx, score), (Q, kk)."""
    s = np.ascontiguousarray(cosines, dtype=np.float32)
    assert s.ndim == 2
    keep = s.shape[1] if k is None else min(int(k), s.shape[1])
    idx = np.empty((s.shape[0], keep), dtype=np.int32)
    val = np.empty((s.shape[0], keep), dtype=np.float32)
    lib = load()
    lib.sert_debug_scorer_rank_select.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.c_void_p, ctypes.c_void_p]
    check(lib.sert_debug_scorer_rank_select(device, s.ctypes.data, s.shape[0], s.shape[1], -1 if k is None else int(k),
                                            idx.ctypes.data, val.ctypes.data))
    return idx, val


def debug_count_ranks(cosines, judged, device=0):
    """sert_debug_count_ranks (test hook): the counting kernel of the counted evaluator on caller-provided cosines (Q, V);
    judged: per row the judged entity indices.  -> per row an int32 array: the 1-based rank of each judged entity under the
    scorer's order."""
    s = np.ascontiguousarray(cosines, dtype=np.float32)
    assert s.ndim == 2 and len(judged) == s.shape[0]
    indptr = np.zeros(s.shape[0] + 1, dtype=np.int64)
    np.cumsum([len(e) for e in judged], out=indptr[1:])
    ents = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.int64) for e in judged]), dtype=np.int32)
    ranks = np.zeros(len(ents), dtype=np.int32)
    lib = load()
    lib.sert_debug_count_ranks.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
    check(lib.sert_debug_count_ranks(device, s.ctypes.data, s.shape[0], s.shape[1], indptr.ctypes.data, ents.ctypes.data,
                                     ranks.ctypes.data))
    return [ranks[indptr[q]:indptr[q + 1]] for q in range(s.shape[0])]


def candidates_csr(candidates, unique=False):
    """Per-query candidate lists (a sequence of integer arrays) as the CSR sert_scorer_pairs / sert_scorer_rank_candidates
    take: (indptr (Q + 1) int64, entities int32).  unique: every list sorted ascending and de-duplicated (np.unique), what
    the ranker requires; otherwise order and duplicates are kept."""
    lists = [np.asarray(c).reshape(-1) for c in candidates]
    for c in lists:
        if c.size and not np.issubdtype(c.dtype, np.integer):
            raise SertError('candidate lists hold integer entity indices')
    def flatten(lists):
        indptr = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum([c.size for c in lists], out=indptr[1:])
        return indptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))

    indptr, flat = flatten(lists)
    if unique and flat.size > 1:
        # (lists that arrive clean -- a run file's, a previous call's -- are recognised in one pass over the flat array)
        rising = flat[1:] > flat[:-1]
        rising[indptr[1:-1][(indptr[1:-1] > 0) & (indptr[1:-1] < flat.size)] - 1] = True      # (across a list boundary: anything goes)
        if not rising.all():
            indptr, flat = flatten([np.unique(c) for c in lists])
    if flat.size and (flat.min() < -2 ** 31 or flat.max() >= 2 ** 31):
        raise SertError('candidate entity index does not fit int32')
    return indptr, np.ascontiguousarray(flat, dtype=np.int32)


def ranked_indptr(indptr, k=None):
    """Where sert_scorer_rank_candidates writes each query's results: the prefix sum of min(k, length) (k None: length)."""
    lengths = np.diff(np.asarray(indptr, dtype=np.int64))
    out = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths if k is None else np.minimum(lengths, int(k)), out=out[1:])
    return out


class Scorer(object):
    """Persistent device copy of the (L2-normalised) entity table + top-k scoring
    (sert_scorer_* in include/sert_hip.h).

    Host arrays cross the boundary through page-locked buffers the scorer owns: fill
    ``query_buffer(Q)`` in place (or pass any array: it is copied there) and read the result
    views, which stay valid until the next call on this scorer."""

    #: upper bound on Q_chunk * V_e floats materialised on the host when no device top-k applies
    MAX_HOST_SCORES = 1 << 26

    def __init__(self, entities, device=0):
        e = np.ascontiguousarray(entities, dtype=np.float32)
        assert e.ndim == 2
        self.num_entities, self.dim = e.shape
        self._lib = load()
        self._h = ctypes.c_void_p()
        check(self._lib.sert_scorer_create(device, e.ctypes.data, e.shape[0], e.shape[1],
                                           ctypes.byref(self._h)))
        self._pin_q, self._pin_idx, self._pin_val = PinnedBuffer(np.float32), PinnedBuffer(np.int32), PinnedBuffer(np.float32)

    def query_buffer(self, num_queries):
        """A page-locked (Q, d) float32 array to build the query block in (zero-copy upload)."""
        return self._pin_q.view((num_queries, self.dim))

    def _stage(self, projections):
        p = np.asarray(projections, dtype=np.float32)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        assert p.shape[1] == self.dim
        if self._pin_q.holds(p):
            return p
        staged = self._pin_q.view(p.shape)
        np.copyto(staged, p)
        return staged

    def topk(self, projections, k):
        p = self._stage(projections)
        q = p.shape[0]
        idx = self._pin_idx.view((q, k))
        val = self._pin_val.view((q, k))
        check(self._lib.sert_scorer_topk(self._h, p.ctypes.data, q, k, idx.ctypes.data,
                                         val.ctypes.data))
        return idx, val

    def scores(self, projections):
        p = np.ascontiguousarray(projections, dtype=np.float32)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        assert p.shape[1] == self.dim
        out = np.empty((p.shape[0], self.num_entities), dtype=np.float32)
        check(self._lib.sert_scorer_scores(self._h, p.ctypes.data, p.shape[0], out.ctypes.data))
        return out

    def cosines(self, projections):
        """(Q, V_e) float32: the cosines topk() orders by and derives its scores from, bit for bit."""
        p = np.ascontiguousarray(projections, dtype=np.float32)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        assert p.shape[1] == self.dim
        out = np.empty((p.shape[0], self.num_entities), dtype=np.float32)
        check(self._lib.sert_scorer_cosines(self._h, p.ctypes.data, p.shape[0], out.ctypes.data))
        return out

    def debug_path_counts(self):
        """sert_debug_scorer_counts (test hook): [fused calls, of those bf16-filtered, fused chunks, flagged rows, rows of
        directly materialised calls, bf16 prefilter demoted]."""
        v = (ctypes.c_int64 * 6)()
        self._lib.sert_debug_scorer_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
        check(self._lib.sert_debug_scorer_counts(self._h, v, 6))
        return [int(x) for x in v]

    def debug_rank_counts(self):
        """sert_debug_scorer_rank_counts (test hook): [rank calls that reached the library, their query chunks, rows ranked by
        the top-k path, by the LDS sort, by the counting-sort passes, microseconds the copies of the two sorts' results took
        on the second stream]."""
        v = (ctypes.c_int64 * 6)()
        self._lib.sert_debug_scorer_rank_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
        check(self._lib.sert_debug_scorer_rank_counts(self._h, v, 6))
        return [int(x) for x in v]

    def rank(self, projections, k=None, on_device=True):
        """(idx, score) per query, best first; k=None ranks every entity.  One order whatever k: the cosine descending
        (-0 equal to +0), NaN after every number, ties by lowest entity index -- so rank(p, k) is the head of rank(p).
        k <= min(V_e, 1024) is topk() (views of the scorer's page-locked buffers); everything else is ranked on the device by
        sert_scorer_rank into ordinary arrays of the caller's (a 10 000 x 100 000 ranking is 8 GB: not to be page-locked).
        on_device=False: the same ranking by ordering sert_scorer_cosines on the host (the comparison path of the tests and
        of tools/score_rank_bench.py)."""
        if k is not None and k <= 0:
            raise SertError('Scorer.rank: k must be None (every entity) or positive')
        if k is not None and k <= min(self.num_entities, 1024):
            return self.topk(projections, k)
        p = np.ascontiguousarray(projections, dtype=np.float32)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        assert p.shape[1] == self.dim
        keep = self.num_entities if k is None else min(k, self.num_entities)
        idx = np.empty((p.shape[0], keep), dtype=np.int32)
        val = np.empty((p.shape[0], keep), dtype=np.float32)
        if on_device:
            check(self._lib.sert_scorer_rank(self._h, p.ctypes.data, p.shape[0], -1 if k is None else int(k), idx.ctypes.data,
                                             val.ctypes.data))
            return idx, val
        # full cosine rows, a bounded number of queries at a time (the reference scores one query at a time,
        # query.py:304-318; 10k queries x 100k entities in one block would be 4 GB of host memory)
        step = max(1, self.MAX_HOST_SCORES // self.num_entities)
        for lo in range(0, p.shape[0], step):
            # the COSINE is ordered; (cos + 1)/2 maps several cosines to one score, so the score is applied after
            # the sort.  -cos + 0: -0 and +0 become one value; NaN sorts last in numpy; stable: lowest index first
            cos = self.cosines(p[lo:lo + step])
            order = np.argsort(-cos + np.float32(0), axis=1, kind='stable')[:, :keep]
            idx[lo:lo + step] = order
            val[lo:lo + step] = (np.take_along_axis(cos, order, axis=1) + np.float32(1)) / np.float32(2)
        return idx, val

    def _queries(self, projections, count):
        p = np.ascontiguousarray(projections, dtype=np.float32)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        assert p.shape == (count, self.dim), (p.shape, count, self.dim)
        return p

    def score_pairs(self, projections, candidates, raw=False):
        """(indptr, values): the value of every (query, candidate) pair, candidates[q] the integer entity indices of query q
        -- in the caller's order, duplicates kept; query q's values are values[indptr[q]:indptr[q + 1]].  raw: the cosine
        itself, else (cos + 1) / 2 (sert_scorer_pairs)."""
        indptr, ents = candidates_csr(candidates)
        p = self._queries(projections, len(indptr) - 1)
        out = np.empty(len(ents), dtype=np.float32)
        # (the library refuses a null pointer: an empty array still has an address to give)
        e, o = (ents, out) if len(ents) else (np.zeros(1, np.int32), np.zeros(1, np.float32))
        check(self._lib.sert_scorer_pairs(self._h, p.ctypes.data, p.shape[0], indptr.ctypes.data, e.ctypes.data,
                                          1 if raw else 0, o.ctypes.data))
        return indptr, out

    def rank_candidates(self, projections, candidates, k=None):
        """(out_indptr, idx, score): each query's candidates ranked, best first, under the scorer's one order; k=None ranks
        the whole list, else its best min(k, length).  Query q's result is idx / score[out_indptr[q]:out_indptr[q + 1]].
        The lists may come in any order and with duplicates: they are sorted and de-duplicated here, as
        sert_scorer_rank_candidates requires."""
        if k is not None and k <= 0:
            raise SertError('Scorer.rank_candidates: k must be None (the whole list) or positive')
        indptr, ents = candidates_csr(candidates, unique=True)
        p = self._queries(projections, len(indptr) - 1)
        out_indptr = ranked_indptr(indptr, k)
        n = int(out_indptr[-1])
        idx = np.empty(max(n, 1), dtype=np.int32)
        val = np.empty(max(n, 1), dtype=np.float32)
        e = ents if len(ents) else np.zeros(1, np.int32)
        check(self._lib.sert_scorer_rank_candidates(self._h, p.ctypes.data, p.shape[0], indptr.ctypes.data, e.ctypes.data,
                                                    -1 if k is None else min(int(k), 2 ** 31 - 1), idx.ctypes.data, val.ctypes.data))
        return out_indptr, idx[:n], val[:n]

    def debug_rerank_counts(self):
        """sert_debug_scorer_rerank_counts (test hook): [score_pairs / rank_candidates calls, their chunks, queries ranked by
        the LDS kernel, by the slab and the counting-sort passes, pairs scored, empty lists]."""
        v = (ctypes.c_int64 * 6)()
        self._lib.sert_debug_scorer_rerank_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        check(self._lib.sert_debug_scorer_rerank_counts(self._h, v))
        return [int(x) for x in v]

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.sert_scorer_destroy(self._h)
            self._h = None
        for b in (getattr(self, '_pin_q', None), getattr(self, '_pin_idx', None), getattr(self, '_pin_val', None)):
            if b is not None:
                b.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RetrievalEval(object):
    """Owner of one sert_reval handle: topics and relevance judgements resident on the engine's device, ``run()`` ranks
    every topic with the engine's parameters as they are now and returns the per-topic metrics computed there.

    token_lists: per topic its token ids (at least one); judgements: per topic (entities int, ascending; gains float);
    ideal_dcg / num_rel: per topic, float64 / int, over ALL its judgements (sert_hip.h); k: None = every entity
    (loglinear, or counted).  counted=True: the evaluator by rank counting (sert_reval_create_counted: vectorspace kinds,
    any depth, no ranking -- ``judged_ranks()`` instead).  The engine must stay alive as long as this object."""

    def __init__(self, engine, token_lists, judgements, ideal_dcg, num_rel, k=None, counted=False):
        self._lib = load()
        self._engine = engine
        self._h = None
        self._tokens, self._offsets = _concat_queries(token_lists)
        q = len(token_lists)
        assert len(judgements) == q and len(ideal_dcg) == q and len(num_rel) == q
        indptr = np.zeros(q + 1, dtype=np.int64)
        np.cumsum([len(e) for e, _ in judgements], out=indptr[1:])
        ents = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.int64) for e, _ in judgements])
                                    if q else np.zeros(0, np.int64), dtype=np.int32)
        gains = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.float64) for _, g in judgements])
                                     if q else np.zeros(0), dtype=np.float32)
        idcg = np.ascontiguousarray(ideal_dcg, dtype=np.float64)
        nrel = np.ascontiguousarray(num_rel, dtype=np.int32)
        v = engine.cfg.num_entities
        self.num_topics = q
        self.depth = v if k is None or k >= v else int(k)
        self.counted = bool(counted)
        self.rel_indptr = indptr
        h = ctypes.c_void_p()
        create = self._lib.sert_reval_create_counted if counted else self._lib.sert_reval_create
        check(create(engine._h, self._tokens.ctypes.data, self._offsets.ctypes.data, q,
                     indptr.ctypes.data, ents.ctypes.data, gains.ctypes.data, idcg.ctypes.data,
                     nrel.ctypes.data, -1 if k is None else int(k), ctypes.byref(h)))
        self._h = h

    def run(self, return_ranking=False):
        """-> (metrics (Q, REVAL_NUM_METRICS) float64, status (Q,) int32[, idx (Q, depth) int32, score (Q, depth) f32])."""
        metrics = np.empty((self.num_topics, REVAL_NUM_METRICS), dtype=np.float64)
        status = np.empty(self.num_topics, dtype=np.int32)
        idx = score = None
        if return_ranking and self.counted:
            raise SertError('a counted RetrievalEval makes no ranking: judged_ranks() has the ranks, Scorer.rank a ranking')
        if return_ranking:
            idx = np.empty((self.num_topics, self.depth), dtype=np.int32)
            score = np.empty((self.num_topics, self.depth), dtype=np.float32)
        check(self._lib.sert_reval_run(self._h, metrics.ctypes.data, status.ctypes.data, _addr(idx), _addr(score)))
        return (metrics, status, idx, score) if return_ranking else (metrics, status)

    def judged_ranks(self):
        """Counted evaluators: the 1-based ranks the last run() found, int32, aligned with the concatenated judgement lists
        (topic q owns [rel_indptr[q], rel_indptr[q + 1])); not cut at the depth."""
        ranks = np.zeros(int(self.rel_indptr[-1]), dtype=np.int32)
        check(self._lib.sert_reval_judged_ranks(self._h, ranks.ctypes.data))
        return ranks

    def num_chunks(self):
        """sert_debug_reval_chunks (test hook): chunks the topics are ranked in."""
        self._lib.sert_debug_reval_chunks.argtypes = [ctypes.c_void_p]
        return int(self._lib.sert_debug_reval_chunks(self._h))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.sert_reval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _FoldHandle(object):
    """What the owners of the four fold-in handles share: the handle ``_h``, the prefix of its library functions, the
    (x, y, w) upload validation, the batch calls and the destruction (_NceFoldHandle, _LlFoldHandle: what two of them share)."""

    _prefix = None          # 'sert_foldin_', 'sert_wfold_', 'sert_ll_foldin_', 'sert_ll_wfold_'

    def _fn(self, name):
        return getattr(self._lib, self._prefix + name)

    def _x(self, x):
        x = np.ascontiguousarray(x, dtype=np.int32)
        return x, x.ndim == 2 and x.shape[1] == self.window_size

    @staticmethod
    def _w(w, M):
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (M,):
                raise SertError('w must be (M,)')
        return w

    def upload(self, x, y, w=None):
        x, ok = self._x(x)
        y = np.ascontiguousarray(y, dtype=np.int32)
        if not ok or y.shape != (x.shape[0],):
            raise SertError('x must be (M, window_size) and y (M,)')
        w = self._w(w, x.shape[0])
        check(self._fn('upload')(self._h, x.ctypes.data, y.ctypes.data, _addr(w), x.shape[0]))

    def num_batches(self):
        return int(self._fn('num_batches')(self._h))

    def _loss_of(self, name, batch_index, *args):
        loss = ctypes.c_float()
        check(self._fn(name)(self._h, int(batch_index), *(args + (ctypes.byref(loss),))))
        return np.float32(loss.value)

    def train_batch(self, batch_index):
        return self._loss_of('train_batch', batch_index)

    def train_batches(self, batch_indices):
        idx = np.ascontiguousarray(batch_indices, dtype=np.int64)
        out = np.empty(idx.size, dtype=np.float32)
        check(self._fn('train_batches')(self._h, idx.ctypes.data, idx.size, out.ctypes.data))
        return out

    def eval_batch(self, batch_index):
        return self._loss_of('eval_batch', batch_index)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._fn('destroy')(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _NceFoldHandle(_FoldHandle):
    """The two handles of a vectorspace model on top of it: the NCE negatives, the rows and Adam's moments, the sampler's
    counters and the config (sert_foldin_config and sert_wfold_config have the same fields)."""

    _config = None          # SertFoldInConfig, SertWFoldConfig
    _rows_shape = None      # of get_rows: set by the constructor

    def _fill_config(self, batch_size, num_negatives, lambda_, lr, beta1, beta2, eps, seed):
        c = self._config()
        c.struct_size = ctypes.sizeof(self._config)
        c.batch_size, c.num_negatives, c.lambda_ = int(batch_size), int(num_negatives), float(lambda_)
        c.lr, c.beta1, c.beta2, c.eps, c.seed = float(lr), float(beta1), float(beta2), float(eps), int(seed)
        self.cfg = c
        return c

    def _negatives(self, negatives):
        if negatives is not None:
            negatives = np.ascontiguousarray(negatives, dtype=np.int64)
            assert negatives.size == self.cfg.batch_size * self.cfg.num_negatives
        return negatives

    def train_batch(self, batch_index, negatives=None):
        return self._loss_of('train_batch', batch_index, _addr(self._negatives(negatives)))

    def eval_batch(self, batch_index, negatives=None):
        return self._loss_of('eval_batch', batch_index, _addr(self._negatives(negatives)))

    def negatives_of_step(self, position, evaluation=False):
        """(B, z) int64 in the range the handle draws from (FoldIn: [0, num_entities + num_new); WordFoldIn:
        [0, num_entities)): what the device sampler draws at training position `position` (= get_step() before the step) or
        for the `position`-th evaluation draw."""
        out = np.empty((self.cfg.batch_size, self.cfg.num_negatives), dtype=np.int64)
        check(self._fn('negatives_of_step')(self._h, int(position), int(bool(evaluation)), out.ctypes.data))
        return out

    def get_rows(self, which=0):
        """``which``: FOLDIN_ROWS / _M / _V, or WFOLD_ROWS / _M / _V (the same three values)."""
        out = np.empty(self._rows_shape, dtype=np.float32)
        check(self._fn('get_rows')(self._h, int(which), out.ctypes.data, out.size))
        return out

    def set_rows(self, which, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        check(self._fn('set_rows')(self._h, int(which), a.ctypes.data, a.size))

    def set_step(self, t):
        check(self._fn('set_step')(self._h, int(t)))

    def get_step(self):
        return int(self._fn('get_step')(self._h))

    def set_eval_draws(self, n):
        check(self._fn('set_eval_draws')(self._h, int(n)))

    def get_eval_draws(self):
        return int(self._fn('get_eval_draws')(self._h))


class _LlFoldHandle(_FoldHandle):
    """The two handles of a loglinear model on top of it: the Adadelta config (sert_ll_foldin_config and sert_ll_wfold_config
    have the same fields) and the upload of label rows."""

    _config = None          # SertLlFoldInConfig, SertLlWFoldConfig

    def _fill_config(self, batch_size, lambda_, lr, rho, eps, max_cache_bytes):
        c = self._config()
        c.struct_size = ctypes.sizeof(self._config)
        c.batch_size, c.lambda_ = int(batch_size), float(lambda_)
        c.lr, c.rho, c.eps, c.max_cache_bytes = float(lr), float(rho), float(eps), int(max_cache_bytes)
        self.cfg = c
        return c

    def upload_csr(self, x, indptr, indices, data, w=None):
        """Label ROWS: a canonical CSR matrix whose column e < num_entities is trained entity e.  LlFoldIn: (M, num_entities +
        num_new), a trained column is a label only and column num_entities + j is new entity j; LlWordFoldIn: (M,
        num_entities), as the model's own training without one-hot classes learns them.  The library validates the rows."""
        x, ok = self._x(x)
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float32)
        if not ok or indptr.shape != (x.shape[0] + 1,):
            raise SertError('x must be (M, window_size) and indptr (M + 1,)')
        # (what the library cannot see: the arrays must be as long as indptr says before it reads them)
        if indices.ndim != 1 or data.shape != indices.shape or (indptr.size and indices.size < indptr.max()):
            raise SertError('indices and data must be (nnz,) with nnz >= max(indptr)')
        w = self._w(w, x.shape[0])
        check(self._fn('upload_csr')(self._h, x.ctypes.data, indptr.ctypes.data, _addr(indices), _addr(data), _addr(w), x.shape[0]))


def _refresh_ids(refresh_ids):
    given = np.asarray(refresh_ids)
    ids = np.ascontiguousarray(given, dtype=np.int32)
    if ids.ndim != 1 or not np.array_equal(ids, given):
        raise SertError('refresh_ids must be a 1-d array of int32 entity indices')
    return ids


class FoldIn(_NceFoldHandle):
    """Owner of one sert_foldin handle (include/sert_hip_foldin.h): ``num_new`` entity rows learnt on top of the frozen
    parameters of ``engine`` (a vectorspace Engine), which are copied at construction -- the engine may train on or be
    closed afterwards.

    ``refresh_ids`` (an array of trained internal indices, possibly empty; None: sert_foldin_create as ever): a REFRESH
    handle (sert_foldin_create_refresh) whose ``num_rows = len(refresh_ids) + num_new`` trainable rows are slots -- the
    refreshed trained rows in the order given, then the new rows; ``new_rows_init`` may then be None (no new entity), y at
    upload is a slot, and get_rows / set_rows are in slot order."""

    _prefix, _config = 'sert_foldin_', SertFoldInConfig

    def __init__(self, engine, new_rows_init, batch_size, num_negatives, lambda_, lr=1e-3, beta1=0.9, beta2=0.999,
                 eps=1e-8, seed=0, refresh_ids=None):
        self._lib = load()
        self._h = None
        if new_rows_init is None and refresh_ids is not None:
            new_rows_init = np.zeros((0, engine.cfg.entity_dim), dtype=np.float32)
        rows = np.ascontiguousarray(new_rows_init, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != engine.cfg.entity_dim:
            raise SertError('new_rows_init must be (num_new, entity_dim)')
        c = self._fill_config(batch_size, num_negatives, lambda_, lr, beta1, beta2, eps, seed)
        self.num_new, self.entity_dim = int(rows.shape[0]), int(rows.shape[1])
        self.num_entities = int(engine.cfg.num_entities)
        self.window_size = int(engine.cfg.window_size)
        h = ctypes.c_void_p()
        if refresh_ids is None:
            self.num_refresh = 0
            check(self._lib.sert_foldin_create(engine._h, self.num_new, rows.ctypes.data if rows.size else None,
                                               ctypes.byref(c), ctypes.byref(h)))
        else:
            ids = _refresh_ids(refresh_ids)
            self.num_refresh = int(ids.size)
            check(self._lib.sert_foldin_create_refresh(engine._h, ids.ctypes.data if ids.size else None, self.num_refresh,
                                                       self.num_new, rows.ctypes.data if rows.size else None,
                                                       ctypes.byref(c), ctypes.byref(h)))
        self.num_rows = self.num_refresh + self.num_new         # the trainable rows E
        self._rows_shape = (self.num_rows, self.entity_dim)
        self._h = h

    def plan(self):
        """sert_debug_foldin_plan (test hook): what the last step of this handle launched -- 'loss' (none / vector / scalar),
        'k' (its template parameter), 'train', 'sort_bits', 'passes', 'vec', 'nch' and 'col_passes' of foldin_chunk_reduce,
        'fixup' (none / wave / workgroup), 'tiles' of the sort.  All zero before the first step; an evaluation rewrites the
        first three entries only."""
        v = (ctypes.c_int32 * 10)()
        self._lib.sert_debug_foldin_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_foldin_plan(self._h, v, 10))
        v = [int(x) for x in v]
        return {'loss': FOLDIN_LOSS_FORMS[v[0]], 'k': v[1], 'train': bool(v[2]), 'sort_bits': v[3], 'passes': v[4], 'vec': v[5],
                'nch': v[6], 'col_passes': v[7], 'fixup': EGRAD_FIXUPS[v[8]], 'tiles': v[9]}

    def table(self):
        """sert_debug_foldin_table (test hook): how this handle addresses its trainable rows -- 'map' (True: the loss kernels
        that look a negative up in slot_of, sert_foldin_create_refresh), 'num_refresh', 'num_new', 'rows' (= Nt)."""
        v = (ctypes.c_int32 * 4)()
        self._lib.sert_debug_foldin_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        check(self._lib.sert_debug_foldin_table(self._h, v, 4))
        return {'map': bool(v[0]), 'num_refresh': int(v[1]), 'num_new': int(v[2]), 'rows': int(v[3])}


class WordFoldIn(_NceFoldHandle):
    """Owner of one sert_wfold handle (include/sert_hip_wfold.h): ``num_new_words`` word rows learnt on top of the frozen
    parameters of ``engine`` (a vectorspace Engine), which are copied at construction -- the engine may train on or be
    closed afterwards.  New word v is token id ``vocab_size + v``; labels and negatives are trained entities."""

    _prefix, _config = 'sert_wfold_', SertWFoldConfig

    def __init__(self, engine, new_rows_init, batch_size, num_negatives, lambda_, lr=1e-3, beta1=0.9, beta2=0.999,
                 eps=1e-8, seed=0):
        self._lib = load()
        self._h = None
        rows = np.ascontiguousarray(new_rows_init, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != engine.cfg.word_dim:
            raise SertError('new_rows_init must be (num_new_words, word_dim)')
        c = self._fill_config(batch_size, num_negatives, lambda_, lr, beta1, beta2, eps, seed)
        self.num_new_words, self.word_dim = int(rows.shape[0]), int(rows.shape[1])
        self._rows_shape = (self.num_new_words, self.word_dim)
        self.vocab_size = int(engine.cfg.vocab_size)
        self.num_entities = int(engine.cfg.num_entities)
        self.window_size = int(engine.cfg.window_size)
        h = ctypes.c_void_p()
        check(self._lib.sert_wfold_create(engine._h, self.num_new_words, rows.ctypes.data if rows.size else None,
                                          ctypes.byref(c), ctypes.byref(h)))
        self._h = h

    def plan(self):
        """sert_debug_wfold_plan (test hook): what the last step of this handle launched -- 'project' (none / vector / scalar:
        the instance of wfold_project), 'loss' (per_candidate: vs_nce; scalar: vs_nce_scalar), 'k' (its template parameter),
        'train', 'levels' of the batch's reduction and its 'items' per level, 'segsum' (rows32 / rows64 / scalar; none without
        a level), 'gemm_p' / 'gemm_g' (GEMM_ROUTES; gemm_g is 'none' after an evaluation).  All zero before the first step."""
        v = (ctypes.c_int32 * 16)()
        check(self._lib.sert_debug_wfold_plan(self._h, v, 16))
        v = [int(x) for x in v]
        route = lambda code: GEMM_ROUTES[code - 1] if code >= 1 else 'none'
        return {'project': WFOLD_PROJECT_FORMS[v[0]], 'loss': NCE_FORMS[v[1]], 'k': v[2], 'train': bool(v[3]), 'levels': v[4],
                'items': v[5:5 + v[4]], 'segsum': WGRAD_FORMS[v[11]], 'gemm_p': route(v[12]), 'gemm_g': route(v[13])}


def debug_wfold_index(tok, num_words, batch=0):
    """Host only (sert_debug_wfold_index): the inverted index a word fold-in builds for batch `batch` of tok
    (num_batches, B, n) int32 -- the new word of every position, or -1.  Returns a dict: 'levels', 'item_counts' and 'part_off'
    per level, 'rows' (the entries: batch rows) and 'items' (k, 4) int32 {begin, end, dst, 0}, level after level."""
    lib = load()
    tok = np.ascontiguousarray(tok, dtype=np.int32)
    assert tok.ndim == 3, tok.shape
    nb, B, n = tok.shape
    levels = np.zeros(13, dtype=np.int32)
    nr, ni = ctypes.c_int64(), ctypes.c_int64()
    args = (_addr(tok), nb, B, n, int(num_words), int(batch), levels.ctypes.data)
    check(lib.sert_debug_wfold_index(*(args + (None, 0, None, 0, ctypes.byref(nr), ctypes.byref(ni)))))
    rows = np.zeros(max(1, nr.value), dtype=np.int32)
    items = np.zeros((max(1, ni.value), 4), dtype=np.int32)
    check(lib.sert_debug_wfold_index(*(args + (rows.ctypes.data, rows.size, items.ctypes.data, items.shape[0], ctypes.byref(nr),
                                               ctypes.byref(ni)))))
    L = int(levels[0])
    return {'levels': L, 'item_counts': [int(x) for x in levels[1:1 + L]], 'part_off': [int(x) for x in levels[7:7 + L]],
            'rows': rows[:nr.value].copy(), 'items': items[:ni.value].copy()}


class LlFoldIn(_LlFoldHandle):
    """Owner of one sert_ll_foldin handle (include/sert_hip_ll_foldin.h): ``num_new`` columns of W and entries of b learnt
    on top of the frozen parameters of ``engine`` (a loglinear Engine), which are copied at construction -- the engine may
    train on or be closed afterwards.  ``init_W``: (word_dim, num_new); ``init_b``: (num_new,) or None (zeros).

    ``refresh_ids`` (distinct trained columns, any order; sert_ll_foldin_create_refresh): these trained columns learn too.
    The trainable columns are then ``num_slots`` = ``num_refresh`` + ``num_new`` SLOTS, the refreshed columns first in the
    order given: integer labels are slots, the tensors are (word_dim, num_slots) / (num_slots,) in slot order, and ``init_W``
    may be None or empty (nothing is new).  Label rows keep the public columns [0, num_entities + num_new)."""

    _prefix, _config = 'sert_ll_foldin_', SertLlFoldInConfig

    def __init__(self, engine, init_W, init_b, batch_size, lambda_, lr=1.0, rho=0.95, eps=1e-6, max_cache_bytes=0,
                 refresh_ids=None):
        self._lib = load()
        self._h = None
        if init_W is None and refresh_ids is not None:
            init_W = np.zeros((engine.cfg.word_dim, 0), dtype=np.float32)
        Wn = np.ascontiguousarray(init_W, dtype=np.float32)
        if Wn.ndim != 2 or Wn.shape[0] != engine.cfg.word_dim:
            raise SertError('init_W must be (word_dim, num_new)')
        bn = None
        if init_b is not None:
            bn = np.ascontiguousarray(init_b, dtype=np.float32)
            if bn.shape != (Wn.shape[1],):
                raise SertError('init_b must be (num_new,)')
        c = self._fill_config(batch_size, lambda_, lr, rho, eps, max_cache_bytes)
        self.word_dim, self.num_new = int(Wn.shape[0]), int(Wn.shape[1])
        self.num_entities = int(engine.cfg.num_entities)
        self.window_size = int(engine.cfg.window_size)
        h = ctypes.c_void_p()
        if refresh_ids is None:
            self.num_refresh = 0
            check(self._lib.sert_ll_foldin_create(engine._h, self.num_new, Wn.ctypes.data if Wn.size else None, _addr(bn),
                                                  ctypes.byref(c), ctypes.byref(h)))
        else:
            ids = _refresh_ids(refresh_ids)
            self.num_refresh = int(ids.size)
            check(self._lib.sert_ll_foldin_create_refresh(engine._h, ids.ctypes.data if ids.size else None, self.num_refresh,
                                                          self.num_new, Wn.ctypes.data if Wn.size else None,
                                                          _addr(bn) if Wn.size else None, ctypes.byref(c), ctypes.byref(h)))
        self.num_slots = self.num_refresh + self.num_new        # the trainable columns
        self._h = h

    def _shape(self, which):
        if which not in (LL_FOLDIN_W, LL_FOLDIN_B, LL_FOLDIN_ACCU_W, LL_FOLDIN_ACCU_B, LL_FOLDIN_DELTA_W, LL_FOLDIN_DELTA_B):
            raise SertError('which must be one of LL_FOLDIN_W, _B, _ACCU_W, _ACCU_B, _DELTA_W, _DELTA_B')
        return (self.num_slots,) if which in (LL_FOLDIN_B, LL_FOLDIN_ACCU_B, LL_FOLDIN_DELTA_B) else (self.word_dim, self.num_slots)

    def get_tensor(self, which):
        out = np.empty(self._shape(int(which)), dtype=np.float32)
        check(self._lib.sert_ll_foldin_get_tensor(self._h, int(which), out.ctypes.data, out.size))
        return out

    def set_tensor(self, which, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        check(self._lib.sert_ll_foldin_set_tensor(self._h, int(which), a.ctypes.data, a.size))

    def layout(self):
        """sert_debug_ll_foldin_layout (test hook): (V_f, Nt, internal_of) -- the frozen and the trainable columns the step
        kernels see and the internal column of every public column [0, num_entities + num_new)."""
        vf, nt = ctypes.c_int32(), ctypes.c_int32()
        out = np.empty(self.num_entities + self.num_new, dtype=np.int32)
        self._lib.sert_debug_ll_foldin_layout.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                                          ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int64]
        check(self._lib.sert_debug_ll_foldin_layout(self._h, ctypes.byref(vf), ctypes.byref(nt), out.ctypes.data, out.size))
        return int(vf.value), int(nt.value), out


class LlWordFoldIn(_LlFoldHandle):
    """Owner of one sert_ll_wfold handle (include/sert_hip_ll_wfold.h): ``num_new_words`` word rows learnt on top of the frozen
    parameters of ``engine`` (a loglinear Engine), which are copied at construction -- the engine may train on or be closed
    afterwards.  New word v is token id ``vocab_size + v``; labels are trained entities."""

    _prefix, _config = 'sert_ll_wfold_', SertLlWFoldConfig

    def __init__(self, engine, new_rows_init, batch_size, lambda_, lr=1.0, rho=0.95, eps=1e-6, max_cache_bytes=0):
        self._lib = load()
        self._h = None
        rows = np.ascontiguousarray(new_rows_init, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != engine.cfg.word_dim:
            raise SertError('new_rows_init must be (num_new_words, word_dim)')
        c = self._fill_config(batch_size, lambda_, lr, rho, eps, max_cache_bytes)
        self.num_new_words, self.word_dim = int(rows.shape[0]), int(rows.shape[1])
        self._rows_shape = (self.num_new_words, self.word_dim)
        self.vocab_size = int(engine.cfg.vocab_size)
        self.num_entities = int(engine.cfg.num_entities)
        self.window_size = int(engine.cfg.window_size)
        h = ctypes.c_void_p()
        check(self._lib.sert_ll_wfold_create(engine._h, self.num_new_words, rows.ctypes.data if rows.size else None,
                                             ctypes.byref(c), ctypes.byref(h)))
        self._h = h

    def get_rows(self, which=0):
        """``which``: LL_WFOLD_ROWS (Nv) / LL_WFOLD_ACCU / LL_WFOLD_DELTA (Adadelta's accumulators of Nv)."""
        out = np.empty(self._rows_shape, dtype=np.float32)
        check(self._lib.sert_ll_wfold_get_rows(self._h, int(which), out.ctypes.data, out.size))
        return out

    def set_rows(self, which, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        check(self._lib.sert_ll_wfold_set_rows(self._h, int(which), a.ctypes.data, a.size))

    def plan(self):
        """sert_debug_ll_wfold_plan (test hook): what the last step of this handle launched -- 'form' (none / reg / stream: the
        instance of llw_row), 'vec' (16-byte rows), 'train', 'levels' of the batch's reduction and its 'items' per level,
        'segsum' (rows64 / scalar; none without a level), 'gemm_z' / 'gemm_g' (GEMM_ROUTES; gemm_g is 'none' after an
        evaluation), 'splits' (the k ranges of G), 'labels' (int / rows: the upload's label kind, which picks llw_row or
        llw_row_csr).  All zero before the first step."""
        v = (ctypes.c_int32 * 16)()
        check(self._lib.sert_debug_ll_wfold_plan(self._h, v, 16))
        v = [int(x) for x in v]
        route = lambda code: GEMM_ROUTES[code - 1] if code >= 1 else 'none'
        return {'form': LL_WFOLD_FORMS[v[0]], 'vec': bool(v[1]), 'train': bool(v[2]), 'levels': v[3], 'items': v[4:4 + v[3]],
                'segsum': WGRAD_FORMS[v[10]], 'gemm_z': route(v[11]), 'gemm_g': route(v[12]), 'splits': v[13],
                'labels': LL_WFOLD_LABELS[v[14]]}


def bench_gemm(M, N, K, ta=0, tb=0, epi=0, splits=1, iters=20, device=0):
    """Average launch time (us) of the fp32 MFMA GEMM on random device operands."""
    us = ctypes.c_double()
    check(load().sert_bench_gemm(device, ta, tb, epi, M, N, K, splits, iters, ctypes.byref(us)))
    return us.value


MEMBENCH_COPY, MEMBENCH_READ, MEMBENCH_GATHER, MEMBENCH_OPTIMIZER = 0, 1, 2, 3
SEPARATE_ALLOCATIONS = ctypes.c_size_t(-1).value


def debug_word_index_sum(ids, vocab, src, batch=0, row_groups=1, dense_heavy=False, divisor=1.0, sort_level0=False):
    """Host only: the word-table gradient of one batch through the inverted index as the segmented-sum kernels walk it
    (sert_debug_word_index_sum).  ids (num_batches, B, n) unsigned; src (B, d) float32.  sort_level0: level 0 sorted by item
    length with every item's first row number in its descriptor (what the vectorspace models upload).  Returns (grad (vocab, d), stats)."""
    lib = load()
    ids = np.ascontiguousarray(ids)
    assert ids.ndim == 3 and ids.dtype in (np.uint8, np.uint16, np.uint32), (ids.shape, ids.dtype)
    src = np.ascontiguousarray(src, dtype=np.float32)
    nb, B, n = ids.shape
    assert src.shape[0] == B
    d = src.shape[1]
    out = np.empty((vocab, d), dtype=np.float32)
    stats = np.zeros(11, dtype=np.int64)
    lib.sert_debug_word_index_sum.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                              ctypes.c_void_p, ctypes.c_void_p]
    check(lib.sert_debug_word_index_sum(_addr(ids), ids.dtype.itemsize, nb, B, n, int(vocab), int(row_groups), int(bool(dense_heavy)) | (2 if sort_level0 else 0),
                                        int(batch), _addr(src), d, float(divisor), _addr(out), _addr(stats)))
    keys = ('levels', 'items', 'partial_rows', 'final_items', 'dense_words', 'row_groups', 'level0_items', 'distinct_words',
            'fused_upper_ok', 'heavy_cnt', 'level1_items')
    return out, dict(zip(keys, [int(x) for x in stats]))


def debug_gemm(A, B, ta=0, tb=0, epi=0, bias=None, device=0):
    """C = epi(op(A).op(B)) through the library's GEMM dispatch (sert_debug_gemm); shapes from the arrays."""
    lib = load()
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    K, M = A.shape if ta else A.shape[::-1]
    N = B.shape[0] if tb else B.shape[1]
    assert (B.shape[1] if tb else B.shape[0]) == K, (A.shape, B.shape)
    C = np.empty((M, N), dtype=np.float32)
    if bias is not None:
        bias = np.ascontiguousarray(bias, dtype=np.float32)
    lib.sert_debug_gemm.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 4
    check(lib.sert_debug_gemm(device, int(ta), int(tb), int(epi), M, N, K, _addr(A), _addr(B),
                              _addr(bias) if bias is not None else None, _addr(C)))
    return C


def debug_gemm_splitk(A, B, splits, device=0):
    """(A^T.B, column sums of B) through the split-K launch + combine of a training step (sert_debug_gemm_splitk);
    A (K, M), B (K, N)."""
    lib = load()
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    K, M = A.shape
    N = B.shape[1]
    assert B.shape[0] == K
    out = np.empty(M * N + N, dtype=np.float32)
    lib.sert_debug_gemm_splitk.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    check(lib.sert_debug_gemm_splitk(device, M, N, K, int(splits), _addr(A), _addr(B), _addr(out)))
    return out[:M * N].reshape(M, N), out[M * N:]


def debug_gemm_longk(A, B, splits, tb=0, device=0):
    """A.op(B) over a long K cut into `splits` k ranges + combine (sert_debug_gemm_longk); A (M, K), B (K, N) or (N, K) if tb."""
    lib = load()
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    M, K = A.shape
    N = B.shape[0] if tb else B.shape[1]
    assert (B.shape[1] if tb else B.shape[0]) == K
    out = np.empty((M, N), dtype=np.float32)
    lib.sert_debug_gemm_longk.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3
    check(lib.sert_debug_gemm_longk(device, int(tb), M, N, K, int(splits), _addr(A), _addr(B), _addr(out)))
    return out


GEMM_FORM_PLAIN, GEMM_FORM_SPLITK, GEMM_FORM_LONGK = 0, 1, 2
# sert_debug_gemm_route's codes (include/sert_hip_debug.h: SERT_GEMM_ROUTE_*), in order from 1
GEMM_ROUTES = ('f32_tile64', 'f32_tile128', 'f32_tile128x160', 'x3_128_vec', 'x3_128_scalar', 'x3_256', 'x3_320',
               'x3_ta_single', 'x3_ta_320x160', 'x3_ta_tiles')


def debug_gemm_route(form, M, N, K, ta=0, tb=0, splits=1, align=16):
    """The kernel debug_gemm (GEMM_FORM_PLAIN), debug_gemm_splitk or debug_gemm_longk would launch for a shape, by name
    (GEMM_ROUTES) -- sert_debug_gemm_route: host only, the launchers' own predicates."""
    lib = load()
    lib.sert_debug_gemm_route.argtypes = [ctypes.c_int] * 8
    code = lib.sert_debug_gemm_route(int(form), int(ta), int(tb), int(M), int(N), int(K), int(splits), int(align))
    if code < 1 or code > len(GEMM_ROUTES):
        raise SertError('sert_debug_gemm_route: %s' % (lib.sert_last_error() or b'').decode())
    return GEMM_ROUTES[code - 1]


def bench_memory(kind, nbytes, table_bytes=0, row_bytes=512, window=10, gap_bytes=0, blocks=0, iters=20, device=0):
    """Average launch time (us) of a memory-system micro-benchmark (include/sert_hip.h:
    sert_bench_memory): stream copy / read, the window gather over random rows, the dense
    optimiser's seven streams."""
    us = ctypes.c_double()
    check(load().sert_bench_memory(device, kind, nbytes, table_bytes, row_bytes, window, gap_bytes, blocks, iters,
                                   ctypes.byref(us)))
    return us.value


def debug_row_lists(allbits, rank, rows_per_rank, vocab, batch):
    """sert_debug_row_lists (host only): the exchange lists of one rank and batch as numpy arrays."""
    allbits = np.ascontiguousarray(allbits, dtype=np.uint32)
    world, nb, bw = allbits.shape
    cap = int(vocab) + 2
    i32 = lambda n: np.zeros(n, dtype=np.int32)
    scnt, fcnt = i32(world), i32(world)
    srows, frows, urows, ptr, ent = (i32(cap * world) for _ in range(5))
    sizes = np.zeros(5, dtype=np.int64)
    check(load().sert_debug_row_lists(allbits.ctypes.data, world, rank, nb, bw, rows_per_rank, vocab, batch,
                                      scnt.ctypes.data, fcnt.ctypes.data, srows.ctypes.data, frows.ctypes.data,
                                      urows.ctypes.data, ptr.ctypes.data, ent.ctypes.data, cap * world, sizes.ctypes.data))
    ns, nf, nu, ne = (int(x) for x in sizes[:4])
    return dict(serve_cnt=scnt, fetch_cnt=fcnt, serve_rows=srows[:ns], fetch_rows=frows[:nf], union_rows=urows[:nu],
                ptr=ptr[:nu + 1], ent=ent[:ne], max_xfer_rows=int(sizes[4]))


class profile_range(object):
    """with profile_range('epoch 3'): ...   -- a roctx range (sert_profile_range_push / pop)."""

    def __init__(self, name):
        self.name = name.encode() if isinstance(name, str) else name

    def __enter__(self):
        check(load().sert_profile_range_push(self.name))
        return self

    def __exit__(self, *exc):
        check(load().sert_profile_range_pop())
