/*
 * sert_hip_debug.h -- test hooks and micro-benchmarks of libsert_hip.so.
 *
 * NOT part of the drop-in boundary (include/sert_hip.h is): nothing here replaces a reference function and no product code
 * path (sert_amd/models.py, inference.py, scoring.py, training.py, bin/) calls these.  They exist so that
 *   - every GEMM kernel of the library can be pinned against float64, and against products known to the bit, on host
 *     arrays (tests/test_gpu_gemm.py), and the kernel a shape is routed to can be asked for (sert_debug_gemm_route),
 *   - the host-side index / exchange-list builders can be checked without a GPU (tests/test_word_index_cpu.py,
 *     tests/test_row_exchange_cpu.py),
 *   - bench.py can measure the denominators of its roofline fractions on the box it runs on (sert_bench_memory).
 * Same conventions as sert_hip.h (0 = ok, sert_last_error()).
 */
#ifndef SERT_HIP_DEBUG_H
#define SERT_HIP_DEBUG_H

#include "sert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Launches of the word-table update (sert/models.py:548-549 applied to R_w) by kernel form since sert_create -- host
 * counters, test hook: out[0] dense (adam_l2 / adadelta_l2), out[1] dense_update_lazy, out[2..7] dense_update_skip
 * <32,1> <64,1> <32,3> <64,2> <64,3> <64,4> (lanes per row, float4 columns per lane), out[8] the dense_update_skip passes
 * that read and wrote every row, out[9] its sparse passes.  n <= 10.  The tests assert through this that every template
 * shape met the oracle (tests/test_gpu_skip_shapes.py). */
int sert_debug_update_counts(sert_model* m, int64_t* out, int n);

/* Tail launches of the single-GPU vectorspace step (split-K combine of dW / db, the W, b update, the loss) since sert_create
 * -- host counters, test hook: out[0] launched alone (vs_tail), out[1] launched as the leading workgroups of the next
 * batch's gather (vs_gather_mean_tail: hinted steps, sert_hint_next_batch).  n <= 2.  (tests/test_gpu_tail_in_gather.py) */
int sert_debug_tail_counts(sert_model* m, int64_t* out, int n);

/* Transitions of the state one training step leaves for the next call (a run-ahead step, rows of the lazy word table that are
 * behind, a deferred entity-table update, the sums of squares of R_e handed from step to step) since sert_create -- host
 * counters incremented where the transition is made, test hook, no device is touched and nothing that is launched depends on
 * them: out[0] run-ahead steps discarded (a wrong hint, explicit negatives, any call that invalidates the speculation),
 * out[1] run-ahead steps consumed by the step they were issued for, out[2] flushes of the lazy word table (every row brought
 * to the step counter), out[3] deferred entity-table updates a later reader of R_e waited for, and the deferring steps whose
 * sums of squares of R_e out[4] were left by the previous step's launch, out[5] came from a read-only pass over a small table
 * (sumsq_like_small), out[6] from one over a big table (sumsq_like_adam).  n <= 7.  tests/test_gpu_op_sequences.py asserts
 * through this that the calls it puts between two steps met the state they are there to break. */
int sert_debug_state_counts(sert_model* m, int64_t* out, int n);

/* The loss form the LAST loglinear forward of this model launched (sert_train_batch, sert_eval_batch, ...) -- host record, test
 * hook, no device is touched: out[0] one of SERT_LL_FORM_*, out[1] its template parameter (WAVE: float4 chunks per lane 1 / 2 /
 * 4 / 8; TABLE and FUSED_ROW: threads per row 128 / 512; STREAM: 1 = 16-byte rows (V_e % 4 == 0), 0 = scalar rows), out[2] 1 for
 * the training instance of the form and 0 for the evaluating one, out[3] 1 when the logits were read from the distinct-word
 * table through the per-token slots, out[4] the segments per row of the streaming form (0 otherwise).  n <= 5; all zero before
 * the first forward.  tests/test_gpu_ll_csr.py asserts through this that every label structure reaches the kernel it is there
 * for: a threshold of the dispatch that moves takes the case off its kernel, and the test says so. */
enum {
    SERT_LL_FORM_NONE = 0,
    SERT_LL_FORM_WAVE = 1,       /* ll_row_wave<E>: one wave per row, labels serially on the owner lane */
    SERT_LL_FORM_TABLE = 2,      /* ll_row_from_table<NT>: per-thread label fix-up list */
    SERT_LL_FORM_FUSED_ROW = 3,  /* ll_fused_row<TRAIN, NT>: the (n, V_e) slab in LDS, per-thread label fix-up list */
    SERT_LL_FORM_STREAM = 4,     /* ll_s_*: label fix-ups in memory (ll_s_rowloss, ll_s_labfix) */
    SERT_LL_FORM_ROWWISE = 5     /* ll_softmax_rows + ll_window (cross-check knob of a variants build) */
};
int sert_debug_ll_loss_form(sert_model* m, int32_t* out, int n);

/* What the LAST vectorspace backward of this model launched for dR_e, the entity-table gradient (csrc/kernels_egrad.h, dispatch
 * in csrc/host/step_vectorspace.inc; the sorted chain's in csrc/host/lazy_segsum.inc: EntityChain) -- host record written where the launches are made, test hook, no device is touched:
 * out[0] one of SERT_EGRAD_PATH_*.  BUCKET: out[1] rows per sub-group, out[2] sub-groups, out[3] sub-groups per row group,
 * out[4] row groups, out[5] ranges of 16 entities, out[6] 1 when egrad_group_sum was launched and 0 when the sum of the group
 * tables was left to the optimiser.  SORTED: out[7] key bits of the counting sort, out[8] its digit passes, out[9] / out[10] VEC
 * and NCH of egrad_chunk_reduce<VEC, NCH>, out[11] one of SERT_EGRAD_FIXUP_*.  The entries of the path not taken are 0.  n <= 12;
 * all zero before the first backward.  tests/test_gpu_egrad_keys.py asserts through this that every key structure of
 * tests/egrad_key_cases.py reaches the kernels it is there for. */
enum { SERT_EGRAD_PATH_NONE = 0, SERT_EGRAD_PATH_BUCKET = 1, SERT_EGRAD_PATH_SORTED = 2 };
enum {
    SERT_EGRAD_FIXUP_WAVE = 1,       /* egrad_fixup<VEC>: one wave per entity */
    SERT_EGRAD_FIXUP_WORKGROUP = 2   /* egrad_fixup_wg<VEC>: one workgroup per entity (V_e < 256) */
};
int sert_debug_egrad_plan(sert_model* m, int32_t* out, int n);

/* The NCE score / loss / gradient kernel the LAST vectorspace forward of this model launched (vs_loss in
 * csrc/host/step_vectorspace.inc, kernels in csrc/kernels_vs.h; sert_train_batch, sert_eval_batch, ...) -- host record written
 * where the launch is made, test hook, no device is touched: out[0] one of SERT_NCE_FORM_*, out[1] the float4 chunks per lane NCH
 * (REGS, PER_CANDIDATE) or the columns per lane NPL (SCALAR), out[2] MAXC of vs_nce_regs<NCH, ., MAXC> (0 for the other forms;
 * 6 for z + 1 <= 6, 11 for z + 1 == 11 exactly, 12 for every other z + 1 <= 12),
 * out[3] 1 for the training instance and 0 for the evaluating one, out[4] workgroups of the launch, out[5] the per-workgroup loss
 * partials the kernel left for the loss reduction (0: the reduction starts from the row losses).  n <= 6; all zero before the
 * first forward and for a model that has no NCE loss.  tests/test_gpu_nce_forms.py asserts through this that every case of
 * tests/nce_cases.py reaches the template instance it is there for. */
enum {
    SERT_NCE_FORM_NONE = 0,
    SERT_NCE_FORM_REGS = 1,           /* vs_nce_regs<NCH, TRAIN, MAXC>: every candidate row of a batch row in registers */
    SERT_NCE_FORM_PER_CANDIDATE = 2,  /* vs_nce<NCH, TRAIN>: one candidate after the other */
    SERT_NCE_FORM_SCALAR = 3          /* vs_nce_scalar<NPL, TRAIN>: d_e % 4 != 0, one wave per row */
};
int sert_debug_nce_form(sert_model* m, int32_t* out, int n);

/* What the LAST step of a fold-in handle launched (include/sert_hip_foldin.h; kernels in csrc/kernels_foldin.h, dispatch in
 * csrc/host/api_foldin.inc: foldin_loss, foldin_grad; lazy_segsum.inc: EntityChain, shared with the model) -- host record written where the launches are made, test hook, no device is
 * touched: out[0] one of SERT_FOLDIN_LOSS_*, out[1] its template parameter (VECTOR: float4 chunks per lane; SCALAR: columns per
 * lane), out[2] 1 for the training instance and 0 for the evaluating one, out[3] key bits of the counting sort (the smallest b
 * with 2^b > num_new: the sentinel key is num_new itself), out[4] its digit passes, out[5] / out[6] VEC and NCH of
 * foldin_chunk_reduce<VEC, NCH>, out[7] its column passes, out[8] one of SERT_EGRAD_FIXUP_*, out[9] the tiles of 2048 keys of the
 * sort.  n <= 10; all zero before the first step.  An evaluation launches the loss kernel alone: it rewrites out[0..2] and leaves
 * out[3..9] as the last training step left them.  tests/test_gpu_foldin_keys.py asserts through this that every key structure of
 * tests/foldin_key_cases.py reaches the kernels it is there for. */
enum {
    SERT_FOLDIN_LOSS_NONE = 0,
    SERT_FOLDIN_LOSS_VECTOR = 1,   /* foldin_nce<K, TRAIN>: d_e % 4 == 0, sixteen lanes per instance */
    SERT_FOLDIN_LOSS_SCALAR = 2    /* foldin_nce_scalar<K, TRAIN>: any other d_e, one wave per instance */
};
int sert_debug_foldin_plan(sert_foldin* f, int32_t* out, int n);

/* How a fold-in handle addresses its trainable rows -- host record, test hook, no device is touched: out[0] 1 for the map form
 * (sert_foldin_create_refresh: foldin_nce_map* look every negative up in slot_of) and 0 for sert_foldin_create, out[1]
 * num_refresh, out[2] num_new, out[3] Nt = the rows of E.  n <= 4.  sert_debug_foldin_plan keeps its ten entries and their
 * meaning for a refresh handle (num_new there reads Nt). */
int sert_debug_foldin_table(sert_foldin* f, int32_t* out, int n);

/* What the LAST step of a word fold-in handle launched (include/sert_hip_wfold.h; kernels in csrc/kernels_wfold.h, dispatch in
 * csrc/host/api_wfold.inc: wfold_forward_loss, wfold_segsum, wfold_step_async) -- host record written where the launches are
 * made, test hook, no device is touched: out[0] one of SERT_WFOLD_PROJECT_* (the instance of wfold_project), out[1] the loss
 * kernel's form (SERT_NCE_FORM_PER_CANDIDATE: vs_nce<K, TRAIN>; SERT_NCE_FORM_SCALAR: vs_nce_scalar<K, TRAIN>), out[2] its K,
 * out[3] 1 for the training instance and 0 for the evaluating one, out[4] the levels of the batch's reduction (0: the batch
 * holds no new word), out[5 + l] the items of level l < 6, out[11] the reduction kernel (SERT_WGRAD_FORM_ROWS32 / _ROWS64 /
 * _SCALAR; 0 without a level), out[12] / out[13] the GEMM kernel chosen for P = Nv W and for G = S W^T (SERT_GEMM_ROUTE_*).
 * n <= 16; all zero before the first step.  An evaluation runs the forward alone: out[4..11] and out[13] are zero after it. */
enum {
    SERT_WFOLD_PROJECT_NONE = 0,
    SERT_WFOLD_PROJECT_VECTOR = 1,   /* wfold_project<4>: d_e % 4 == 0, float4 columns */
    SERT_WFOLD_PROJECT_SCALAR = 2    /* wfold_project<1>: any other d_e */
};
typedef struct sert_wfold sert_wfold;
int sert_debug_wfold_plan(sert_wfold* f, int32_t* out, int n);

/* Host only, no device is touched: the inverted index of a word fold-in (csrc/wfold_index.h: build_wfold_index) for batch
 * `batch` of tok (num_batches, B, n), the new word of every position or -1 -- levels[0] the levels, levels[1 + l] the items of
 * level l < 6, levels[7 + l] the first partial row of level l's output (13 ints); rows_out the entries (batch rows), items_out
 * the items {begin, end, dst, 0}, level after level; *num_rows / *num_items what the batch holds (nothing is copied when a
 * capacity is too small). */
int sert_debug_wfold_index(const int32_t* tok, int64_t num_batches, int B, int n, int num_words, int64_t batch, int32_t* levels,
                           int32_t* rows_out, int64_t rows_cap, int32_t* items_out, int64_t items_cap, int64_t* num_rows,
                           int64_t* num_items);

/* What the LAST step of a loglinear word fold-in handle launched (include/sert_hip_ll_wfold.h; kernels in
 * csrc/kernels_ll_wfold.h, dispatch in csrc/host/api_ll_wfold.inc: llw_forward, llw_segsum, llw_grad_gemm) -- host record
 * written where the launches are made, test hook, no device is touched: out[0] the row kernel's form (SERT_LL_WFOLD_FORM_*),
 * out[1] 1 when it reads and writes 16-byte pieces (V_e % 4 == 0), out[2] 1 for the training instance and 0 for the evaluating
 * one, out[3] the levels of the batch's reduction (0: the batch holds no new word), out[4 + l] the items of level l < 6, out[10]
 * the reduction kernel (SERT_WGRAD_FORM_ROWS64 / _SCALAR; 0 without a level), out[11] / out[12] the GEMM kernel chosen for
 * Zn = Nv W + b and for G = dZ W^T (SERT_GEMM_ROUTE_*), out[13] the k ranges of G (1: one launch, no combine), out[14] the
 * label kind of the upload the step ran on (SERT_LL_WFOLD_LABELS_*: llw_row or llw_row_csr).  n <= 16; all zero before the first
 * step.  An evaluation runs the forward alone: out[3..10], out[12] and out[13] are zero after it. */
enum {
    SERT_LL_WFOLD_LABELS_INT = 0,    /* sert_ll_wfold_upload: llw_row */
    SERT_LL_WFOLD_LABELS_ROWS = 1    /* sert_ll_wfold_upload_csr: llw_row_csr */
};
enum {
    SERT_LL_WFOLD_FORM_NONE = 0,
    SERT_LL_WFOLD_FORM_REG = 1,      /* llw_row<TRAIN, LLW_FORM_REG>: V_e <= 1024, J in four registers per thread */
    SERT_LL_WFOLD_FORM_STREAM = 2    /* llw_row<TRAIN, LLW_FORM_STREAM>: J through DJ, overwritten in place */
};
typedef struct sert_ll_wfold sert_ll_wfold;
int sert_debug_ll_wfold_plan(sert_ll_wfold* f, int32_t* out, int n);

/* The column layout of a loglinear fold-in handle (include/sert_hip_ll_foldin.h: sert_ll_foldin_create_refresh;
 * csrc/ll_label_remap.h) -- host record, test hook, no device is touched: *V_f the frozen columns the step kernels see as
 * V_e, *Nt the trainable ones they see as N (either may be NULL), internal_of_public[e] the internal column of public column e
 * -- the frozen columns in ascending trained index, the refreshed slots in the order of refresh_ids behind them, the new
 * columns last.  count must be V_e + num_new; for sert_ll_foldin_create the map is the identity.  Touches nothing else; fails
 * with a message on a null handle. */
int sert_debug_ll_foldin_layout(sert_ll_foldin* f, int32_t* V_f, int32_t* Nt, int32_t* internal_of_public, int64_t count);

/* What the LAST backward of this model launched for the per-word sums -- the word-table gradient of the vectorspace models
 * (word_grad_segsum) or dZu of the loglinear model (dzu_from_dj), both in csrc/host/lazy_segsum.inc over the tree of
 * csrc/word_index.h -- host record written where the launches are made, test hook, no device is touched:
 * out[0] one of SERT_WGRAD_PATH_*, out[1] levels of the batch's tree, out[2] tree launches made (levels 1 and 2 in one launch
 * count once), out[3] dense words of the batch, out[4] one of SERT_WGRAD_HEAVY_*, out[5] batch rows per workgroup of the dense
 * pass, out[6] its row blocks, out[7] 1 when the dense words' combine was launched alone, out[8] 1 when level 0 is sorted by
 * length with the first row in the descriptor; then per tree launch k < 6: out[10 + 2 k] one of SERT_WGRAD_FORM_*,
 * out[11 + 2 k] its gridDim.y.  n <= 24; all zero before the first backward.  tests/test_gpu_wgrad_cases.py asserts through this
 * that every count plan of tests/wgrad_cases.py reaches the kernels it is there for. */
enum { SERT_WGRAD_PATH_NONE = 0, SERT_WGRAD_PATH_WORD_GRAD = 1, SERT_WGRAD_PATH_DZU = 2 };
enum {
    SERT_WGRAD_HEAVY_NONE = 0,
    SERT_WGRAD_HEAVY_FUSED = 1,         /* extra workgroups of the tree's launches (segsum_rows_plus / segsum_rows_plus_ll) */
    SERT_WGRAD_HEAVY_TWO_LAUNCHES = 2,  /* segsum_heavy + segsum_heavy_combine in front of the tree */
    SERT_WGRAD_HEAVY_WIDE = 3           /* segsum_heavy_wide + segsum_heavy_combine_ll behind the tree */
};
enum {
    SERT_WGRAD_FORM_ROWS32 = 1,        /* segsum_rows<32> */
    SERT_WGRAD_FORM_ROWS64 = 2,        /* segsum_rows<64> (loglinear: <64, true, true[, true]>) */
    SERT_WGRAD_FORM_SCALAR = 3,        /* segsum_rows_scalar<false> / <true> */
    SERT_WGRAD_FORM_ROWS_PLUS = 4,     /* segsum_rows_plus */
    SERT_WGRAD_FORM_ROWS_PLUS_LL = 5,  /* segsum_rows_plus_ll */
    SERT_WGRAD_FORM_UPPER_FUSED = 6,   /* segsum_upper_fused */
    SERT_WGRAD_FORM_SCALAR_LL = 7,     /* segsum_rows_scalar<true, true> */
    SERT_WGRAD_FORM_BUNDLED = 8        /* segsum_rows_bundled (variants build) */
};
int sert_debug_wgrad_plan(sert_model* m, int32_t* out, int n);

/* The SCHEDULE of the vectorspace training step (csrc/step_plan.h): which queue the pieces of the backward and of the update
 * went to, in what order, and which events order them.  sert_debug_vs_plan: the plan of the step this model issued LAST, out[i]
 * by SERT_VS_PLAN_*, n <= SERT_VS_PLAN_COUNT -- host record, no device is touched; the default plan (everything on the main
 * queue) before the first step and for a loglinear model.  sert_debug_vs_facts: the facts that plan was decided from, out[i] by
 * SERT_VS_FACT_*, n <= SERT_VS_FACT_COUNT.  sert_debug_vs_plan_for: the same pure function on facts the caller
 * provides, facts[i] by SERT_VS_FACT_* (missing trailing facts take their defaults: no knob set) -- no model, no device; the
 * knob values are facts here, so the product library answers for a variants build's knobs too.
 * tests/test_step_plan_cpu.py pins the plan of every schedule, tests/test_gpu_step_plan.py that the steps ran it. */
enum {  /* facts: what the schedule depends on */
    SERT_VS_FACT_KIND = 0,          /* SERT_KIND_* */
    SERT_VS_FACT_HOST_AR, SERT_VS_FACT_COMM,   /* data parallel: host transport / communicator */
    SERT_VS_FACT_TIMING,            /* sert_timing_enable(m, 1) */
    SERT_VS_FACT_NSTREAMS,          /* SERT_STREAMS (default 2) */
    SERT_VS_FACT_N_RE,              /* elements of R_e, saturated at INT32_MAX */
    SERT_VS_FACT_BIG_RE, SERT_VS_FACT_BIG_W,   /* R_e / W of more than 2^22 elements (a streaming update of its own) */
    SERT_VS_FACT_KEEP_GRADS,
    SERT_VS_FACT_BATCH, SERT_VS_FACT_WORD_DIM, SERT_VS_FACT_ENTITY_DIM, SERT_VS_FACT_NUM_NEGATIVES,
    SERT_VS_FACT_HAS_ENTITIES,
    SERT_VS_FACT_SORT_FREE,         /* the sort-free entity chain (V_e <= 2048, d_e <= 128) */
    SERT_VS_FACT_CAND_EARLY,        /* the early sort's key buffer exists */
    SERT_VS_FACT_NEG_SIDE_READY,    /* this step's negatives were drawn during the previous step */
    SERT_VS_FACT_HAS_LABELS,
    SERT_VS_FACT_NEXT_NEG_DRAWN,    /* the next step's negatives exist already */
    SERT_VS_FACT_DH_STRIP, SERT_VS_FACT_BWD_FUSED_SHAPE,   /* variants build: shape predicates of gemm_strip / vs_bwd_fused */
    /* the knobs, by value (csrc/step_plan.h: VsKnobs has the defaults) */
    SERT_VS_FACT_K_EXT_EVENTS, SERT_VS_FACT_K_FORK_LATE,
    SERT_VS_FACT_K_FORK_AT,         /* SERT_FORK_AT: 0 unset, 1 nce, 2 nce_dw */
    SERT_VS_FACT_K_SIDE_HEAVY, SERT_VS_FACT_K_RE_DEFER,
    SERT_VS_FACT_K_EARLY_BUCKET,    /* -1 unset */
    SERT_VS_FACT_K_NO_EARLY_BUCKET, SERT_VS_FACT_K_EARLY_SORT, SERT_VS_FACT_K_NO_EARLY_SORT,
    SERT_VS_FACT_K_DW_FIRST,        /* -1 unset */
    SERT_VS_FACT_K_DP_LATE, SERT_VS_FACT_K_NO_TAIL, SERT_VS_FACT_K_EGRAD_GROUP_SUM, SERT_VS_FACT_K_BWD_FUSED,
    SERT_VS_FACT_COUNT
};
enum {  /* the plan */
    SERT_VS_PLAN_FORK_AT = 0,       /* SERT_VS_FORK_*: the kernel behind which the side queue starts its chain */
    SERT_VS_PLAN_FORK_CARRIED,      /* its own completion signal is the fork event */
    SERT_VS_PLAN_FORK_RECORDED,     /* a hipEventRecord behind the loss kernel is */
    SERT_VS_PLAN_DH_EVENT,          /* SERT_VS_EVENT_*: what the end of the dh GEMM marks */
    SERT_VS_PLAN_DH_CARRIED,        /* by its completion signal */
    SERT_VS_PLAN_ORDER,             /* four entries, SERT_VS_PIECE_*, in order of issue */
    SERT_VS_PLAN_ENTITY_QUEUE = SERT_VS_PLAN_ORDER + 4, SERT_VS_PLAN_DENSE_QUEUE,   /* SERT_VS_QUEUE_* */
    SERT_VS_PLAN_SIDE_MEETS_FORK,   /* the side queue waits for the fork in front of the pieces */
    SERT_VS_PLAN_ENTITY_WAITS_FORK, /* the entity chain's queue waits for it at its head */
    SERT_VS_PLAN_DENSE_EVENT,       /* SERT_VS_EVENT_*: what the dense gradients record behind themselves */
    SERT_VS_PLAN_BWD_FUSED,
    SERT_VS_PLAN_BUCKET_EARLY, SERT_VS_PLAN_SORT_EARLY, SERT_VS_PLAN_DRAW_NEXT_NEG,   /* on the side queue, in front of its fork wait */
    SERT_VS_PLAN_LAZY_JOIN,         /* the main queue never waits for the entity chain */
    SERT_VS_PLAN_END_JOIN,          /* it joins the side queue at the end of the backward */
    SERT_VS_PLAN_DP_LATE_JOIN,      /* the communication queue does */
    SERT_VS_PLAN_COMBINE_IN_TAIL, SERT_VS_PLAN_RE_IN_PARTS,
    SERT_VS_PLAN_SIDE_SMALL,        /* the small tensors are updated on the side queue */
    SERT_VS_PLAN_SMALL_ORDER,       /* SERT_VS_EVENT_*: what orders that queue in front of them */
    SERT_VS_PLAN_SPLIT_SMALL, SERT_VS_PLAN_DEFER_RE, SERT_VS_PLAN_DEFER_SMALL, SERT_VS_PLAN_RE_ON_SIDE,
    SERT_VS_PLAN_COUNT
};
enum { SERT_VS_FORK_NONE = 0, SERT_VS_FORK_LOSS = 1, SERT_VS_FORK_DH = 2 };
enum { SERT_VS_PIECE_ENTITY = 0, SERT_VS_PIECE_DH = 1, SERT_VS_PIECE_DENSE = 2, SERT_VS_PIECE_WORD_SUM = 3 };
enum { SERT_VS_QUEUE_MAIN = 0, SERT_VS_QUEUE_SIDE = 1, SERT_VS_QUEUE_THIRD = 2 };
enum { SERT_VS_EVENT_NONE = 0, SERT_VS_EVENT_FORK = 1, SERT_VS_EVENT_DENSE = 2, SERT_VS_EVENT_JOIN3 = 3, SERT_VS_EVENT_OPT_FORK = 4 };
int sert_debug_vs_plan(sert_model* m, int32_t* out, int n);
int sert_debug_vs_facts(sert_model* m, int32_t* out, int n);
int sert_debug_vs_plan_for(const int32_t* facts, int nfacts, int32_t* out, int n);

/* Which path the rows of a scorer's sert_scorer_topk calls took since sert_scorer_create -- host counters, test hook: out[0]
 * calls that took the fused path (sampled thresholds, filtering GEMM), out[1] those of them that filtered in bf16, out[2] the
 * query chunks of the fused calls, out[3] rows the fused path flagged and handed to the materialising path, out[4] rows of calls
 * that went to the materialising path directly, out[5] 1 while the table's bf16 prefilter is demoted to the fp32 filter.
 * n <= 6.  tests/test_gpu_score_contract.py asserts through this that its shapes reach the path they are there for. */
int sert_debug_scorer_counts(sert_scorer* s, int64_t* out, int n);

/* Test hook: the scorer's own selection kernels on cosines the caller provides, S (Q, V) f32 host -- values no dot product
 * of the library produces can be fed this way (every accumulator starts at +0, so a cosine of -0 never comes out of one).
 * mode 0: topk_rows<false> on S as the materialising path runs it.  mode 1: topk_from_groups on the per-(row, 64-entity
 * group) lists the fp32 filtering epilogue would leave for the threshold `thr` (elements with S >= thr, keyed by plain
 * desc_key, 16 slots per group, candidate capacity 1024); a row that kernel flags (fewer than k or more than 1024
 * candidates, an overflowed group) comes back with idx -1.  idx_out / score_out (Q, k): entity and (cos + 1)/2. */
int sert_debug_scorer_select(int device, int mode, const float* S, int64_t num_queries, int32_t V, int32_t k, float thr,
                             int32_t* idx_out, float* score_out);

/* Which path the rows of a scorer's sert_scorer_rank calls took since sert_scorer_create -- host counters, test hook: out[0]
 * calls, out[1] their query chunks (SERT_SCORE_RANK_BUDGET; at most 2048 queries and fewer than 2^31 elements per sorted
 * chunk), rows ranked by out[2] the top-k path (kk <= 1024), out[3] the LDS sort (V_e <= 8192), out[4] the counting-sort
 * passes, out[5] microseconds the copies of the results to the host took on the scorer's second stream, between events
 * recorded around them (LDS and counting-sort rows only: the top-k path copies inside sert_scorer_topk).  n <= 6. */
int sert_debug_scorer_rank_counts(sert_scorer* s, int64_t* out, int n);

/* Test hook: the ranking kernels of sert_scorer_rank on cosines the caller provides, S (Q, V) f32 host -- the only way to
 * feed them -0, NaNs of both signs and infinities.  The path goes by V alone: the LDS sort up to 8192, the counting-sort
 * passes above (Q <= 2048 and Q V < 2^31 there); the top-k kernels have sert_debug_scorer_select.  k = -1 or positive, ranked
 * depth kk as sert_scorer_rank.  idx_out / score_out (Q, kk): entity and (cos + 1)/2. */
int sert_debug_scorer_rank_select(int device, const float* S, int64_t num_queries, int32_t V, int32_t k, int32_t* idx_out,
                                  float* score_out);

/* What a scorer's sert_scorer_pairs and sert_scorer_rank_candidates calls did since sert_scorer_create -- host counters, test
 * hook: out[0] calls of the two that passed their argument checks, out[1] their chunks (SERT_SCORE_RANK_BUDGET), queries
 * ranked by out[2] the LDS kernel (1 .. 8192 candidates), out[3] the slab and the counting-sort passes (more), out[4] pairs
 * scored (a pair of sert_scorer_rank_candidates is scored once, whichever kernel ranks it), out[5] empty lists. */
int sert_debug_scorer_rerank_counts(sert_scorer* s, int64_t out[6]);

/* Test hook: overwrite the step's gradient scratch -- the flat buffer [g_Rw | g_Re | g_W | g_b | loss, sum of squares] with
 * quiet NaNs, the per-entity sorted-run bounds behind it with the wrong run [0, 1) -- after waiting for the device.  A step
 * whose negatives were drawn ahead launches NO prologue (nothing is zeroed): it relies on every value it reads having been
 * written by this step's own kernels.  A run with this call between the steps must equal the run without it bit for bit
 * (tests/test_gpu_parity.py::test_steps_read_nothing_stale_from_the_gradient_scratch).  Fails while a run-ahead step
 * (sert_hint_next_batch) is in flight: its gradients live there. */
int sert_debug_poison_scratch(sert_model* m);

/* Host-only (no device is touched): the row-exchange lists rank `rank` of `world` derives for batch
 * `batch` from the touched-row bitmaps of ALL ranks, allbits[world][num_batches][bit_words] -- the
 * function sert_upload_dataset runs on the gathered bitmaps (csrc/kernels_xchg.h).  Lets the
 * multi-rank algebra of the exchange be checked without any GPU: serve_cnt / fetch_cnt [world];
 * serve_rows / fetch_rows peer-major; union_rows with their contributions ptr / ent in rank order
 * (ent < 0: this rank's own row); sizes[5] = {serve, fetch, union, entries, largest transfer in rows}.
 * Every output array must hold `capacity` entries. */
int sert_debug_row_lists(const uint32_t* allbits, int world, int rank, int64_t num_batches, int64_t bit_words,
                         int64_t rows_per_rank, int64_t vocab, int64_t batch, int32_t* serve_cnt,
                         int32_t* fetch_cnt, int32_t* serve_rows, int32_t* fetch_rows, int32_t* union_rows,
                         int32_t* ptr, int32_t* ent, int64_t capacity, int64_t* sizes);

/* Host only, no GPU (test hook, no reference counterpart): the inverted index word -> batch rows that
 * sert_upload_dataset builds for a vectorspace model (the order-fixed replacement of Theano's AdvancedIncSubtensor1,
 * autodiff of sert/models.py:180), built for ids[num_batches][B][n] and EVALUATED ON THE HOST the way the segmented-sum
 * kernels walk it: grad_out[vocab][d] = the word-table gradient of batch `batch` for source rows src[B][d] (dh), i.e.
 * sum over the occurrences of a word of src[row] / divisor.  row_groups > 1: level 0 cut into row ranges (XCD lists);
 * dense_heavy: bit 0 = the batch's heaviest words summed outside the tree, bit 1 = level 0 sorted by item length with every
 * item's first row number in its descriptor (what the vectorspace models upload).  stats[11] = {levels, items, partial rows, final items,
 * dense words, row groups, level-0 items, distinct words, fused_upper_ok (levels 1 and 2 may run as one launch), heavy_cnt (words
 * whose level-1 chunks are summed again at level 2 of a three-level tree), level-1 items}. */
int sert_debug_word_index_sum(const void* ids, int id_bytes, int64_t num_batches, int B, int n, int vocab, int row_groups,
                              int dense_heavy, int64_t batch, const float* src, int d, float divisor, float* grad_out,
                              int64_t* stats);

/* Test hook: the aggregate and ranking kernels of sert_ll_rank_queries on per-token distributions the caller provides,
 * P (offsets[Q], V) f32 host, rows in query order; same outputs as sert_ll_rank_queries.  Pins the device ranking to the
 * reference's recorded LogLinearCallback outputs (tests/test_gpu_ll_rank.py). */
int sert_debug_ll_rank_distributions(int device, const float* P, const int64_t* offsets, int64_t num_queries, int32_t V,
                                     int32_t k, int32_t* idx_out, float* score_out, float* joint_entropy_out,
                                     float* token_entropy_out, int32_t* status_out);

/* Test hook: sert_debug_ll_rank_distributions plus the candidate CSR and the ragged outputs of sert_ll_rank_candidates -- the
 * aggregate and the candidate-ranking kernels (csrc/kernels_ll_rerank.h) on per-token distributions the caller provides, all
 * queries as one chunk. */
int sert_debug_ll_rank_candidates_distributions(int device, const float* P, const int64_t* offsets, int64_t num_queries,
                                                int32_t V, const int64_t* cand_indptr, const int32_t* cand_entities, int32_t k,
                                                int32_t* idx_out, float* score_out, float* joint_entropy_out,
                                                float* token_entropy_out, int32_t* status_out);

/* What the sert_ll_rank_candidates and sert_debug_ll_rank_candidates_distributions calls of this PROCESS did -- host counters,
 * test hook: out[0] calls that passed their argument checks, out[1] their chunks (SERT_LL_RANK_BUDGET), lists ranked by out[2]
 * the LDS kernel (1 .. 8192 candidates), out[3] the slab and the counting-sort passes (more), out[4] empty lists.  One
 * process-wide set for both calls (the debug call has no model to keep them in): compare two readings. */
int sert_debug_ll_rerank_counts(int64_t out[5]);

/* Micro-benchmark of the fp32 MFMA GEMM on device-resident random operands:
 * C (M,N) = op(A).op(B); ta/tb as in gemm.h; epi 0 = store, 1 = +bias, 2 = tanh(+bias);
 * splits > 1 = split-K partial slabs.  Returns the average launch time in *avg_us
 * (HIP events, `iters` launches after 2 warm-ups). */
int sert_bench_gemm(int device, int ta, int tb, int epi, int M, int N, int K, int splits,
                    int iters, double* avg_us);

/* The same dispatch on HOST arrays (test hook, no reference counterpart): C (M,N) = epi(op(A).op(B)), A (M,K) or
 * (K,M) if ta, B (K,N) or (N,K) if tb, bias (N) for epi 1 / 2 (only with ta = 0).  The shape is routed to the kernel a
 * training step would use for it, so every GEMM kernel of the library can be pinned against float64. */
int sert_debug_gemm(int device, int ta, int tb, int epi, int M, int N, int K, const float* A, const float* B,
                    const float* bias, float* C);

/* The split-K form of the same dispatch (test hook): out (M*N + N) = A^T.B, A (K,M), B (K,N) host arrays, followed by
 * the N column sums of B -- the split-K launch with the column sums riding along + the order-fixed combine that the
 * projection's dW / db take in a training step (sert/models.py:1057-1061, autodiff). */
int sert_debug_gemm_splitk(int device, int M, int N, int K, int splits, const float* A, const float* B, float* out);

/* ... and of a product A.op(B) over a long K cut into `splits` k ranges (test hook): C (M,N), A (M,K), B (K,N) or (N,K) if tb,
 * through the split launch + order-fixed combine of the loglinear dG = dZ.W^T over a large entity vocabulary
 * (sert/models.py:846-849, autodiff). */
int sert_debug_gemm_longk(int device, int tb, int M, int N, int K, int splits, const float* A, const float* B, float* C);

/* Host only, no device is touched (test hook): the kernel the three hooks above would launch for a shape -- `form` one of
 * SERT_GEMM_FORM_*, ta / tb as sert_debug_gemm takes them (SPLITK is A^T.B, LONGK A.op(B)), `splits` as the split forms take
 * it (ignored for PLAIN), `align` the byte alignment of both operands (16 or more: device allocations; 4: an operand that
 * starts anywhere).  Asked of the predicates the launchers themselves ask (gemm.h, gemm_x3.h), under the process's
 * SERT_GEMM_FP32.  Returns a SERT_GEMM_ROUTE_* code; < 0 on a bad argument.  tests/test_x3_split_cpu.py asserts through it
 * that the shapes of the exact-product tests reach every kernel form of the product build. */
enum { SERT_GEMM_FORM_PLAIN = 0, SERT_GEMM_FORM_SPLITK = 1, SERT_GEMM_FORM_LONGK = 2 };
enum {
    SERT_GEMM_ROUTE_F32_TILE64 = 1,      /* gemm.h: 64 x 64 tiles */
    SERT_GEMM_ROUTE_F32_TILE128 = 2,     /*         128 x 128 tiles, persistent */
    SERT_GEMM_ROUTE_F32_TILE128X160 = 3, /*         128 x 160 tiles */
    SERT_GEMM_ROUTE_X3_128_VEC = 4,      /* gemm_x3.h: 128 x 128 tiles, 16-byte loaders */
    SERT_GEMM_ROUTE_X3_128_SCALAR = 5,   /*            128 x 128 tiles, dword loaders (any alignment) */
    SERT_GEMM_ROUTE_X3_256 = 6,          /*            256 x 256 tiles */
    SERT_GEMM_ROUTE_X3_320 = 7,          /*            256 x 320 tiles */
    SERT_GEMM_ROUTE_X3_TA_SINGLE = 8,    /*            A^T.B, one 128 x 128 tile per k range */
    SERT_GEMM_ROUTE_X3_TA_320X160 = 9,   /*            A^T.B, 320 x 160 tiles of ten waves */
    SERT_GEMM_ROUTE_X3_TA_TILES = 10     /*            A^T.B, 128 x 128 tiles over M and N */
};
int sert_debug_gemm_route(int form, int ta, int tb, int M, int N, int K, int splits, int align);

/* Memory-system micro-benchmarks: the denominators a step's memory-bound kernels are priced
 * against (no reference counterpart; measurement only).  Average launch time over `iters`
 * launches (HIP events on the launching stream, 2 warm-ups) in *avg_us.
 *   SERT_MEMBENCH_COPY       float4 stream copy: `bytes` read + `bytes` written per launch
 *   SERT_MEMBENCH_READ       float4 stream read of `bytes`
 *   SERT_MEMBENCH_GATHER     the step's own window gather (vs_gather_mean) over uniformly random
 *                            rows: `bytes` of output rows of `row_bytes`, each the mean of `window`
 *                            rows of a table of `table_bytes` -> bytes * window fetched per launch
 *   SERT_MEMBENCH_OPTIMIZER  the dense Adam kernel over four arrays of `bytes` (4 read, 3 written),
 *                            placed `gap_bytes` apart inside one allocation ((size_t)-1: four
 *                            allocations of their own, as a model holds them)
 * blocks: workgroups of the launch (0 = the kernel's default). */
enum { SERT_MEMBENCH_COPY = 0, SERT_MEMBENCH_READ = 1, SERT_MEMBENCH_GATHER = 2, SERT_MEMBENCH_OPTIMIZER = 3 };
int sert_bench_memory(int device, int kind, size_t bytes, size_t table_bytes, int row_bytes,
                      int window, size_t gap_bytes, int blocks, int iters, double* avg_us);

/* Test hook: the number of chunks a sert_reval handle (sert_hip.h) ranks its topics in -- 1 for the vectorspace kinds, for
 * loglinear what SERT_LL_RANK_BUDGET gave when the handle was created; < 0 on error. */
struct sert_reval;
int sert_debug_reval_chunks(struct sert_reval* r);

/* Test hook: the counting kernel of the counted evaluator (sert_hip_reval_counted.h; csrc/kernels_reval.h: reval_count_ranks)
 * alone, on cosines the caller provides, cos (Q, V) f32 host -- the only way to feed it -0, NaNs of both signs and
 * infinities.  rel_indptr (Q + 1) / rel_ent: per row the judged entities, each in [0, V), any order; ranks_out
 * (rel_indptr[Q]) int32: 1 + the number of entities that precede the judged one under the scorer's order.  Q <= 65535,
 * Q V <= 2^31.  The tile (8 or 32 judged entities in registers) goes by the longest list, the row form by V % 4. */
int sert_debug_count_ranks(int device, const float* cos, int64_t Q, int64_t V, const int64_t* rel_indptr, const int32_t* rel_ent,
                           int32_t* ranks_out);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_DEBUG_H */
