/*
 * sert_hip.h -- C ABI of libsert_hip.so, the MI355X (gfx950) execution engine
 * behind the sert.models / sert.inference Python surface.
 *
 * The reference (cvangysel/SERT) has no FFI: its hot path is the body of four
 * compiled Theano functions created in sert/models.py:530-608 (train_fn,
 * test_fn, validate_fn, predict_fn).  Each entry point below replaces one of
 * those functions or one Theano primitive they rely on; the file:line it
 * replaces is cited next to it.  The Python host (sert_amd/models.py) binds
 * these with ctypes; INTEGRATION.md shows the stub a SERT maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from sert_last_error() (thread-local, valid until the next call)
 *   - plain pointers and sizes only; host pointers are borrowed for the
 *     duration of the call; device memory is owned by the sert_model handle
 *   - one handle = one model replica on one HIP device with one HIP stream;
 *     a handle is not thread-safe
 *   - all floating point data is IEEE fp32 (floatX=float32, product-search.sh:95)
 */
#ifndef SERT_HIP_H
#define SERT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sert_model sert_model;

/* model kind: bin/train.py:21-24 */
enum {
    SERT_KIND_LOGLINEAR = 0,   /* sert.models.LanguageModel            (models.py:804) */
    SERT_KIND_VECTORSPACE = 1, /* sert.models.VectorSpaceLanguageModel (models.py:1024) */
    /* ADDITIVE, not in the reference (BASELINE.json configs[1] wording
     * "embed gather + MFMA projection + full softmax"): the vectorspace encoder
     * (gather, mean-pool, tanh projection) scored against ALL entities,
     * logits = clip(t).R_e^T, clipped softmax cross-entropy, dense L2, Adam. */
    SERT_KIND_VECTORSPACE_SOFTMAX = 2
};

/* data split: ModelBase.TRAIN / VALIDATE givens (models.py:482-522) */
enum { SERT_SPLIT_TRAIN = 0, SERT_SPLIT_VALIDATE = 1 };

/* tensors addressable through sert_get_tensor / sert_set_tensor */
enum {
    SERT_T_RW = 0,      /* word representations   (V_w, d_w)  models.py:167-171 */
    SERT_T_RE = 1,      /* entity representations (V_e, d_e)  models.py:940     */
    SERT_T_W = 2,       /* dense weights: VS (d_w, d_e) models.py:1057; LL (d_w, V_e) :846 */
    SERT_T_B = 3,       /* dense bias:    VS (d_e);  LL (V_e)                    */
    /* optimiser state, same shapes: Adam m / Adadelta accu  = STATE0,
     *                               Adam v / Adadelta delta = STATE1 */
    SERT_T_STATE0_RW = 4, SERT_T_STATE0_RE = 5, SERT_T_STATE0_W = 6, SERT_T_STATE0_B = 7,
    SERT_T_STATE1_RW = 8, SERT_T_STATE1_RE = 9, SERT_T_STATE1_W = 10, SERT_T_STATE1_B = 11,
    /* last-step gradients (data term + L2 term) and activations: readable only from a
     * model created with cfg.keep_grads (sert_get_tensor fails otherwise: without it these
     * buffers are scratch) */
    SERT_T_GRAD_RW = 12, SERT_T_GRAD_RE = 13, SERT_T_GRAD_W = 14, SERT_T_GRAD_B = 15,
    /* last-step activations (debug / parity): */
    SERT_T_ACT_H = 16,   /* VS mean-pooled window (B, d_w)      models.py:226  */
    SERT_T_ACT_T = 17,   /* VS tanh(hW+b)         (B, d_e)      models.py:1057 */
    SERT_T_ACT_DA = 18,  /* VS dL/d(hW+b)         (B, d_e)                     */
    SERT_T_ACT_DH = 19,  /* VS dL/dh              (B, d_w)                     */
    SERT_T_ACT_ROWLOSS = 20 /* per-instance loss  (B,)          models.py:1098, :292 */
};

typedef struct sert_config {
    uint32_t struct_size;     /* = sizeof(sert_config), checked */
    int32_t kind;             /* SERT_KIND_* */
    int32_t batch_size;       /* rows this replica processes per step (B_local) */
    int32_t global_batch_size;/* B of the model: divisor of the loss mean and of the
                                 L2 term lambda/(2B) (models.py:281-282, :773-791).
                                 == batch_size unless data-parallel */
    int32_t window_size;      /* n,   models.py:697 */
    int32_t vocab_size;       /* V_w, models.py:701 */
    int32_t num_entities;     /* V_e, models.py:924 / output_layer_size :809 */
    int32_t word_dim;         /* d_w, models.py:702 */
    int32_t entity_dim;       /* d_e, models.py:925 (vectorspace only) */
    int32_t num_negatives;    /* z,   models.py:961 (vectorspace only) */
    int32_t id_bytes;         /* width of token ids in x: 1, 2 or 4
                                 (np.min_scalar_type, bin/prepare.py:380) */
    int32_t device;           /* HIP device ordinal */
    int32_t keep_grads;       /* keep SERT_T_GRAD_* readable after a step (debug) */
    int32_t deterministic;    /* 1: order-fixed reductions everywhere */
    int32_t inference_only;   /* 1: parameters only (no optimiser state, gradients or
                                 activations); only sert_predict_* and tensor I/O work */
    float lambda_;            /* regularization_lambda, models.py:704 */
    /* optimiser hyper-parameters.  vectorspace: Adam (models.py:922)
     * lr, beta1, beta2, eps.  loglinear: Adadelta (models.py:820) lr, rho(beta1), eps. */
    float lr, beta1, beta2, eps;
    uint64_t seed;            /* device negative sampler (replaces RandomStreams
                                 seeding, models.py:958-959) */
} sert_config;

/* ---- lifetime ----------------------------------------------------------- */

/* Replaces model construction + theano.function compilation
 * (models.py:422-480, :530-608). Allocates parameters (zero), optimiser state,
 * gradient and activation buffers on cfg->device. */
int sert_create(const sert_config* cfg, sert_model** out);
int sert_destroy(sert_model* m);

const char* sert_last_error(void);

/* Human-readable device description ("gfx950 ... 256 CUs ..."); returns the
 * number of bytes written (excluding NUL) or <0 on error. */
int sert_device_info(int device, char* buf, size_t buflen);
/* Number of visible HIP devices, <0 on error. */
int sert_device_count(void);

/* ---- parameters and state ---------------------------------------------- */

/* theano.shared(...).set_value / get_value (models.py:183, :328-330, :945).
 * `count` must equal the tensor's element count. */
int sert_set_tensor(sert_model* m, int which, const float* host, size_t count);
int sert_get_tensor(sert_model* m, int which, float* host, size_t count);
/* element count of a tensor (0 if not present for this model kind) */
size_t sert_tensor_size(sert_model* m, int which);

/* Adam's shared step counter t (Lasagne adam t_prev); resume support. */
int sert_set_step(sert_model* m, int64_t t);
int64_t sert_get_step(sert_model* m);

/* Position of the EVALUATION negative stream (the reference keeps a second RandomStreams for
 * the evaluation loss, models.py:751 -> :1074; here: the odd Philox stream, advanced once per
 * evaluated batch).  With sert_set_step -- the training stream's position is the optimiser
 * step -- a resumed run draws what the uninterrupted run would have drawn. */
int sert_set_eval_draws(sert_model* m, int64_t n);
int64_t sert_get_eval_draws(sert_model* m);

/* The (B, z) negatives the device sampler draws for the training step taken when `position` optimiser updates have been
 * applied (evaluation = 0; position = sert_get_step before the step), or for the `position`-th evaluated batch
 * (evaluation = 1) -- what RandomStreams.choice (models.py:970-973) hands the reference's graph.  out (B, z) int64.  A pure
 * function of (seed, position, rank): no state of the model changes, so a caller can replay a device-sampled run with
 * explicit negatives (sert_train_batch's `negatives`) or feed the same ids to a CPU implementation. */
int sert_negatives_of_step(sert_model* m, int64_t position, int evaluation, int64_t* out);

/* ---- data set ---------------------------------------------------------- */

/* Replaces theano.shared(x/y/w) of the whole data set (models.py:470-480):
 * one H2D upload, batches are then slices [i*B, (i+1)*B) (models.py:322-326).
 *   x        (N, n) token ids, id_bytes wide, row-major
 *   y_int    (N,) int32 labels, or NULL when the labels are CSR
 *   csr_*    CSR label matrix (N, V_e) f32 (loglinear without --one_hot_classes,
 *            models.py:66-89 densifies it per batch); NULL when y_int given.
 *            The contract: csr_indptr (N + 1) starts at 0 and does not decrease; the columns of a row
 *            (csr_indices) lie in [0, V_e) and are STRICTLY INCREASING -- canonical CSR, no duplicate
 *            column, as scipy's sum_duplicates() leaves it; anything else is refused here (the loss
 *            kernels add a row's label entries to its gradient from different threads, so two entries
 *            of one column would race).  A row may hold any number of labels from none (loss 0, no
 *            gradient) to V_e; the values (csr_data) are arbitrary finite floats -- a stored 0, rows
 *            that do not sum to 1.
 *   w        (N,) f32 instance weights, NULL = all ones (train split only)
 * In data-parallel mode every rank uploads the rows it owns of every global
 * batch (see sert_amd/distributed.py). */
int sert_upload_dataset(sert_model* m, int split, const void* x, const int32_t* y_int,
                        const int64_t* csr_indptr, const int32_t* csr_indices,
                        const float* csr_data, const float* w, int64_t num_instances);

/* ---- the hot path ------------------------------------------------------- */

/* train_fn(batch_index) (models.py:581-588): forward, backward, L2, optimiser
 * update on rows [batch_index*B, (batch_index+1)*B) of the train split.
 * *loss_out receives the training loss evaluated BEFORE the update.
 *   negatives  (B, z) int64 entity ids (vectorspace; models.py:970-973) or NULL
 *              to let the device sampler draw them (iid uniform, with
 *              replacement, keyed by (seed, step, global row, j)).
 * With a communicator attached (sert_comm_init) the gradients are summed over
 * ranks before the (replicated) update, and *loss_out is the global loss. */
int sert_train_batch(sert_model* m, int64_t batch_index, const int64_t* negatives,
                     float* loss_out);

/* Additive.  Announces the batch the call AFTER the next sert_train_batch will train.
 * The next sert_train_batch then lets that batch run ahead of the host: behind its own
 * step, and BEFORE it waits for its own loss, it enqueues the announced batch's forward
 * and backward (single GPU, device-drawn negatives; data parallel: the parameter-only
 * forward projection) -- everything that depends on parameters, data and the step
 * counter only and writes activations and gradient scratch only -- so the device does not
 * idle through the host round trip of the reference's per-batch loop
 * (sert/models.py:369-379: train_fn, isfinite check, next train_fn).  The announced step's
 * UPDATE (optimiser, loss) is never issued ahead: a step that raises on a non-finite loss
 * leaves the model exactly as without the hint.  A following call that does not match
 * (another batch, explicit negatives, an evaluation, new parameters or data) simply
 * recomputes.  next_batch_index < 0 clears the hint. */
int sert_hint_next_batch(sert_model* m, int64_t next_batch_index);

/* Same, for `count` batches back to back with no host synchronisation in
 * between (device sampler only).  losses_out[count]. */
int sert_train_batches(sert_model* m, const int64_t* batch_indices, int64_t count,
                       float* losses_out);

/* test_fn / validate_fn (models.py:593-608): unweighted, unregularised mean
 * loss of one batch of `split`; no parameter change. */
int sert_eval_batch(sert_model* m, int split, int64_t batch_index,
                    const int64_t* negatives, float* loss_out);

/* The same for `count` batches with ONE host synchronisation (device-drawn negatives): the
 * error passes of bin/train.py (train_error / validation_error, models.py:649-668, run before
 * training and after every epoch, train.py:262-348) are loops over all batches whose results
 * are only averaged.  losses_out[i] = the value sert_eval_batch would return for
 * batch_indices[i], in order; a non-finite value is reported by the caller after the call. */
int sert_eval_batches(sert_model* m, int split, const int64_t* batch_indices, int64_t count,
                      float* losses_out);

/* vectorspace predict_fn (models.py:1107-1118), batched over Q queries:
 * out[q] = tanh(avg[q] . W + b)   (no clip).  avg (Q, d_w), out (Q, d_e). */
int sert_predict_project(sert_model* m, const float* avg, int64_t num_queries, float* out);

/* loglinear predict_fn (models.py:880-890): ids (rows, n) -> per-token
 * distributions out (rows, n, V_e).  rows need not equal batch_size. */
int sert_predict_tokens(sert_model* m, const void* ids, int64_t rows, float* out);

/* ---- loglinear query ranking (bin/query.py:199-236, batched) ----------- */

/* Per-query status of sert_ll_rank_queries */
enum {
    SERT_LL_STATUS_DEVICE = 0, /* ranked on the device */
    SERT_LL_STATUS_HOST = 1    /* the joint's sum S is 0 or not finite: the reference's `joint /= joint.sum()` gives NaN
                                  and logs the non-normalised-mass error (query.py:213-219); the caller runs the query
                                  through the per-token host path (sert_predict_tokens + LogLinearCallback.process).
                                  Its idx / score rows and joint entropy are not meaningful. */
};

/* WordBatcher -> predict_fn -> LogLinearCallback.process for Q queries at once (sert/inference.py:28-143, :170-174;
 * bin/query.py:199-236): the per-token entity distributions are computed once per distinct token and never leave the
 * device.  For every query q with tokens[offsets[q] .. offsets[q+1]) (ids < vocab_size, at least one per query):
 *   L_e = sum_t (p_te > 0 ? log p_te : 0) in token order, j_e = exp(L_e), score_e = j_e / sum_e j_e
 *     (inference.py:174 product with log 0 -> 0, query.py:213-214 renormalisation)
 *   idx_out (Q, kk) int32 / score_out (Q, kk) f32: the kk best entities, score descending, entity index ascending
 *     (query.py:231 argsort reversed, ties in a fixed order); kk = V_e for k = -1 (every entity, as the reference ranks)
 *     or k >= V_e, else k
 *   joint_entropy_out (Q) f32: normalised base-2 entropy of the joint (query.py:222-226 _debug line)
 *   token_entropy_out (offsets[Q]) f32: normalised base-2 entropy of every token's distribution (query.py:209)
 *   status_out (Q) int32: SERT_LL_STATUS_*
 * A query's results do not depend on the other queries of the call or on how the call is cut into chunks
 * (SERT_LL_RANK_BUDGET: device bytes per chunk, default 2 GiB).  Same preconditions as sert_predict_tokens; like it,
 * COLLECTIVE in data parallel (the word table is first all-gathered). */
int sert_ll_rank_queries(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_queries, int32_t k,
                         int32_t* idx_out, float* score_out, float* joint_entropy_out, float* token_entropy_out,
                         int32_t* status_out);

/* Re-ranking with the loglinear model: sert_ll_rank_queries restricted to per-query candidate lists.  tokens / offsets,
 * joint_entropy_out, token_entropy_out and status_out are exactly those of sert_ll_rank_queries (the entropies are over ALL
 * entities).  cand_indptr (Q + 1) / cand_entities: the CSR of sert_scorer_rank_candidates -- cand_indptr starts at 0 and never
 * decreases, a list may be empty, entities lie in [0, V_e) and are STRICTLY ASCENDING inside a list.  k = -1 ranks the whole
 * list, k >= 1 its best kk_q = min(k, length); query q writes at out_ptr[q] = sum_{p < q} kk_p of idx_out / score_out (the
 * ragged layout of sert_scorer_rank_candidates).
 *   For a query with status DEVICE the result is sert_ll_rank_queries(k = -1)'s ranking of that query restricted to its list,
 *   cut to its head: the same entities in the same order (score descending, ties by lowest entity index) and the same score
 *   BITS -- the scores stay normalised over all entities, the partition function is not restricted.  A query with status HOST
 *   has a zeroed joint row: its list comes back in entity order with score 0, not meaningful; the caller takes the host path.
 * A query's result does not depend on the other queries of the call, on their lists, or on how the call is cut into chunks
 * (SERT_LL_RANK_BUDGET; a chunk holds joint rows but neither a V_e-wide sort scratch nor V_e-wide outputs, so far more queries
 * than one of sert_ll_rank_queries).  Every argument fault -- a null pointer, cand_indptr[0] != 0, a decreasing cand_indptr, an
 * entity out of range, an unsorted or duplicated list, k == 0 or k < -1, a vectorspace model, a bad token or offset -- returns
 * before anything is launched; a failed call leaves nothing queued.  COLLECTIVE in data parallel, as sert_ll_rank_queries. */
int sert_ll_rank_candidates(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_queries,
                            const int64_t* cand_indptr, const int32_t* cand_entities, int32_t k,
                            int32_t* idx_out, float* score_out, float* joint_entropy_out,
                            float* token_entropy_out, int32_t* status_out);

/* ---- retrieval evaluation on the live model (product-search.sh:136-170, W3C-expert-finding.sh:108-124) ---- */

typedef struct sert_reval sert_reval;

/* columns of sert_reval_run's metrics_out */
enum {
    SERT_REVAL_NDCG = 0,        /* NDCG at the ranked depth (trec_eval ndcg_cut_K; ndcg when every entity is ranked) */
    SERT_REVAL_MAP = 1,         /* average precision over the ranked depth */
    SERT_REVAL_RECIP_RANK = 2,
    SERT_REVAL_P5 = 3,
    SERT_REVAL_NUM_REL_RET = 4, /* relevant entities among the ranked ones */
    SERT_REVAL_NUM_METRICS = 5
};

/* Replaces, for a model that is being trained, the reference's way to one retrieval figure per epoch: dump the model, start
 * bin/query.py on it, run trec_eval on the run file (product-search.sh:136-170).  Topics and relevance judgements are uploaded
 * ONCE, to the model's device; the handle borrows `m`, which must outlive it.
 *   tokens / offsets   the topics as a ragged int32 array, as for sert_ll_rank_queries: topic q owns
 *                      tokens[offsets[q] .. offsets[q+1]) (ids < vocab_size, at least one per topic)
 *   rel_indptr (Q+1) / rel_entities / rel_gains   the judgements as CSR per topic: entity indices < num_entities, strictly
 *                      ascending inside a topic, gains f32; an entity counts as relevant when its gain is > 0
 *   ideal_dcg (Q) f64  the topic's ideal DCG at the ranked depth, num_rel (Q) its number of relevant entities: computed by
 *                      the caller in float64 over ALL judgements of the topic, those of entities the model does not know included
 *   k                  entities ranked per topic.  loglinear: -1 = every entity (as the reference ranks), or positive.
 *                      vectorspace kinds: 1 .. min(num_entities, 1024), the range of sert_scorer_topk; other values are refused
 *                      (any depth: the counted evaluator, sert_hip_reval_counted.h).
 * The ranked depth kk is num_entities for k = -1 or k >= num_entities, else k. */
int sert_reval_create(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_topics,
                      const int64_t* rel_indptr, const int32_t* rel_entities, const float* rel_gains,
                      const double* ideal_dcg, const int32_t* num_rel, int32_t k, sert_reval** out);

/* Rank every topic with the parameters AS THEY ARE on the device now and compute the per-topic metrics there; only the results
 * cross to the host.  The parameters are first brought up to date as for sert_get_tensor (lazily updated word rows, deferred
 * entity and dense updates); a batch announced with sert_hint_next_batch stays announced.  No parameter, optimiser state or
 * sampler position changes: training continues as if the call had not happened.
 *   vectorspace kinds: mean of the topic's word rows (fp32, token order, one division: bit for bit numpy's mean of the rows) ->
 *     sert_predict_project's GEMM -> the kernels of sert_scorer_topk against the live entity table.  The ranking is the one
 *     sert_get_tensor -> mean -> sert_predict_project -> sert_scorer_create -> sert_scorer_topk gives on the same parameters.
 *   loglinear: the chunks and kernels of sert_ll_rank_queries.
 *   metrics_out (Q, SERT_REVAL_NUM_METRICS) f64, accumulated in float64 on the device in a fixed order.  Ties in the score
 *     are ranked by lowest entity index (trec_eval re-sorts a run file's ties by entity id descending; the ranking evaluated
 *     here is the device's).
 *   status_out (Q) int32: SERT_LL_STATUS_*; a loglinear topic reported SERT_LL_STATUS_HOST has no meaningful metrics or
 *     ranking, the caller evaluates it through the per-token host path.  Always DEVICE for the vectorspace kinds.
 *   idx_out (Q, kk) int32 / score_out (Q, kk) f32: the ranking itself, or both NULL.
 * Like sert_ll_rank_queries, COLLECTIVE in data parallel (the word table is first all-gathered): every rank calls it, in the
 * same order (collective; tested at world size 1 only). */
int sert_reval_run(sert_reval* r, double* metrics_out, int32_t* status_out, int32_t* idx_out, float* score_out);
int sert_reval_destroy(sert_reval* r);

/* Evaluation at any depth for the vectorspace kinds -- k = -1, k above 1024 -- by counting the judged entities' ranks instead
 * of ranking: the counted evaluator's create call and the call that returns the ranks of its last run are declared in
 * sert_hip_reval_counted.h, which is part of this boundary. */
#include "sert_hip_reval_counted.h"

/* ---- entity scoring (bin/query.py:239-370, batched) --------------------- */

typedef struct sert_scorer sert_scorer;

/* VectorSpaceCallback.__init__ (query.py:241-302): take the entity table
 * (V_e, d) f32 (host, un-normalised; not modified), L2-normalise a device copy
 * (query.py:270-274).  Replaces NearestNeighbors.fit (query.py:288-293). */
int sert_scorer_create(int device, const float* entities, int64_t num_entities, int32_t dim,
                       sert_scorer** out);
int sert_scorer_destroy(sert_scorer* s);

/* VectorSpaceCallback.process (query.py:320-367) for Q queries at once: L2-normalise
 * each projection (query.py:333-336), score every entity with (cos + 1)/2
 * (query.py:352-357) and return the k best per query, sorted by score
 * descending, ties by lowest entity index (replaces kneighbors / cdist+argsort,
 * query.py:304-318, and the Python candidate loop :348-365).
 *   proj (Q, d) f32 host;  idx_out (Q, k) int32;  score_out (Q, k) f32;  1 <= k <= min(V_e, 1024)
 * The ranking and the scores are those of the fp32 cosine.  For large tables (V_e >= 32768) the
 * candidates are found by a bf16 matrix-pipe pass whose proven error bound decides which
 * entities get the fp32 score; rows where that bound cannot separate the top k are computed in
 * fp32 throughout (csrc/kernels_score_bf16.h).  SERT_SCORE_FP32=1 disables the bf16 pass. */
int sert_scorer_topk(sert_scorer* s, const float* proj, int64_t num_queries, int32_t k,
                     int32_t* idx_out, float* score_out);

/* The full ranking (query.py:250-260: --top unset ranks every entity; so do --top above 1024 and above V_e), on the device.
 * k = -1 ranks every entity, k >= 1 the k best; the ranked depth kk is num_entities for k = -1 or k >= num_entities, else k
 * (the convention of sert_ll_rank_queries); k = 0 and k < -1 are refused.  idx_out / score_out (Q, kk) host arrays.
 * The order is sert_scorer_topk's: the COSINE descending (-0 equal to +0), a NaN of either sign after every number, ties and
 * the NaNs among themselves by lowest entity index; score = (cos + 1)/2 applied after the ordering; kk distinct indices
 * always.  The cosines ordered come from the branch sert_scorer_cosines takes (exact_dot32 for a bf16-prefiltered table, the
 * fp32 GEMM otherwise), in launches of at most 512 rows, so for kk > 1024 the call with k is the head of the call with -1 by
 * construction.  They are sert_scorer_cosines' bit for bit as long as that call's block stays on the fp32 GEMM kernels: not
 * for d_e >= 256 with 1024 queries or more in a block (nor from 16 384 queries at any d_e), where its GEMM runs on the
 * split-bf16 kernels and entities within a rounding of each other can be ordered differently by the two.  kk <= 1024 IS sert_scorer_topk(kk) (and carries its caveat for a bf16-prefiltered table, see
 * sert_scorer_cosines); above, V_e <= 8192 sorts each query in one workgroup's LDS, larger tables by stable counting-sort
 * passes (csrc/kernels_rank.h).  Queries are cut into chunks whose device footprint fits SERT_SCORE_RANK_BUDGET bytes
 * (default 2 GiB; at least one query); a chunk's results travel to the host while the next chunk is sorted.  For kk > 1024 a
 * query's result does not depend on the chunking or on the other queries of the call.  The kk <= 1024 path is cut by the
 * same budget into sert_scorer_topk calls: it equals one sert_scorer_topk of the whole block when it is one chunk, and
 * otherwise as far as sert_scorer_topk's own GEMM does not change kernels with the row count (it does for d_e >= 256 at
 * 1024 rows). */
int sert_scorer_rank(sert_scorer* s, const float* proj, int64_t num_queries, int32_t k,
                     int32_t* idx_out, float* score_out);

/* All scores (no selection): score_out (Q, V_e) f32 = (cos + 1)/2.  Not a ranking: (cos + 1)/2 is not injective in fp32,
 * so whoever needs the order asks sert_scorer_rank (or orders sert_scorer_cosines, below). */
int sert_scorer_scores(sert_scorer* s, const float* proj, int64_t num_queries, float* score_out);

/* All cosines (no selection, no (cos + 1)/2): cos_out (Q, V_e) f32, bit for bit the values sert_scorer_topk orders by and
 * derives its scores from on this table.  (cos + 1)/2 is not injective in fp32 -- two cosines below 0.5 in magnitude can
 * share a score -- so sert_scorer_rank, and a caller that ranks on the host, sorts THESE, under the order of sert_scorer_topk
 * (descending, -0 equal to +0, NaN after every number, ties by lowest entity index), and applies (cos + 1)/2 afterwards: the
 * first k of that ranking are then sert_scorer_topk's k -- exactly for V_e < 32768 and under SERT_SCORE_FP32=1.  For a bf16-prefiltered table
 * the cosines are the exact_dot32 ones; a row the fused path hands to the materialising path, every row of a table whose
 * prefilter was demoted and every row under SERT_SCORE_MATERIALISE=1 pick their k entities on the GEMM's cosines before
 * they are re-scored, so two entities within an fp32 rounding of each other across rank k can swap between the two.
 * An all-zero entity row or query has no direction: its cosines are NaN. */
int sert_scorer_cosines(sert_scorer* s, const float* proj, int64_t num_queries, float* cos_out);

/* Re-ranking: score and order the candidates a first stage found for each query, instead of every entity (no reference
 * counterpart: the reference ranks all of V_e and leaves the restriction to whoever reads the run file).  The candidates are
 * CSR: cand_indptr (Q + 1) int64 starts at 0 and never decreases, cand_entities int32 in [0, V_e); query q owns
 * cand_entities[cand_indptr[q] .. cand_indptr[q + 1]), which may be empty.  All arrays on the host.
 * ONE ARITHMETIC: the projections are L2-normalised as for every other call of the scorer, and a pair's cosine is exact_dot32
 * (csrc/kernels_score_bf16.h) of the normalised query row and the normalised table row -- whatever the table size, whichever
 * kernel ranks the list.  For d % 4 != 0, which exact_dot32's 16-byte loads cannot take, the same lanes own the same columns
 * and run the same fmaf chain and the same shuffle tree on scalar loads.  So
 *   - for a bf16-prefiltered table (V_e >= 32768, d % 4 == 0, no SERT_SCORE_FP32) the pair cosines are sert_scorer_cosines'
 *     values bit for bit, and the ranking of a list is sert_scorer_rank(-1)'s ranking restricted to the list;
 *   - for smaller tables sert_scorer_cosines / _scores / _rank / _topk report the fp32 GEMM's cosines, which differ from
 *     exact_dot32's within fp32 rounding: the two calls below can then differ from them in the last bits of a value, and in the
 *     order of two entities whose cosines lie within a rounding of each other.  Small tables are not routed through the GEMM to
 *     hide this: the work would again be V_e per query.
 * A failed argument check (null pointer, cand_indptr[0] != 0, a decreasing cand_indptr, an entity out of range, and for the
 * ranker an unsorted or duplicated list or a bad k) returns before anything is launched; sert_last_error names the fault.
 *
 * sert_scorer_pairs: out[j] for every j in [0, cand_indptr[Q]), in the caller's order, = the cosine of the pair (raw = 1) or
 * (cos + 1)/2 (raw = 0).  Any order and duplicates are allowed inside a list.  One half-wave per pair, the work cut by pairs
 * and not by queries (csrc/kernels_rerank.h); chunks of SERT_SCORE_RANK_BUDGET / 8 pairs. */
int sert_scorer_pairs(sert_scorer* s, const float* proj, int64_t num_queries, const int64_t* cand_indptr,
                      const int32_t* cand_entities, int raw, float* out);

/* sert_scorer_rank_candidates: every list STRICTLY ASCENDING (hence free of duplicates).  k = -1 ranks the whole list, k >= 1
 * its best min(k, length) -- the ranked depth kk_q; k = 0 and k < -1 are refused.  The results are compact: query q's kk_q
 * entries start at sum_{p < q} kk_p of idx_out / score_out (the caller sizes both from cand_indptr and k).  The order is the
 * scorer's one order (sert_scorer_rank) on the cosines sert_scorer_pairs(raw = 1) returns for the list: cosine descending
 * (-0 equal to +0), a NaN of either sign after every number, ties and the NaNs among themselves by lowest entity index; score
 * = (cos + 1)/2, applied after the ordering.  The kernel goes by the query's own list length: up to 8192 candidates are
 * scored, sorted and emitted by one workgroup in LDS; longer lists have their cosines written to a NaN-padded slab, ordered
 * by the counting-sort passes of sert_scorer_rank and mapped back to entities.  Queries are cut into chunks of consecutive
 * queries whose device footprint fits SERT_SCORE_RANK_BUDGET (at least one query; at most 2048 long lists and fewer than 2^31
 * slab elements); a query's result depends neither on the chunking nor on the other queries of the call. */
int sert_scorer_rank_candidates(sert_scorer* s, const float* proj, int64_t num_queries, const int64_t* cand_indptr,
                                const int32_t* cand_entities, int32_t k, int32_t* idx_out, float* score_out);

/* Page-locked host memory for the arrays that cross this boundary on every query call (the
 * (Q, d) projections in, the (Q, k) indices and scores out).  The reference hands numpy arrays
 * to sklearn (query.py:304-318); a caller that builds its query block in such a buffer and reads
 * the results from one lets sert_scorer_topk move them at PCIe speed, asynchronously, instead of
 * through the driver's pageable staging copies (0.4 ms of a 1.25 ms C5 call). */
int sert_host_alloc(void** out, size_t bytes);
int sert_host_free(void* p);

/* Convenience: create + topk + destroy. */
int sert_score_topk(int device, const float* entities, int64_t num_entities, int32_t dim,
                    const float* proj, int64_t num_queries, int32_t k,
                    int32_t* idx_out, float* score_out);

/* ---- folding unseen entities into a trained vectorspace model ----------- */

/* Entities that arrive after training get rows of their own without retraining: the word table, the projection and the
 * trained entity rows stay fixed and only the new rows learn, with the same NCE objective.  The handle and its calls are
 * declared in sert_hip_foldin.h, which is part of this boundary. */
#include "sert_hip_foldin.h"

/* ---- folding unseen entities into a trained loglinear model ------------- */

/* The same for the expert-finding model: R_w, W and b stay fixed and N new columns of W and entries of b learn, with the
 * model's own loss on the extended entity set.  The logits of the trained entities are cached per distinct word at upload.
 * The handle and its calls are declared in sert_hip_ll_foldin.h, which is part of this boundary. */
#include "sert_hip_ll_foldin.h"

/* ---- folding unseen words into a trained vectorspace model -------------- */

/* The other half of a catalogue that changes after training: the vocabulary grows.  The trained word rows, the projection and
 * the whole entity table stay fixed and only the rows of the new words learn, with the same NCE objective.  The handle and its
 * calls are declared in sert_hip_wfold.h, which is part of this boundary. */
#include "sert_hip_wfold.h"

/* ---- folding unseen words into a trained loglinear model ---------------- */

/* The same for the expert-finding model: the trained word rows, W and b stay fixed and only the rows of the new words learn,
 * with the model's own loss.  The handle and its calls are declared in sert_hip_ll_wfold.h, which is part of this boundary. */
#include "sert_hip_ll_wfold.h"

/* ---- data parallel (new: the reference is single-device) ---- */

#define SERT_COMM_ID_BYTES 128
/* ncclGetUniqueId; rank 0 calls it and ships the bytes to the other ranks. */
int sert_comm_unique_id(char id[SERT_COMM_ID_BYTES]);
/* ncclCommInitRank on this handle's device.  From here on the model is data parallel
 * (SURVEY 8-e, 8-f4): rank r trains rows [r*B_l, (r+1)*B_l) of every global batch.  Every rank
 * OWNS 1/world of the word table (and of any other tensor beyond 4 M elements): the dense
 * optimiser (sert/models.py:548-549: every element, every step) runs on the owned share only and
 * only that share of the optimiser state exists.
 *   word table, default: owned BY ROWS; per step two all-to-alls over static per-batch lists --
 *     the parameter rows a rank's batch touches come from their owners before the forward, their
 *     gradient rows go back after the backward (csrc/kernels_xchg.h).  Rows nobody touches do not
 *     travel.  Until the next collective read, a rank's copy of R_w is current only where it owns
 *     or has fetched: sert_get_tensor(SERT_T_RW), the evaluation calls and sert_predict_tokens then
 *     first all-gather the table and are therefore COLLECTIVE (every rank, same order).
 *   SERT_DP_EXCHANGE=zero1 (or a word dim that is no multiple of 4, keep_grads, SERT_AR_CHUNKS > 1)
 *     and every other big tensor: gradient reduce-scattered, owned slabs updated, all-gathered.
 * The small tensors' gradients and the loss sum are all-reduced and those tensors updated
 * identically everywhere.  sert_get_tensor of a SERT_T_STATE* tensor is a COLLECTIVE call. */
int sert_comm_init(sert_model* m, const char id[SERT_COMM_ID_BYTES], int rank, int world);
/* Host-mediated exchange: every collective of the data-parallel step becomes device -> pinned host
 * -> fn -> device, synchronously.  fn is an ALL-TO-ALL of float segments: on entry `send` holds, for
 * every rank q (this rank included), send_counts[q] floats at send_offsets[q]; on return `recv` must
 * hold, at recv_offsets[q], the recv_counts[q] floats rank q addressed to this rank.  Offsets and
 * counts are in floats; fn moves bits and never does arithmetic on them.  Returns 0 on success.
 * Reduce-scatter, all-gather, all-reduce and the row exchange are all expressed through it, every
 * rank receiving exactly its pieces (sums are formed in rank order on the host).  A verification
 * transport, not a fast path: it lets several ranks share ONE GPU (RCCL refuses duplicate devices),
 * so the data-parallel step -- row sharding, global 1/B scaling, rank-invariant negatives, piece and
 * slab indexing of the owned tensors, L2 applied once, loss reduction -- can be checked against a
 * single-process run on a 1-GPU box. */
typedef int (*sert_alltoall_fn)(void* user, const float* send, const int64_t* send_offsets,
                                const int64_t* send_counts, float* recv, const int64_t* recv_offsets,
                                const int64_t* recv_counts);
int sert_comm_init_host(sert_model* m, int rank, int world, sert_alltoall_fn fn, void* user);
/* Exchange statistics of a data-parallel model, out[0..n) (n <= 8):
 *   [0] world  [1] exchange of the word table: 0 none, 1 ZeRO-1 (reduce-scatter + all-gather), 2 by rows
 *   [2] bytes this rank sent + received per training step (mean over the steps run so far)
 *   [3] the same figure ZeRO-1 would move: 2 x 2 (N-1)/N x padded table bytes
 *   [4] transport: 1 RCCL, 2 host-mediated  [5] training steps counted
 *   [6] mean rows per batch this rank fetches from peers  [7] mean rows per batch it serves */
int sert_comm_stats(sert_model* m, double* out, int n);
int sert_comm_destroy(sert_model* m);

/* ---- diagnostics -------------------------------------------------------- */

/* roctx ranges around host-side phases (no reference counterpart): forwarded to
 * roctxRangePushA / roctxRangePop of the ROCm tools library when it can be loaded, no-ops otherwise.
 * With SERT_ROCTX=1 in the environment the library itself wraps every kernel group of a step (the
 * sert_timing_name groups) in a range. */
int sert_profile_range_push(const char* name);
int sert_profile_range_pop(void);

/* hipStreamSynchronize on the handle's stream. */
int sert_synchronize(sert_model* m);
/* Average duration in microseconds of the named kernel group over the steps
 * since the last sert_timing_reset (HIP events on the handle's stream).
 * Enabled with sert_timing_enable(m, 1); while enabled the step runs fully serialised
 * on one stream (each kernel is measured alone) and every event record drains the
 * stream, so a timed step is slower than an untimed one: take throughput from
 * untimed steps.  Groups: sert_timing_count / sert_timing_name.
 * sert_timing_enable(m, 2): IN-STEP timing -- the normal schedule (all streams, run-ahead of the announced batch).  Every
 * kernel of the library is started by one function (csrc/launch.h), and in this mode that function binds every plain
 * launch inside a group to a (start, stop) event pair of its own (hipExtLaunchKernel: the kernel's own dispatch
 * timestamps, no barrier packets) -- every one: no call site is left out.  sert_timing_avg_us then returns the group's
 * kernel time per training step as it runs BESIDE the other queue's kernels, sert_timing_launches its timed launches per
 * step.  The only launches not timed are those that carry a completion event of the schedule (the loss kernel or the dh
 * GEMM where the step's plan says `carried`): their groups read low or 0. */
int sert_timing_enable(sert_model* m, int on);
int sert_timing_reset(sert_model* m);
int sert_timing_count(sert_model* m);
const char* sert_timing_name(sert_model* m, int i);
double sert_timing_avg_us(sert_model* m, int i);
double sert_timing_launches(sert_model* m, int i);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_H */
