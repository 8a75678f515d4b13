/*
 * sert_hip_ll_foldin.h -- folding unseen entities into a trained loglinear model.  Part of the boundary: included by
 * sert_hip.h (include that), same conventions (0 = ok, sert_last_error()).
 *
 * The loglinear model is the expert-finding model, whose entity set changes most often: people join.  A fold-in keeps the word
 * table R_w (V_w, d), the projection W (d, V_e) and the bias b (V_e) fixed and learns only N new columns Wn (d, N) and N new
 * biases bn (N), on the new entities' instances; new entity e is column V_e + e.  Stated against oracle/sert_oracle.py, with
 * Wx = concat(W, Wn, axis=1) and bx = concat(b, bn), a step on batch i -- rows [iB, (i + 1)B) of the uploaded instances -- is
 *     loss, grads, _ = LogLinearOracle(B, n, R_w, Wx, bx, lambda).loss_and_grads(X, V_e + y, w)
 * where only Wx[:, V_e:] and bx[V_e:] are parameters:
 *     gradient       grads[1][:, V_e:], which includes lambda / B * Wn, and grads[2][V_e:] (the bias is not regularised)
 *     returned loss  sum(loss_i * w_i) / B + lambda / (2B) * sum(Wn * Wn), evaluated before the update: the L2 term covers the
 *                    trainable columns only
 *     update         oracle.Adadelta over [Wn, bn], zero accumulators at creation, lr / rho / eps from the config
 * The clips are part of the contract: log clip(P) per token, clip(Q) on the label and their inclusive gradient masks, exactly
 * as in the model's step.  R_w, W and b are never written.  The logits of the V_e trained entities for a word cannot change, so
 * they are computed once, at upload, for the upload's distinct words (the logit cache); a step runs an N-wide GEMM, one row
 * kernel over the cached logits and Adadelta on d N + N numbers -- no V_e-wide GEMM, no word-table update.  Every reduction is
 * order-fixed and there are no floating-point atomics: two handles with the same inputs hold the same bits.
 *
 *
 * Label rows.  The expert-finding recipe trains on label DISTRIBUTIONS (bin/train.py without --one_hot_classes: one CSR row per
 * instance, loss_i = -sum_e Y_ie log clip(Q_ie)), and a new person's documents are mostly co-authored with people the model
 * knows.  sert_ll_foldin_upload_csr takes such rows over all V_e + N columns: column e < V_e is trained entity e -- a label
 * only, its parameters stay frozen, but its share of the label mass enters the new columns' gradient through the joint's
 * normaliser and through r_t --, column V_e + j is new entity j.  The step is then, with Ydense the batch's rows densified to
 * (B, V_e + N),
 *     loss, grads, _ = LogLinearOracle(B, n, R_w, Wx, bx, lambda).loss_and_grads(X, Ydense, w)
 * with the gradient, the returned loss and the update as above.  A label on a trained column costs a gather from the logit
 * cache; the cache itself is the same.
 *
 * Refreshing trained columns.  The more common event in an expert-finding collection is that people the model KNOWS write new
 * documents.  sert_ll_foldin_create_refresh makes the trainable columns SLOTS, as sert_foldin_create_refresh does for rows:
 * R = num_refresh trained columns (the refreshed ones), then N = num_new new ones, Nt = R + N >= 1.  Slot s < R stands for
 * trained column refresh_ids[s], slot R + j for column V_e + j; ext_of_slot names that column of the extended model.  With
 * Wx (d, V_e + N) = concat(W, Wn_new) and bx = concat(b, bn_new) in which every slot's CURRENT value is written to its
 * column, a step on batch i is, for integer labels -- y is a SLOT in [0, Nt) --,
 *     loss, grads, _ = LogLinearOracle(B, n, R_w, Wx, bx, lambda).loss_and_grads(X, ext_of_slot[y], w)
 * and for label rows loss_and_grads(X, Ydense, w): the CSR columns stay the PUBLIC ones, e < V_e trained entity e, V_e + j
 * new entity j; a trained column that is refreshed is now a parameter, one that is not stays a frozen co-label.
 *     gradient       columns ext_of_slot of grads[1] and of grads[2]
 *     returned loss  sum(loss_i * w_i) / B + lambda / (2B) * the sum of squares of the Nt trainable columns (not of the bias)
 *     update         oracle.Adadelta over the slot-ordered [Wt (d, Nt), bt (Nt)], zero accumulators at creation
 * sert_ll_foldin_eval_batch is eval_loss on Wx, bx.  R_w and every trained column not in refresh_ids are never written.  A
 * refreshed column starts from its trained value and bias, copied on the device from the model.  It learns from the instances
 * given: to keep an entity's old evidence, upload its old documents along with the new ones.
 * The step does not know about any of this: the handle keeps the V_f = V_e - R frozen columns compact, in ascending trained
 * index, and runs the step above as a fold-in of Nt columns into a model of V_f entities -- the logit cache of an upload
 * takes |D| V_f 4 bytes, and label rows are brought to that column order on the host at upload.  V_f = 0 (every trained
 * column refreshed) is supported: there is no cache then.
 *
 * The handle is an object of its own, like sert_foldin: it COPIES what it needs from the model when it is created and shares
 * no state with the model's step schedule.  Later training or destruction of the model does not change it.
 * Out of scope: data-parallel handles, window sizes above 32, a logit cache that spills or is recomputed per step.
 */
#ifndef SERT_HIP_LL_FOLDIN_H
#define SERT_HIP_LL_FOLDIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sert_model sert_model;
typedef struct sert_ll_foldin sert_ll_foldin;

typedef struct sert_ll_foldin_config {
    uint32_t struct_size;      /* = sizeof(sert_ll_foldin_config), checked */
    int32_t batch_size;        /* B of the fold-in (its own, not the model's): divisor of the loss mean and of lambda/(2B) */
    float lambda_;             /* regularization_lambda of the new columns */
    float lr, rho, eps;        /* Adadelta (oracle.Adadelta) */
    uint64_t max_cache_bytes;  /* upper bound of the logit cache of an upload in bytes; 0 = no cap */
} sert_ll_foldin_config;

enum {
    SERT_LL_FOLDIN_W = 0, SERT_LL_FOLDIN_B = 1, SERT_LL_FOLDIN_ACCU_W = 2, SERT_LL_FOLDIN_ACCU_B = 3,
    SERT_LL_FOLDIN_DELTA_W = 4, SERT_LL_FOLDIN_DELTA_B = 5
};

/* A fold-in of num_new >= 1 entities into model m, with initial columns init_W (d, num_new) row-major and initial biases
 * init_b (num_new) or NULL (zeros).  The model's parameters are first brought up to date, as for sert_get_tensor, then R_w, W
 * and b are copied.  Refused with a message, before any launch: a vectorspace or SERT_KIND_VECTORSPACE_SOFTMAX model; a model
 * with a communicator attached (data parallel); num_new < 1; a window size above 32; a bad config (struct_size, batch_size < 1,
 * lambda < 0, rho outside [0, 1), eps <= 0); the size limits (V_e + num_new and B n num_new below 2^31). */
int sert_ll_foldin_create(sert_model* m, int32_t num_new, const float* init_W, const float* init_b,
                          const sert_ll_foldin_config* cfg, sert_ll_foldin** out);
/* The same with slots (see "Refreshing trained columns" above): refresh_ids (num_refresh) distinct trained columns in
 * [0, V_e), any order -- NULL if and only if num_refresh == 0 --, then num_new new columns with init_new_W (d, num_new)
 * row-major -- NULL if and only if num_new == 0 -- and init_new_b (num_new) or NULL (zeros).  A refreshed column starts from
 * the model's own column and bias.  Refused with a message, before any launch: negative counts; num_refresh + num_new < 1;
 * a null array with a positive count (and an array with a count of 0); an id out of range; a duplicate id; and everything
 * sert_ll_foldin_create refuses, its size limits applied to Nt = num_refresh + num_new in the place of num_new.  With
 * num_refresh == 0 the handle holds the bits of sert_ll_foldin_create(num_new) on the same inputs.
 * On such a handle sert_ll_foldin_upload takes y in [0, Nt), a slot; sert_ll_foldin_upload_csr the public columns
 * [0, V_e + num_new) it always takes; sert_ll_foldin_get_tensor / _set_tensor d * Nt or Nt values in slot order; the logit
 * cache and max_cache_bytes count the V_f = V_e - num_refresh frozen columns. */
int sert_ll_foldin_create_refresh(sert_model* m, const int32_t* refresh_ids, int32_t num_refresh, int32_t num_new,
                                  const float* init_new_W, const float* init_new_b, const sert_ll_foldin_config* cfg,
                                  sert_ll_foldin** out);
int sert_ll_foldin_destroy(sert_ll_foldin* f);

/* The fold-in instances: x (M, n) int32 token ids in [0, V_w), y (M,) int32 in [0, num_new) -- one label per instance --, w (M,)
 * float32 instance weights or NULL (all 1).  Validated on the host (no kernel is launched on bad ids).  Then, once per upload:
 * the sorted distinct words D of x, the logit cache Zold = R_w[D] W + b of shape (|D|, V_e), and per word the (max, sum exp)
 * of its row.  The cache takes |D| V_e 4 bytes; an upload whose cache exceeds max_cache_bytes or cannot be allocated is refused
 * with a message that names the bytes needed, and the handle keeps what it held (a failed allocation: no upload).  Batch i is
 * rows [iB, (i + 1)B); a trailing M mod B instances are never visited, as in training.  Replaces an earlier upload; the
 * optimiser state is kept. */
int sert_ll_foldin_upload(sert_ll_foldin* f, const int32_t* x, const int32_t* y, const float* w, int64_t M);
/* The same with label ROWS: x, w, M, the batches, the trailing M mod B, the logit cache and max_cache_bytes exactly as above;
 * the labels are a canonical CSR matrix (M, V_e + num_new) -- indptr (M + 1) starts at 0 and does not decrease; the columns
 * of a row (indices) lie in [0, V_e + num_new) and are STRICTLY INCREASING; a row holds any number of entries from none (loss
 * 0, no gradient) to V_e + num_new; the values (data) are what sert_upload_dataset takes for csr_data: arbitrary finite
 * floats, a stored 0, rows that do not sum to 1; fewer than 2^31 entries.  Column e < V_e is trained entity e (a label only),
 * column V_e + j new entity j.  Every fault is found on the host before anything is launched, with sert_upload_dataset's
 * wording for csr_*; a refused upload keeps the earlier one.  An upload of either form replaces an upload of either form;
 * the optimiser state is kept. */
int sert_ll_foldin_upload_csr(sert_ll_foldin* f, const int32_t* x, const int64_t* indptr, const int32_t* indices,
                              const float* data, const float* w, int64_t M);
/* number of complete batches of the upload, floor(M / B); < 0 on a null handle */
int64_t sert_ll_foldin_num_batches(sert_ll_foldin* f);

/* One step (see above) on batch `batch`; loss_out: the returned loss. */
int sert_ll_foldin_train_batch(sert_ll_foldin* f, int64_t batch, float* loss_out);
/* `count` steps with ONE host synchronisation: the bits of the sert_ll_foldin_train_batch loop. */
int sert_ll_foldin_train_batches(sert_ll_foldin* f, const int64_t* batches, int64_t count, float* losses_out);

/* LogLinearOracle.eval_loss(X, V_e + y) -- label rows: eval_loss(X, Ydense) -- on the extended model for batch `batch`:
 * unweighted, unregularised; no state changes. */
int sert_ll_foldin_eval_batch(sert_ll_foldin* f, int64_t batch, float* loss_out);

/* which = SERT_LL_FOLDIN_W / _B: Wn (d, num_new) row-major / bn (num_new); _ACCU_* / _DELTA_*: Adadelta's two accumulators of
 * either.  count must be d * num_new or num_new. */
int sert_ll_foldin_get_tensor(sert_ll_foldin* f, int which, float* host, size_t count);
int sert_ll_foldin_set_tensor(sert_ll_foldin* f, int which, const float* host, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_LL_FOLDIN_H */
