/*
 * sert_hip_ll_wfold.h -- folding unseen WORDS into a trained loglinear model.  Part of the boundary: included by sert_hip.h
 * (include that), same conventions (0 = ok, sert_last_error()), the shape of sert_hip_wfold.h.
 *
 * The loglinear model is the expert-finding model.  Its collection changes all the time through new documents by people it
 * already knows, and those documents bring project names, product names and acronyms the vocabulary has never seen.  A word
 * fold-in keeps the V_w trained word rows R_w (V_w, d), the projection W (d, V_e) and the bias b (V_e) fixed and learns only
 * Nw new word rows Nv (Nw, d), with the model's own loss, on instances whose windows may hold new words.  New word v is token
 * id V_w + v.  Stated against oracle/sert_oracle.py, with ExtW = concat(R_w, Nv), a step on batch i -- rows [iB, (i + 1)B) of
 * the uploaded instances -- is
 *     loss, grads, _ = LogLinearOracle(B, n, ExtW, W, b, lambda).loss_and_grads(X, y, w)
 * where only ExtW[V_w:] is a parameter:
 *     gradient       grads[0][V_w:]: the data term over every token position that holds a new word, plus lambda / B * Nv
 *     returned loss  sum(loss_i * w_i) / B + lambda / (2B) * sum(Nv * Nv), evaluated before the update: the L2 term covers the
 *                    trainable rows only
 *     update         oracle.Adadelta over the single tensor Nv, zero accumulators at creation, lr / rho / eps from the config;
 *                    dense -- a row that no token touched still moves by its L2 term
 * The clips are part of the contract: log clip(P) per token, clip(Q) on the label and both inclusive gradient masks, exactly
 * as in the model's step.  y holds integer labels in [0, V_e), one per instance (sert_ll_wfold_upload), or label ROWS
 * (sert_ll_wfold_upload_csr): instance i's labels are row i of a CSR matrix (M, V_e) over the trained entities, the label
 * distributions the model learns when it is trained without one-hot classes.  The contract is the same with y the dense
 * (B, V_e) slice of the rows (LogLinearOracle takes y.ndim == 2):
 *     loss_i = -sum_l Y_l log clip(Q_l),   dJ_e = Q_e (dQ_e - sum_l Q_l dQ_l),   dQ_l = -g Y_l / clip(Q_l) under the mask
 * A row may hold 0 .. V_e entries (no entry: loss 0, no gradient), a stored 0 is legal, and the values need not sum to 1.
 * R_w, W and b are never written.  An instance without a new word is legal: it adds to the loss and moves nothing.  A new
 * word twice in one window is two occurrences.
 *
 * A token's distribution depends on its word only: L_t = log softmax(row_t W + b).  The rows of the upload's distinct FROZEN
 * words Df cannot change, so they are computed once per upload by the model's own forward kernels (the frozen table,
 * (|Df|, V_e), |Df| V_e 4 bytes); the rows Ln (Nw, V_e) of the new words are computed every step (the step table).  With
 *     J_i = sum over the window's positions j of clip(L_{x_ij}),   dJ_i from the label term,
 * a new word's row gradient is the sum of dZ_ij = mask_v dJ_i - P_v <mask_v, dJ_i> over its occurrences (i, j), which is
 *     S_v = sum over the occurrences of dJ_i,   Rsum_v = <mask_v, S_v>,   dZ_v = mask_v S_v - P_v Rsum_v,   G = dZ W^T
 * -- no per-token r and no per-token dZ; lambda / B * Nv is added inside the optimiser kernel.  A step costs two Nw-row
 * GEMMs, one pass over the window's rows and an update of Nw d numbers.  Every reduction is order-fixed, there is no
 * floating-point atomic: two handles with the same inputs hold the same bits.  The result differs from the oracle's in
 * association only.
 *
 * The handle is an object of its own, like sert_wfold: it COPIES R_w, W and b from the model when it is created and shares
 * no state with the model's step schedule.  Later training or destruction of the model does not change it.
 *
 * The design's limits, and out of scope: the step table covers ALL Nw rows, not the batch's distinct new words, and three
 * V_e-wide float tables exist per handle (Ln and S / dZ of Nw rows, DJ of B rows); new entity columns in a word fold-in (fold the
 * entities in first); a per-instance cache of the frozen share of J; a wave-per-row form of the row kernel for small V_e; data-parallel handles; a frozen table that
 * spills or is recomputed.
 */
#ifndef SERT_HIP_LL_WFOLD_H
#define SERT_HIP_LL_WFOLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sert_model sert_model;
typedef struct sert_ll_wfold sert_ll_wfold;

typedef struct sert_ll_wfold_config {
    uint32_t struct_size;      /* = sizeof(sert_ll_wfold_config), checked */
    int32_t batch_size;        /* B of the fold-in (its own, not the model's): divisor of the loss mean and of lambda/(2B) */
    float lambda_;             /* regularization_lambda of the new rows */
    float lr, rho, eps;        /* Adadelta (oracle.Adadelta) */
    uint64_t max_cache_bytes;  /* upper bound of the frozen table of an upload in bytes; 0 = no cap */
} sert_ll_wfold_config;

enum { SERT_LL_WFOLD_ROWS = 0, SERT_LL_WFOLD_ACCU = 1, SERT_LL_WFOLD_DELTA = 2 };

/* A fold-in of num_new_words >= 1 words with initial rows init_rows (num_new_words, d) into model m.  The model's parameters
 * are first brought up to date, as for sert_get_tensor, then R_w, W and b are copied.  Refused with a message, before any
 * launch: a vectorspace or SERT_KIND_VECTORSPACE_SOFTMAX model; a model with a communicator attached (data parallel);
 * num_new_words < 1; a window size above 32; a bad config (struct_size, batch_size < 1, lambda < 0, rho outside [0, 1),
 * eps <= 0); V_w + num_new_words, batch_size * window_size, batch_size * V_e or num_new_words * V_e above 2^31 - 1. */
int sert_ll_wfold_create(sert_model* m, int32_t num_new_words, const float* init_rows, const sert_ll_wfold_config* cfg,
                         sert_ll_wfold** out);
int sert_ll_wfold_destroy(sert_ll_wfold* f);

/* The fold-in instances: x (M, n) int32 token ids in [0, V_w + num_new_words), y (M,) int32 in [0, V_e), w (M,) float32 instance
 * weights or NULL (all 1); M <= 2^31 - 1.  Everything is validated on the host first (no kernel is launched on a bad id).  Then,
 * once: the sorted distinct frozen words Df of x and the frozen table log softmax(R_w[Df] W + b), a slab of rows at a time; per
 * position the row of its table (>= 0: frozen table; < 0: new word ~slot); and per batch the inverted index new word -> batch
 * rows of its occurrences (csrc/wfold_index.h).  The frozen table takes |Df| V_e 4 bytes; an upload whose table exceeds
 * max_cache_bytes or cannot be allocated is refused with a message that names the bytes needed, and the handle keeps the upload
 * it held.  Batch i is rows [iB, (i + 1)B); a trailing M mod B instances are never visited, as in training.  Replaces an earlier
 * upload; the optimiser state is kept. */
int sert_ll_wfold_upload(sert_ll_wfold* f, const int32_t* x, const int32_t* y, const float* w, int64_t M);
/* The same with label ROWS: instance i owns entries indptr[i] .. indptr[i + 1] of (indices, data); indptr (M + 1,) int64,
 * indices (nnz,) int32 columns in [0, V_e) -- a word fold-in has no new entity column --, data (nnz,) float32.  Refused on the
 * host with a message, before any launch: indptr[0] != 0, indptr not non-decreasing, more than 2^31 - 1 entries, a column
 * outside [0, V_e), a row whose columns are not strictly increasing (the message names the row and the column), null arrays,
 * and everything sert_ll_wfold_upload refuses about x and M.  Everything else -- the frozen table, max_cache_bytes, the index,
 * "keeps the earlier upload" on every failure -- is sert_ll_wfold_upload's.  An upload of either kind replaces an upload of
 * either kind and keeps the optimiser state. */
int sert_ll_wfold_upload_csr(sert_ll_wfold* f, const int32_t* x, const int64_t* indptr, const int32_t* indices,
                             const float* data, const float* w, int64_t M);
/* number of complete batches of the upload, floor(M / B); < 0 on a null handle */
int64_t sert_ll_wfold_num_batches(sert_ll_wfold* f);

/* One step (see above) on batch `batch`; loss_out: the returned loss. */
int sert_ll_wfold_train_batch(sert_ll_wfold* f, int64_t batch, float* loss_out);
/* `count` steps with ONE host synchronisation: the bits of the sert_ll_wfold_train_batch loop. */
int sert_ll_wfold_train_batches(sert_ll_wfold* f, const int64_t* batches, int64_t count, float* losses_out);

/* LogLinearOracle.eval_loss(X, y) with the extended word table for batch `batch`: unweighted, unregularised; no state changes. */
int sert_ll_wfold_eval_batch(sert_ll_wfold* f, int64_t batch, float* loss_out);

/* which = SERT_LL_WFOLD_ROWS: Nv; SERT_LL_WFOLD_ACCU / _DELTA: Adadelta's two accumulators of Nv.  count must be
 * num_new_words * d. */
int sert_ll_wfold_get_rows(sert_ll_wfold* f, int which, float* host, size_t count);
int sert_ll_wfold_set_rows(sert_ll_wfold* f, int which, const float* host, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_LL_WFOLD_H */
