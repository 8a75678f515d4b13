/*
 * sert_hip_wfold.h -- folding unseen WORDS into a trained vectorspace model.  Part of the boundary: included by sert_hip.h
 * (include that), same conventions (0 = ok, sert_last_error()), the shape of sert_hip_foldin.h.
 *
 * A catalogue that changes after training brings new words: brand names, model numbers, a new category's jargon.  A word
 * fold-in keeps the V_w trained word rows R_w, the projection W, b and the WHOLE entity table R_e fixed and learns only Nw new
 * word rows Nv (Nw, d_w), with the NCE objective of the vectorspace step on instances whose windows may hold new words.  New
 * word v is token id V_w + v.  Stated against oracle/sert_oracle.py, with ExtW = concat(R_w, Nv), a step on batch i -- rows
 * [iB, (i + 1)B) of the uploaded instances -- is
 *     loss, grads, _ = VectorSpaceOracle(B, n, z, ExtW, R_e, W, b, lambda).loss_and_grads(X, y, w, neg)
 * where only ExtW[V_w:] is a parameter:
 *     gradient       grads[1][V_w:]: the data term over every token position that holds a new word, plus lambda / B * Nv
 *     returned loss  sum(loss_i * w_i) / B + lambda / (2B) * sum(Nv * Nv), evaluated before the update
 *     update         oracle.Adam over the single tensor Nv: a step counter of the handle's own that starts at 0, zero
 *                    moments; dense -- every row of Nv moves every step (L2 and the moments move rows no token touched)
 * R_w, W, b and R_e are never written.  An instance without a new word is legal: it adds to the loss and moves nothing.
 *
 * The projection is linear below the tanh, so a step needs no per-instance GEMM: with P = Nv W (Nw, d_e)
 *     a_i = [hf_i W + b] + sum over the positions j with x_ij >= V_w, ascending, of P[x_ij - V_w], the sum then divided by n
 * where hf_i is the window mean with the new positions counted as zero rows; A0 = hf W + b is computed once, at upload.  The
 * gradient folds the same way: its data term is S W^T with S[v] = (sum of the da rows of v's occurrences in the batch) / n.
 * The factor 1/n is applied ONCE PER WORD in the gradient (the segmented sum divides a word's finished sum by n) and once per
 * instance in the forward (the sum of an instance's P rows is divided by n): never per occurrence.
 * Every reduction is order-fixed, there is no floating-point atomic: two handles with the same inputs and seed hold the same
 * bits.  The result differs from the oracle's in association only.
 *
 * The handle is an object of its own, like sert_foldin: it COPIES what it needs from the model when it is created and shares
 * no state with the model's step schedule.  Later training or destruction of the model does not change it.
 */
#ifndef SERT_HIP_WFOLD_H
#define SERT_HIP_WFOLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sert_model sert_model;
typedef struct sert_wfold sert_wfold;

typedef struct sert_wfold_config {
    uint32_t struct_size;     /* = sizeof(sert_wfold_config), checked */
    int32_t batch_size;       /* B of the fold-in (its own, not the model's): divisor of the loss mean and of lambda/(2B) */
    int32_t num_negatives;    /* z >= 1 */
    float lambda_;            /* regularization_lambda of the new rows */
    float lr, beta1, beta2, eps;   /* Adam (oracle.Adam) */
    uint64_t seed;            /* device negative sampler */
} sert_wfold_config;

enum { SERT_WFOLD_ROWS = 0, SERT_WFOLD_M = 1, SERT_WFOLD_V = 2 };

/* A fold-in of num_new_words >= 1 words with initial rows init_rows (num_new_words, d_w) into model m.  The model's parameters
 * are first brought up to date, as for sert_get_tensor, then R_w, W, b and R_e are copied.  Refused with a message, before any
 * launch: a loglinear or SERT_KIND_VECTORSPACE_SOFTMAX model; a model with a communicator attached (data parallel);
 * num_new_words < 1; a bad config (batch_size < 1, num_negatives < 1, lambda < 0, struct_size); d_e > 512;
 * V_w + num_new_words > 2^31 - 1; batch_size * (1 + num_negatives) > 2^30; batch_size * window_size > 2^31 - 1. */
int sert_wfold_create(sert_model* m, int32_t num_new_words, const float* init_rows, const sert_wfold_config* cfg, sert_wfold** out);
int sert_wfold_destroy(sert_wfold* f);

/* The fold-in instances: x (M, n) int32 token ids in [0, V_w + num_new_words), y (M,) int32 in [0, V_e), w (M,) float32 instance
 * weights or NULL (all 1); M <= 2^31 - 1.  Everything is validated on the host first (no kernel is launched on a bad id).  Then,
 * once: A0 = hf W + b of all M instances by the model's forward (window mean with the new positions pointed at a zero row,
 * projection GEMM), the new-word token of every position (-1: frozen), and per batch the inverted index new word -> batch rows
 * of its occurrences (ascending by (row, position); a word twice in a window is two entries; lists longer than 64 entries are
 * cut into chunks whose sums are added in chunk order at a further level).  Batch i is rows [iB, (i + 1)B); a trailing M mod B
 * instances are never visited, as in training.  Replaces an earlier upload; the optimiser state is kept. */
int sert_wfold_upload(sert_wfold* f, const int32_t* x, const int32_t* y, const float* w, int64_t M);
/* number of complete batches of the upload, floor(M / B); < 0 on a null handle */
int64_t sert_wfold_num_batches(sert_wfold* f);

/* One step (see above) on batch `batch`; loss_out: the returned loss.  negatives: (B, z) int64 in [0, V_e) -- refused with a
 * message otherwise, before anything is launched -- or NULL: drawn on the device by the model's Philox sampler over V_e
 * entities, keyed by (seed, the handle's step counter before the step); even draws train, odd draws evaluate. */
int sert_wfold_train_batch(sert_wfold* f, int64_t batch, const int64_t* negatives, float* loss_out);
/* `count` steps with device-drawn negatives and ONE host synchronisation: the bits of the sert_wfold_train_batch loop. */
int sert_wfold_train_batches(sert_wfold* f, const int64_t* batches, int64_t count, float* losses_out);

/* VectorSpaceOracle.eval_loss with the extended word table for batch `batch`: unweighted, unregularised, no update and no state
 * changed except -- with negatives == NULL -- the position of the evaluation sampler (advanced by one per call). */
int sert_wfold_eval_batch(sert_wfold* f, int64_t batch, const int64_t* negatives, float* loss_out);

/* (B, z) int64: what the device sampler draws at training position `position` (= sert_wfold_get_step before the step) or,
 * evaluation != 0, for the position-th evaluation draw.  A pure function of (seed, position, evaluation). */
int sert_wfold_negatives_of_step(sert_wfold* f, int64_t position, int evaluation, int64_t* out);

/* which = SERT_WFOLD_ROWS: Nv; SERT_WFOLD_M / SERT_WFOLD_V: Adam's moments of Nv.  count must be num_new_words * d_w. */
int sert_wfold_get_rows(sert_wfold* f, int which, float* host, size_t count);
int sert_wfold_set_rows(sert_wfold* f, int which, const float* host, size_t count);

/* Adam's step counter t of the fold-in = the position of its training sampler; the position of its evaluation sampler. */
int sert_wfold_set_step(sert_wfold* f, int64_t t);
int64_t sert_wfold_get_step(sert_wfold* f);
int sert_wfold_set_eval_draws(sert_wfold* f, int64_t n);
int64_t sert_wfold_get_eval_draws(sert_wfold* f);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_WFOLD_H */
