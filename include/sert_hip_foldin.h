/*
 * sert_hip_foldin.h -- folding unseen entities into a trained vectorspace model.  Part of the boundary: included by
 * sert_hip.h (include that), same conventions (0 = ok, sert_last_error()).
 *
 * A catalogue gains entities after training.  A fold-in keeps the word table R_w, the projection W, b and the V_e trained
 * entity rows R_e fixed and learns only N new rows E, with the NCE objective of the vectorspace step on the new entities'
 * instances.  Stated against oracle/sert_oracle.py, with Ext = concat(R_e, E) (new entity e is row V_e + e), a step on batch
 * i -- rows [iB, (i + 1)B) of the uploaded instances -- is
 *     loss, grads, _ = VectorSpaceOracle(B, n, z, R_w, Ext, W, b, lambda).loss_and_grads(X, V_e + y, w, neg)
 * where only Ext[V_e:] is a parameter:
 *     gradient       grads[0][V_e:]: the data term over every pair (positive or negative) whose candidate is a new row, plus
 *                    lambda / B * E
 *     returned loss  sum(loss_i * w_i) / B + lambda / (2B) * sum(E * E), evaluated before the update
 *     update         oracle.Adam over the single tensor E: a step counter of the fold-in's own that starts at 0, zero
 *                    moments; dense -- every row of E moves every step (L2 and the moments move rows no pair touched)
 * R_w, W, b and Ext[:V_e] are never written.  The projections tanh(h W + b) of the instances cannot change, so they are
 * computed once, at upload; a step runs no gather, no GEMM and no word-table update.  Every reduction is order-fixed: two
 * handles with the same inputs and seed hold the same bits.
 *
 * The handle is an object of its own, like sert_scorer: it COPIES what it needs from the model when it is created and
 * shares no state with the model's step schedule.  Later training or destruction of the model does not change it.
 */
#ifndef SERT_HIP_FOLDIN_H
#define SERT_HIP_FOLDIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sert_model sert_model;
typedef struct sert_foldin sert_foldin;

typedef struct sert_foldin_config {
    uint32_t struct_size;     /* = sizeof(sert_foldin_config), checked */
    int32_t batch_size;       /* B of the fold-in (its own, not the model's): divisor of the loss mean and of lambda/(2B) */
    int32_t num_negatives;    /* z >= 1 */
    float lambda_;            /* regularization_lambda of the new rows */
    float lr, beta1, beta2, eps;   /* Adam (oracle.Adam) */
    uint64_t seed;            /* device negative sampler */
} sert_foldin_config;

enum { SERT_FOLDIN_ROWS = 0, SERT_FOLDIN_M = 1, SERT_FOLDIN_V = 2 };

/* A fold-in of num_new >= 1 entities with initial rows init_rows (num_new, d_e) into model m.  The model's parameters are
 * first brought up to date, as for sert_get_tensor (lazy word-table rows, a deferred entity-table update), then R_w, W, b and
 * R_e are copied.  Refused with a message: a loglinear or SERT_KIND_VECTORSPACE_SOFTMAX model; a model with a communicator
 * attached (data parallel); num_new < 1; a bad config (batch_size < 1, num_negatives < 1, lambda < 0, struct_size). */
int sert_foldin_create(sert_model* m, int32_t num_new, const float* init_rows, const sert_foldin_config* cfg, sert_foldin** out);
int sert_foldin_destroy(sert_foldin* f);

/* REFRESH: a fold-in whose trainable table E is any set of rows of the extended table -- trained rows that gained documents
 * (new reviews of a known product) and new entities, in one handle.  E has Nt = num_refresh + num_new rows, the SLOTS:
 *     slot s < num_refresh      trained row refresh_ids[s]; its initial value is copied on the device from the model's R_e, after
 *                               the preamble of sert_foldin_create
 *     slot num_refresh + e      new entity e = row V_e + e of Ext; its initial value is init_new_rows[e]
 * With ext_of_slot the row of Ext a slot stands for and Ext = concat(R_e, new rows) in which EVERY slot's current value is
 * written to its row, a step on batch i is, against oracle/sert_oracle.py,
 *     loss, grads, _ = VectorSpaceOracle(B, n, z, R_w, Ext, W, b, lambda).loss_and_grads(X, ext_of_slot[y], w, neg)
 *     gradient       grads[0][ext_of_slot], the Nt rows in slot order, plus lambda / B * E
 *     returned loss  sum(loss_i * w_i) / B + lambda / (2B) * sum(E * E) over the Nt trainable rows only
 *     update         oracle.Adam over the single tensor E: zero moments, a step counter of the handle's own, dense over all
 *                    Nt rows
 * y at upload is a SLOT in [0, Nt): every instance's positive is a trainable row.  Negatives are ids of the extended table in
 * [0, V_e + num_new), explicit or from the unchanged Philox sampler over V_e + num_new; a negative that names a refreshed row
 * moves it, as in the oracle.  sert_foldin_get_rows / sert_foldin_set_rows take Nt * d_e values in slot order.  R_w, W, b and
 * every trained row not in refresh_ids are never written; the snapshot's stale copy of a refreshed row is never read.  Upload,
 * the projection slabs, train_batches, eval_batch, negatives_of_step and the step and sampler state work as on a handle of
 * sert_foldin_create.  A refreshed row learns from the instances given: to keep its old evidence, upload the entity's old
 * documents along with the new ones.
 * refresh_ids: distinct, each in [0, V_e), any order; may be NULL iff num_refresh == 0.  init_new_rows: (num_new, d_e); may be
 * NULL iff num_new == 0.  Refused with a message before any launch: num_refresh < 0 or num_new < 0; Nt < 1; a null array with
 * a positive count; an id outside [0, V_e); a duplicate id; and everything sert_foldin_create refuses (loglinear, the
 * full-softmax variant, a communicator, the config, d_e > 512, the size limits).  With num_refresh == 0 the handle holds the
 * bits of sert_foldin_create(num_new) on the same inputs and seed. */
int sert_foldin_create_refresh(sert_model* m, const int32_t* refresh_ids, int32_t num_refresh, int32_t num_new,
                               const float* init_new_rows, const sert_foldin_config* cfg, sert_foldin** out);

/* The fold-in instances: x (M, n) int32 token ids in [0, V_w), y (M,) int32 in [0, num_new) (a refresh handle: a slot in
 * [0, Nt)), w (M,) float32 instance
 * weights or NULL (all 1).  Validated on the host (no kernel is launched on bad ids), then the projections
 * T = VectorSpaceOracle.forward(x, ..)['t'] = tanh(h W + b) of all M instances are computed and kept (the model's
 * forward: window mean, projection GEMM).  Batch i is rows [iB, (i + 1)B); a trailing M mod B instances are never
 * visited, as in training.  Replaces an earlier upload; the optimiser state is kept. */
int sert_foldin_upload(sert_foldin* f, const int32_t* x, const int32_t* y, const float* w, int64_t M);
/* number of complete batches of the upload, floor(M / B); < 0 on a null handle */
int64_t sert_foldin_num_batches(sert_foldin* f);

/* One step (see above) on batch `batch`; loss_out: the returned loss.  negatives: (B, z) int64 in [0, V_e + num_new) --
 * refused with a message otherwise, before anything is launched -- or NULL: drawn on the device by the model's Philox
 * sampler over V_e + num_new entities (iid uniform, with replacement, target not excluded), keyed by (seed, the fold-in's
 * step counter before the step). */
int sert_foldin_train_batch(sert_foldin* f, int64_t batch, const int64_t* negatives, float* loss_out);
/* `count` steps with device-drawn negatives and ONE host synchronisation: the bits of the sert_foldin_train_batch loop. */
int sert_foldin_train_batches(sert_foldin* f, const int64_t* batches, int64_t count, float* losses_out);

/* VectorSpaceOracle.eval_loss on the extended table for batch `batch`: unweighted, unregularised, no update and no state
 * changed except -- with negatives == NULL -- the position of the evaluation sampler (the odd Philox stream, advanced by one
 * per call). */
int sert_foldin_eval_batch(sert_foldin* f, int64_t batch, const int64_t* negatives, float* loss_out);

/* (B, z) int64: what the device sampler draws at training position `position` (= sert_foldin_get_step before the step) or,
 * evaluation != 0, for the position-th evaluation draw.  A pure function of (seed, position, evaluation). */
int sert_foldin_negatives_of_step(sert_foldin* f, int64_t position, int evaluation, int64_t* out);

/* which = SERT_FOLDIN_ROWS: E; SERT_FOLDIN_M / SERT_FOLDIN_V: Adam's moments of E.  count must be num_new * d_e (a refresh
 * handle: Nt * d_e, slot order). */
int sert_foldin_get_rows(sert_foldin* f, int which, float* host, size_t count);
int sert_foldin_set_rows(sert_foldin* f, int which, const float* host, size_t count);

/* Adam's step counter t of the fold-in = the position of its training sampler; the position of its evaluation sampler. */
int sert_foldin_set_step(sert_foldin* f, int64_t t);
int64_t sert_foldin_get_step(sert_foldin* f);
int sert_foldin_set_eval_draws(sert_foldin* f, int64_t n);
int64_t sert_foldin_get_eval_draws(sert_foldin* f);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_FOLDIN_H */
