/*
 * sert_hip_reval_counted.h -- retrieval evaluation at any depth, by counting ranks.  Part of the boundary: included by
 * sert_hip.h (include that), same conventions (0 = ok, sert_last_error()).
 *
 * sert_reval_create holds the vectorspace kinds to k in 1 .. min(num_entities, 1024), the range of sert_scorer_topk, and
 * keeps a (Q, k) ranking on the device.  Every figure sert_reval_run reports depends only on the RANKS of a topic's judged
 * entities, and a rank under the scorer's order is a count: one plus the number of entities that precede the judged one.
 * A counted handle makes that count in one streaming pass over the topic's cosine row -- no sort, no (Q, depth) array -- so
 * its depth may be anything: MAP at trec_eval's 1000, NDCG over the whole collection.
 */
#ifndef SERT_HIP_REVAL_COUNTED_H
#define SERT_HIP_REVAL_COUNTED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sert_model sert_model;
typedef struct sert_reval sert_reval;

/* The evaluator by rank counting: same arguments and validation as sert_reval_create; vectorspace kinds only (a loglinear
 * model is refused with a message: it ranks every entity through sert_reval_create); k = -1 (every entity) or any positive
 * k; depth kk = num_entities for k = -1 or k >= num_entities, else k; k = 0 and k < -1 are refused.  Device memory: the
 * topics and judgements, one (min(Q, 512), num_entities) f32 cosine buffer, one int32 per judged entity and the kk + 1
 * float64 of the log2 table -- nothing else grows with the depth.  Destroyed by sert_reval_destroy. */
int sert_reval_create_counted(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_topics,
                              const int64_t* rel_indptr, const int32_t* rel_entities, const float* rel_gains,
                              const double* ideal_dcg, const int32_t* num_rel, int32_t k, sert_reval** out);

/* sert_reval_run on a counted handle: the same preamble (parameters brought up to date as for sert_get_tensor, an announced
 * batch stays announced, nothing training depends on changes, COLLECTIVE in data parallel), then mean of the topic's word
 * rows -> sert_predict_project's GEMM -> the live entity table normalised -> per slab of at most 512 topics the cosine slab
 * of sert_scorer_rank (exact_dot32 for a bf16-prefiltered table, the fp32 GEMM otherwise), the ranks of the judged entities
 * counted over it, the metrics from the ranks.
 *   rank(q, e) = 1 + #{e' : (key(cos[q][e']), e') < (key(cos[q][e]), e)}, key = the scorer's (cosine descending, -0 equal
 *     to +0, a NaN of either sign after every number; ties and the NaNs among themselves by lowest entity index): a judged
 *     entity's rank IS its position in sert_scorer_rank(proj, -1) on the same parameters, ties and NaNs included.
 *   metrics_out as for sert_reval_run, each the definition of the ranking form restated on ranks <= kk; float64 sums in
 *     judgement-list order (csrc/kernels_reval.h), independent of the other topics and of the slab a topic falls into.
 *   status_out: all SERT_LL_STATUS_DEVICE.   idx_out / score_out: must be NULL -- a counted handle makes no ranking
 *     (sert_scorer_rank returns one); anything else is refused with a message.
 *
 * sert_reval_judged_ranks: the ranks the last sert_reval_run of a counted handle found: ranks_out (rel_indptr[Q]) int32,
 * 1-based, aligned with rel_entities, pairwise distinct inside a topic; NOT cut at the depth.  Refused for a handle of
 * sert_reval_create and before the first run. */
int sert_reval_judged_ranks(sert_reval* r, int32_t* ranks_out);

#ifdef __cplusplus
}
#endif
#endif /* SERT_HIP_REVAL_COUNTED_H */
