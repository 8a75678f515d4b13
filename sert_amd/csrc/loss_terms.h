// The loss terms of the reference, each stated ONCE ("One statement of each loss term").  A kernel of
// kernels_vs.h, kernels_foldin.h, kernels_ll.h, kernels_seg.h or kernels_egrad.h that needs one calls it from here and does
// not restate it: a correction (the next NaN, a clip detail of Theano's) is made in this file and reaches every kernel.
//   nce_term                     sigmoid, clip, log, inclusive mask, du              sert/models.py:896-900
//   clip_proj / clip_proj_bwd    clip of the projection and Clip.grad * tanh'        sert/models.py:1065-1068
//   prob_inside                  the clip's inclusive gradient mask on a probability
//   LlLabels / ll_label_term     a row's label entries; -y log clip(q), q dq         sert/models.py:289-292
//   logp_inside / ll_dz          the clip mask of a LOG-probability; dZ = mask dJ - P r   sert/models.py:200-212
//   fs_label_term                the full-softmax label entry                        sert/models.py:289-292
// Every helper is __forceinline__: after inlining a kernel holds the operations it held when it spelled them out, in
// the same order (checked against the parent bit for bit, tools/ab_bits.py).  A helper with two results hands them back
// through REFERENCES, not in a struct: returned as a pair of floats, the two products of ll_label_term were packed into one
// v_pk_mul_f32 in ll_row_wave and the row's loss lost the fma it is summed with -- other bits in a row with two labels on a lane.
#pragma once
#include "common.h"

namespace sert {

// the INCLUSIVE gradient mask of clip(p, eps, 1 - eps) on a probability ([upstream Clip.grad]); false for a NaN
__device__ __forceinline__ bool prob_inside(float p) { return (p >= SERT_CLIP_LO) && (p <= SERT_CLIP_HI); }

// ---- NCE (vectorspace step, fold-in) ----------------------------------------------------------------------------------
// One candidate of one instance, u = <R_e[c], clip(t)>:  sig = sigmoid(u), s = clip(sig, eps, 1 - eps),
//   logterm = log s (the positive) or log(1 - s) (a negative) -- the caller SUBTRACTS it from the row's loss;
//   TRAIN: du = d loss / d u, with g = w_i / B, under the clip's INCLUSIVE gradient mask on sig ([upstream Clip.grad]); else 0.
template <bool TRAIN>
__device__ __forceinline__ void nce_term(float u, bool positive, float g, float& logterm, float& du) {
#if defined(SERT_VARIANTS) && defined(KO_MATH)   // timing knock-out (wrong results), variants build only
    const float sig = u * 0.01f + 0.5f;
    const float s = clip_prob(sig);
    logterm = s;
#else
    const float sig = theano_sigmoid(u);
    const float s = clip_prob(sig);
    logterm = positive ? logf(s) : logf(1.0f - s);
#endif
    du = 0.f;
    if (TRAIN) {
        if (prob_inside(sig)) {
            const float ds = sig * (1.0f - sig);
            du = positive ? -(g / s) * ds : (g / (1.0f - s)) * ds;
        }
    }
}

// ---- clip of the projection ----------------------------------------------------------------------------------------------
// p = clip(t, -(1 - eps), 1 - eps) in front of a dot product.  This one KEEPS the fminf(fmaxf()) form, which turns a NaN
// unit into -(1 - eps): the NaN-keeping selects of clip_unit (common.h) are value-identical for every finite t but change
// how the compiler contracts the dot products behind the clip.  The NaN of a unit reaches the loss beside it, through
// row_nan (kernels_vs.h).  A kernel that STORES clip(t) uses clip_unit.
__device__ __forceinline__ float clip_proj(float t) { return fminf(fmaxf(t, -SERT_CLIP_HI), SERT_CLIP_HI); }
__device__ __forceinline__ float4 clip_proj(const float4& t) {
    return make_float4(clip_proj(t.x), clip_proj(t.y), clip_proj(t.z), clip_proj(t.w));
}
// da = dp * [|t| <= 1 - eps] * (1 - t^2)   (Clip.grad, inclusive, times tanh')
__device__ __forceinline__ float clip_proj_bwd(float t, float dp) {
    return (t >= -SERT_CLIP_HI && t <= SERT_CLIP_HI) ? dp * (1.0f - t * t) : 0.f;
}
__device__ __forceinline__ float4 clip_proj_bwd(const float4& t, const float4& dp) {
    return make_float4(clip_proj_bwd(t.x, dp.x), clip_proj_bwd(t.y, dp.y), clip_proj_bwd(t.z, dp.z), clip_proj_bwd(t.w, dp.w));
}

// ---- loglinear label entries -----------------------------------------------------------------------------------------------
// The label entries of batch row i: ONE entry (entity y_int[i], value 1) with integer labels, else the CSR row
// indptr[i] .. indptr[i + 1] of (indices, data) -- the reference densifies it per batch (models.py:66-89).  Entries are
// l0 <= l < l1; `slot(l)` is where a per-entry scratch value of the row lives (ll_s_rowloss -> ll_s_labfix).
struct LlLabels {
    const int32_t* __restrict__ y_int;
    const int32_t* __restrict__ indices;
    const float* __restrict__ data;
    int i;
    int64_t l0, l1;
    __device__ __forceinline__ LlLabels(const int32_t* __restrict__ y_int_, const int64_t* __restrict__ indptr,
                                        const int32_t* __restrict__ indices_, const float* __restrict__ data_, int i_)
        : y_int(y_int_), indices(indices_), data(data_), i(i_), l0(0), l1(1) {
        if (y_int == nullptr) { l0 = indptr[i]; l1 = indptr[i + 1]; }
    }
    __device__ __forceinline__ int entity(int64_t l) const { return y_int ? y_int[i] : indices[l]; }
    __device__ __forceinline__ float value(int64_t l) const { return y_int ? 1.f : data[l]; }
    __device__ __forceinline__ int64_t slot(int64_t l) const { return y_int ? (int64_t)i : l; }
};
// One label entry, q = Q_e, yv = Y_e:  ylog = y log clip(q) -- the caller SUBTRACTS it from the row's loss;
//   TRAIN: qdq = Q_e dQ_e, dQ_e = -g y / clip(q) under the inclusive mask eps <= q <= 1 - eps; else 0.
template <bool TRAIN>
__device__ __forceinline__ void ll_label_term(float q, float yv, float g, float& ylog, float& qdq) {
    const float qc = clip_prob(q);
    ylog = yv * logf(qc);
    qdq = TRAIN ? q * (prob_inside(q) ? -(g * yv) / qc : 0.f) : 0.f;
}

// ---- the token distributions, in the log domain ------------------------------------------------------------------------------
// the clip's inclusive mask eps <= P <= 1 - eps on lp = log P (lo = log eps, hi = log(1 - eps)); false for a NaN
__device__ __forceinline__ bool logp_inside(float lp, float lo, float hi) { return lp >= lo && lp <= hi; }
// dJ where the mask holds
__device__ __forceinline__ float ll_masked(float lp, float dj, float lo, float hi) { return logp_inside(lp, lo, hi) ? dj : 0.f; }
// dZ = mask dJ - P r
__device__ __forceinline__ float ll_dz(float lp, float dj, float r, float lo, float hi) {
    return ll_masked(lp, dj, lo, hi) - __expf(lp) * r;
}
__device__ __forceinline__ float4 ll_dz(const float4& lp, const float4& dj, float r, float lo, float hi) {
    return make_float4(ll_dz(lp.x, dj.x, r, lo, hi), ll_dz(lp.y, dj.y, r, lo, hi), ll_dz(lp.z, dj.z, r, lo, hi),
                       ll_dz(lp.w, dj.w, r, lo, hi));
}

// ---- full softmax -----------------------------------------------------------------------------------------------------------
// The label's entry, py = P[y_i]:  loss = -w_i log clip(py);  TRAIN: g = w_i / B under the inclusive mask on py, else 0.
template <bool TRAIN>
__device__ __forceinline__ void fs_label_term(float py, float wi, float inv_batch, float& loss, float& g) {
    loss = -wi * logf(clip_prob(py));
    g = (TRAIN && prob_inside(py)) ? wi * inv_batch : 0.f;
}

}  // namespace sert
