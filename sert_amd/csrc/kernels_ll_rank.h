// Batched loglinear query ranking (bin/query.py:199-236 LogLinearCallback.process, sert/inference.py:170-174
// aggregate_distribution(mode='product')), gfx950.  The per-token distributions come from the predict_fn chain
// (ll_gather_rows -> launch_gemm<EPI_BIAS> -> ll_softmax_rows, kernels_ll.h), one row per distinct token of a chunk;
// everything below reads them in place, so the (T, V_e) distributions never leave the device.  The joint rows are ranked by
// topk_rows<true> (kernels_score.h) or by the full-ranking kernels in their RAW form (kernels_rank.h).
//
// Every float32 value here keeps its denormals (HIP's default on gfx950: .amdhsa_float_denorm_mode_32 = 3) and the
// transcendental calls are the full-precision logf / expf, so a joint in the denormal range is the small number the
// host computes, not a flushed zero.
#pragma once
#include "common.h"

namespace sert {

enum { kLLRankDevice = 0, kLLRankHost = 1 };     // per-query status (include/sert_hip.h: SERT_LL_STATUS_*)

// ---- the host's float32 sums, in the host's order ------------------------------------------------------------------
// The scores and entropies the reference reports are float32 NumPy / SciPy results (joint.sum(), scipy.stats.entropy
// on float32 arrays).  Near a one-hot distribution the entropy is ill-conditioned in float32: -q log q of a q next to 1
// keeps about one ulp of 1, so an entropy summed in another order or precision differs from the host's by far more than
// rounding of the result.  These sums therefore follow NumPy's float32 add.reduce of a contiguous vector exactly:
// chunks of 8192 elements (the ufunc buffer) added in order to 0, each chunk by pairwise_sum -- blocks of at most 128
// elements summed with 8 accumulators, larger ranges halved at a multiple of 8.  (A fixed-order tree: deterministic.)
constexpr int kNpBuf = 8192, kNpBlock = 128;

template <typename F>
__device__ float np_leaf_sum(const F& f, int off, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += f(off + i);
        return r;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = f(off + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += f(off + i + j);
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += f(off + i);
    return res;
}

// Walk of one chunk's pairwise_sum tree (m <= 8192 elements from c0): visit(leaf index, offset, length) for every leaf
// in order -- pre-order, left first.  A chunk has at most 128 leaves (every leaf of a split range holds >= 64).
template <typename V_>
__device__ __forceinline__ void np_leaves(int c0, int m, const V_& visit) {
    int so[16], sn[16], sp = 1, li = 0;
    so[0] = c0; sn[0] = m;
    while (sp) {
        --sp;
        const int o = so[sp], k = sn[sp];
        if (k <= kNpBlock) { visit(li++, o, k); continue; }
        int h = k / 2;
        h -= h % 8;
        so[sp] = o + h; sn[sp] = k - h; ++sp;
        so[sp] = o; sn[sp] = h; ++sp;
    }
}

// pairwise_sum's additions over one chunk's leaf sums: left + right at every split (post-order walk)
__device__ __forceinline__ float np_combine(int m, const float* leaf) {
    int so[16], sn[16], ss[16], sp = 1, vp = 0, li = 0;
    float vs[16];
    so[0] = 0; sn[0] = m; ss[0] = 0;
    while (sp) {
        const int t = sp - 1, o = so[t], k = sn[t];
        if (k <= kNpBlock) { vs[vp++] = leaf[li++]; --sp; continue; }
        int h = k / 2;
        h -= h % 8;
        if (ss[t] == 0)      { ss[t] = 1; so[sp] = o; sn[sp] = h; ss[sp] = 0; ++sp; }
        else if (ss[t] == 1) { ss[t] = 2; so[sp] = o + h; sn[sp] = k - h; ss[sp] = 0; ++sp; }
        else { const float b = vs[--vp], a = vs[--vp]; vs[vp++] = a + b; --sp; }
    }
    return vs[0];
}

constexpr int kNpGroup = 16;   // chunks summed side by side: 16 threads per chunk

// sum_{i < n} f(i) in NumPy's order, 256-thread workgroup (every thread calls it; result in every thread).
// leaf: kNpGroup * kNpBlock floats of LDS, csum: kNpGroup floats.  Up to 16 chunks at a time: the 16 threads of a chunk
// sum its leaves, one thread per chunk combines them, and the chunk sums are added in order.
template <typename F>
__device__ float np_sum_f32(int n, const F& f, float* leaf, float* csum, float* bcast) {
    const int tid = threadIdx.x, mine = tid / kNpGroup, lane = tid % kNpGroup;
    float total = 0.f;
    for (int g0 = 0; g0 < n; g0 += kNpGroup * kNpBuf) {
        const int c0 = g0 + mine * kNpBuf;
        const int m = c0 < n ? min(kNpBuf, n - c0) : 0;
        if (m > 0)
            np_leaves(c0, m, [&](int li, int o, int k) {
                if (li % kNpGroup == lane) leaf[mine * kNpBlock + li] = np_leaf_sum(f, o, k);
            });
        __syncthreads();
        if (lane == 0 && m > 0) csum[mine] = np_combine(m, leaf + mine * kNpBlock);
        __syncthreads();
        if (tid == 0)
            for (int c = 0; c < kNpGroup && g0 + c * kNpBuf < n; ++c) total = total + csum[c];
        __syncthreads();
    }
    if (tid == 0) *bcast = total;
    __syncthreads();
    const float r = *bcast;
    __syncthreads();
    return r;
}

// scipy.special.entr on float32: -x log x evaluated in double, rounded to float; entr(0) = 0
__device__ __forceinline__ float entr_f32(float x) {
    const double d = (double)x;
    return d > 0.0 ? (float)(-d * log(d)) : (d == 0.0 ? 0.f : -INFINITY);
}

// math_utils.entropy(row, base=2, normalize=True) of a float32 row, as the host computes it (scipy.stats.entropy):
// pk = row / sum(row), S = sum(entr(pk)), S / float(ln 2), then / float(log2 V) -- ln2_f = float(log(2)),
// log2v_f = float(log(V) / log(2)), both from the host's libm.  Every float32 operation is the host's, in its order.
__device__ float np_entropy_norm2(const float* row, int V, float ln2_f, float log2v_f, float* leaf, float* csum,
                                  float* bcast) {
    const float s1 = np_sum_f32(V, [&](int e) { return row[e]; }, leaf, csum, bcast);
    const float h = np_sum_f32(V, [&](int e) { return entr_f32(row[e] / s1); }, leaf, csum, bcast);
    return (h / ln2_f) / log2v_f;
}

// Normalised base-2 entropy of every row of P (rows, V): scipy.stats.entropy semantics (math_utils.entropy) -- the row
// is renormalised first, 0 log 0 = 0 -- divided by log2(V).  One workgroup per row.
__global__ __launch_bounds__(256) void ll_row_entropy(const float* __restrict__ P, int V, float ln2_f, float log2v_f,
                                                      float* __restrict__ H) {
    __shared__ float leaf[kNpGroup * kNpBlock];
    __shared__ float csum[kNpGroup];
    __shared__ float bcast;
    const float h = np_entropy_norm2(P + (size_t)blockIdx.x * V, V, ln2_f, log2v_f, leaf, csum, &bcast);
    if (threadIdx.x == 0) H[blockIdx.x] = h;
}

// One workgroup per query q, tokens [offs[q], offs[q+1]) of the chunk, tok_row[t] = the token's row of P:
//   L_e = sum_t (p_te > 0 ? logf(p_te) : 0), tokens in query order     (np.ma.log(...).filled(0).sum(axis=0))
//   j_e = expf(L_e);  S = sum_e j_e (joint.sum(): NumPy's order);  J_e = j_e / S   (joint /= joint.sum())
//   joint_h = math_utils.entropy(J, base=2, normalize=True)
// status = host when S is 0 or not finite -- the queries for which the host's `joint /= joint.sum()` gives NaN; their
// J row is zeroed (the caller re-runs them on the host path).
__global__ __launch_bounds__(256) void ll_query_aggregate(const float* __restrict__ P, const int32_t* __restrict__ tok_row,
                                                          const int64_t* __restrict__ offs, int V, float ln2_f,
                                                          float log2v_f, float* __restrict__ J,
                                                          float* __restrict__ joint_h, int32_t* __restrict__ status) {
    __shared__ float leaf[kNpGroup * kNpBlock];
    __shared__ float csum[kNpGroup];
    __shared__ float bcast;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = offs[q], t1 = offs[q + 1];
    float* Jq = J + (size_t)q * V;
    for (int e = tid; e < V; e += 256) {
        float L = 0.f;
        for (int64_t t = t0; t < t1; ++t) {
            const float p = P[(size_t)tok_row[t] * V + e];
            L += p > 0.f ? logf(p) : 0.f;
        }
        Jq[e] = expf(L);
    }
    __syncthreads();
    const float S = np_sum_f32(V, [&](int e) { return Jq[e]; }, leaf, csum, &bcast);
    const bool host = !(S > 0.f) || !isfinite(S);
    if (host) {
        for (int e = tid; e < V; e += 256) Jq[e] = 0.f;
        if (tid == 0) { status[q] = kLLRankHost; joint_h[q] = NAN; }
        return;
    }
    for (int e = tid; e < V; e += 256) Jq[e] = Jq[e] / S;
    __syncthreads();
    const float h = np_entropy_norm2(Jq, V, ln2_f, log2v_f, leaf, csum, &bcast);
    if (tid == 0) { status[q] = kLLRankDevice; joint_h[q] = h; }
}

}  // namespace sert
