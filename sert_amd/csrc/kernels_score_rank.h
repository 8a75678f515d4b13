// Full rankings of the cosine scorer (include/sert_hip.h: sert_scorer_rank; k = -1 or k > 1024), gfx950.  The slab S holds
// the cosines sert_scorer_cosines returns; the kernels below order every row of it under the scorer's one order (DESIGN.md,
// "One ranking order": cosine descending, -0 equal to +0, a NaN of either sign after every number, ties and the NaNs among
// themselves by lowest entity index) and emit (entity, (cos + 1) / 2) -- the score from the slab's cosine, AFTER the ordering.
// They are the loglinear ranker's two sorts (kernels_ll_rank.h) on score_key instead of desc_key; the query-index keys of the
// LSD form are that ranker's ll_query_keys.
#pragma once
#include "common.h"

namespace sert {

// Full ranking of one row of S (V <= N) in LDS: N 64-bit words (score_key(cos) << 32 | entity), bitonic sort, the first kk
// written.  The ~0 padding sorts after a NaN's word, whose low half is an entity index.  N = 8192 is 64 KiB of LDS (two
// workgroups per CU).
template <int N>
__global__ __launch_bounds__(256) void score_rank_lds(const float* __restrict__ S, int V, int kk, int32_t* __restrict__ idx_out,
                                                      float* __restrict__ val_out) {
    __shared__ unsigned long long keys[N];
    const int tid = threadIdx.x;
    const float* row = S + (size_t)blockIdx.x * V;
    int sort_n = 2;
    while (sort_n < V) sort_n <<= 1;
    for (int i = tid; i < sort_n; i += 256)
        keys[i] = i < V ? ((unsigned long long)score_key(row[i]) << 32) | (uint32_t)i : ~0ull;
    __syncthreads();
    for (int size = 2; size <= sort_n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < sort_n / 2; i += 256) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < kk; i += 256) {
        const uint32_t e = (uint32_t)keys[i];
        idx_out[(size_t)blockIdx.x * kk + i] = (int32_t)e;
        val_out[(size_t)blockIdx.x * kk + i] = (row[e] + 1.0f) / 2.0f;      // (cos_to_score's two operations; NaN stays NaN)
    }
}

// Above kLLRankLdsMax entities, the LSD passes of kernels_sort.h: the 32-bit score key of every (query, entity) element ...
__global__ void score_rank_keys(const float* __restrict__ S, int n, int32_t* __restrict__ keys) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = (int32_t)score_key(S[i]);
}
// ... and after them (query q's elements at [q V, (q+1) V) in ranking order, vals = flat indices q V + e) its first kk as
// (entity, (cos + 1) / 2)
__global__ void score_rank_emit(const int32_t* __restrict__ vals, const float* __restrict__ S, int Q, int V, int kk,
                                int32_t* __restrict__ idx_out, float* __restrict__ val_out) {
    const size_t total = (size_t)Q * kk;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t q = t / kk, i = t - q * kk;
        const int32_t v = vals[q * V + i];
        idx_out[t] = v - (int32_t)(q * V);
        val_out[t] = (S[v] + 1.0f) / 2.0f;
    }
}

}  // namespace sert
