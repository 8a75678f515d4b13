// Full rankings of the rows of a (queries, V) matrix, gfx950: one set of kernels for the two rankers that order every entity
// of a query -- the cosine scorer (include/sert_hip.h: sert_scorer_rank, k = -1 or k > 1024; host/api_scorer_rank.inc) and the
// loglinear query ranker (sert_ll_rank_queries, sert_reval_run; host/api_ll_rank.inc).  As topk_rows<RAW> (kernels_score.h),
// the two differ only in the key and in the emitted value:
//   RAW          rows of joint scores: desc_key (score descending), the score itself emitted;
//   scorer form  rows of cosines under the scorer's one order ("One ranking order": cosine descending, -0 equal to
//                +0, a NaN of either sign after every number): score_key, (cos + 1) / 2 emitted -- from the row's cosine,
//                AFTER the ordering.
// Ties (and the scorer's NaNs among themselves) go by lowest entity index in both.  The host chain is host/rank_rows.inc.
#pragma once
#include "common.h"
#include "kernels_sort.h"

namespace sert {

constexpr int kRankLdsMax = 8192;               // V up to this: the whole ranking sorted in one workgroup's LDS

// Ascending bitonic sort of keys[0, sort_n) in LDS by a 256-thread workgroup: sort_n a power of two >= 2, the words already
// written and a barrier behind them.  (The sort of rank_rows_lds; ll_rerank_lds, kernels_ll_rerank.h, sorts through it too.)
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* keys, int sort_n) {
    const int tid = threadIdx.x;
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
}

// Full ranking of one row of S (V <= N) in LDS: N 64-bit words (rank_key(x) << 32 | entity), bitonic sort, the first kk
// written.  The ~0 padding sorts after a NaN's word, whose low half is an entity index.  N = 8192 is 64 KiB of LDS (two
// workgroups per CU).  RAW gives the score back from the key (desc_key is a bijection on bit patterns).
template <int N, bool RAW>
__global__ __launch_bounds__(256) void rank_rows_lds(const float* __restrict__ S, int V, int kk, int32_t* __restrict__ idx_out,
                                                     float* __restrict__ val_out) {
    __shared__ unsigned long long keys[N];
    const int tid = threadIdx.x;
    const float* row = S + (size_t)blockIdx.x * V;
    int sort_n = 2;
    while (sort_n < V) sort_n <<= 1;
    for (int i = tid; i < sort_n; i += 256)
        keys[i] = i < V ? ((unsigned long long)rank_key<RAW>(row[i]) << 32) | (uint32_t)i : ~0ull;
    __syncthreads();
    bitonic_sort_lds(keys, sort_n);
    for (int i = tid; i < kk; i += 256) {
        const unsigned long long kv = keys[i];
        const uint32_t e = (uint32_t)kv;
        idx_out[(size_t)blockIdx.x * kk + i] = (int32_t)e;
        if constexpr (RAW) val_out[(size_t)blockIdx.x * kk + i] = key_to_float((uint32_t)(kv >> 32));
        else val_out[(size_t)blockIdx.x * kk + i] = (row[e] + 1.0f) / 2.0f;      // (cos_to_score's two operations; NaN stays NaN)
    }
}

// Above kRankLdsMax entities, the LSD passes of kernels_sort.h:
//   the order-preserving 32-bit key of every (query, entity) element ...
template <bool RAW>
__global__ void rank_keys(const float* __restrict__ S, int n, int32_t* __restrict__ keys) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = (int32_t)rank_key<RAW>(S[i]);
}
//   ... then the query index of every element, read from its value (the flat index q V + e)
__global__ void rank_query_keys(const int32_t* __restrict__ vals, int n, int V, int32_t* __restrict__ keys) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = vals[i] / V;
}
// After the passes query q's elements sit at [q V, (q+1) V) in ranking order: its first kk as (entity, emitted value).
template <bool RAW>
__global__ void rank_emit(const int32_t* __restrict__ vals, const float* __restrict__ S, int Q, int V, int kk,
                          int32_t* __restrict__ idx_out, float* __restrict__ val_out) {
    const size_t total = (size_t)Q * kk;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t q = t / kk, i = t - q * kk;
        const int32_t v = vals[q * V + i];
        idx_out[t] = v - (int32_t)(q * V);
        val_out[t] = RAW ? S[v] : (S[v] + 1.0f) / 2.0f;
    }
}

// ---- host side: what one sorted chunk (the LSD passes) may hold and needs -------------------------------------------------
// Q queries of V entities fit one sorted chunk: the query index is one digit (kSortMaxBins), and the csort_* kernels and the
// grid-stride loops above index with int -- the margin keeps the last tile's indices and `i += gridDim.x * blockDim.x` (a
// stride of up to 2048 x 256) below 2^31 as well.
constexpr int64_t kRankMaxElems = ((int64_t)1 << 31) - ((int64_t)1 << 20);
inline bool rank_chunk_fits(int64_t Q, int64_t V) { return Q <= kSortMaxBins && Q * V <= kRankMaxElems; }

// Scratch of the LSD passes over n = Q V elements: four key / value arrays (ka | va | kb | vb, n each) in one allocation, and
// the histogram (kSortMaxBins x tiles) with the kSortMaxBins bin totals at its tail.  Grown on demand, never shrunk.
struct RankSortScratch {
    int32_t* keys = nullptr;
    int32_t* hist = nullptr;
    int64_t cap = 0;               // elements both hold room for
};
inline void rank_scratch_free(RankSortScratch& r) {      // (rank_scratch_reserve: host/rank_rows.inc)
    (void)hipFree(r.keys); (void)hipFree(r.hist);
    r = RankSortScratch();
}
inline int64_t rank_hist_ints(int64_t n) { return (int64_t)kSortMaxBins * cdiv(n, kSortTile) + kSortMaxBins; }
inline size_t rank_scratch_bytes(int64_t n) { return (size_t)n * 16 + (size_t)rank_hist_ints(n) * 4; }

}  // namespace sert
