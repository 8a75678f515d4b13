// Re-ranking per-query candidate lists with the loglinear model, gfx950 (include/sert_hip.h: sert_ll_rank_candidates;
// host/api_ll_rerank.inc).  Everything in front of the joint rows J (Qc, V_e) is the chain of sert_ll_rank_queries
// (kernels_ll_rank.h: the partition function is over ALL entities, so J stays V_e wide); the kernels here only decide what of
// a joint row is sorted and written out.  The candidates are CSR, chunk-relative: query q of the chunk owns
// ents[indptr[q] .. indptr[q + 1]), strictly ascending, and writes its kk = out_ptr[q + 1] - out_ptr[q] best at out_ptr[q].
//
// One key, one emitted value: rank_key<true> (desc_key) of J[q, e] orders a list and key_to_float gives the score back, as
// rank_rows_lds<N, true> does for the whole row -- so a list's ranking is the full ranking restricted to the list, same score
// bits, by construction.
//   ll_rerank_lds<N>       lists of 1 .. kRankLdsMax candidates: one workgroup per query, (key << 32 | entity) words in LDS,
//                          bitonic_sort_lds, the head emitted.  Ascending lists: the entity in the low word breaks ties by index.
//   ll_rerank_gather_slab  longer lists: J[q, list] into a (rows, lmax) slab, -inf behind every list (a DEVICE query's joints
//                          are finite and >= 0, a HOST query's row is zero: the padding ranks last under desc_key); the slab's
//                          rows go through the counting-sort passes of kernels_rank.h (RAW) as POSITIONS, and rerank_compact
//                          (kernels_rerank.h, shared with the cosine re-ranker) maps them to entities in the ragged output.
// The reads of J are scattered 4-byte loads inside one row (V_e floats: 400 kB at V_e = 100 000, resident in L2 right behind
// ll_query_aggregate, which wrote it); ascending entities keep neighbouring lanes in neighbouring cache lines.
#pragma once
#include "common.h"
#include "kernels_rank.h"
#include "kernels_rerank.h"

namespace sert {

// One workgroup per query of qlist, each with 1 .. N candidates.  N = 8192 is rank_rows_lds<8192>'s 64 KiB of LDS.
template <int N>
__global__ __launch_bounds__(256) void ll_rerank_lds(const float* __restrict__ J, int V, const int32_t* __restrict__ ents,
                                                     const int64_t* __restrict__ indptr, const int64_t* __restrict__ out_ptr,
                                                     const int32_t* __restrict__ qlist, int32_t* __restrict__ idx_out,
                                                     float* __restrict__ val_out) {
    __shared__ unsigned long long keys[N];
    const int tid = threadIdx.x;
    const int q = qlist[blockIdx.x];
    const int64_t b = indptr[q];
    const int m = (int)(indptr[q + 1] - b);
    const int64_t o = out_ptr[q];
    const int kk = (int)(out_ptr[q + 1] - o);
    const float* row = J + (size_t)q * V;
    int sort_n = 2;
    while (sort_n < m) sort_n <<= 1;
    for (int i = tid; i < sort_n; i += 256) {
        unsigned long long w = ~0ull;                 // (the padding sorts behind every word: a real one's low half is an entity)
        if (i < m) {
            const uint32_t e = (uint32_t)ents[b + i];
            w = ((unsigned long long)rank_key<true>(row[e]) << 32) | e;
        }
        keys[i] = w;
    }
    __syncthreads();
    bitonic_sort_lds(keys, sort_n);
    for (int i = tid; i < kk; i += 256) {
        const unsigned long long kv = keys[i];
        idx_out[o + i] = (int32_t)(uint32_t)kv;
        val_out[o + i] = key_to_float((uint32_t)(kv >> 32));
    }
}

// slab (rows, lmax): row r = the joints of query row_query[r] at its candidates, in list order, -inf behind them
__global__ void ll_rerank_gather_slab(const float* __restrict__ J, int V, const int32_t* __restrict__ ents,
                                      const int64_t* __restrict__ indptr, const int32_t* __restrict__ row_query, int rows,
                                      int lmax, float* __restrict__ slab) {
    const size_t total = (size_t)rows * lmax;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t r = t / lmax;
        const int64_t i = (int64_t)(t - r * lmax);
        const int q = row_query[r];
        const int64_t b = indptr[q];
        slab[t] = i < indptr[q + 1] - b ? J[(size_t)q * V + ents[b + i]] : -INFINITY;
    }
}

}  // namespace sert
