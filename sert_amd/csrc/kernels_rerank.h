// Re-ranking: cosines and rankings of per-query candidate lists, gfx950 (include/sert_hip.h: sert_scorer_pairs,
// sert_scorer_rank_candidates; host/api_scorer_rerank.inc, and for the rankings the host chain of host/rank_lists.inc).  The
// candidates are CSR: query q owns cand_entities[indptr[q] .. indptr[q + 1]).  The ranker's arrays are chunk-relative: its
// kernels see the queries, the candidates and the output offsets of one chunk, counted from that chunk's first query.
//
// One arithmetic: every pair's cosine is exact_dot32_any (kernels_score_bf16.h) of the normalised query row and the normalised
// table row -- whatever the table size, whichever kernel below computes it.
//   rerank_pair_cosines   one 32-lane half-wave per pair, the work flattened over PAIRS (uneven lists do not unbalance it),
//                         four pairs per half-wave and trip so that four table rows are in flight together.  It is
//                         sert_scorer_pairs, and (SLAB) it fills the padded cosine slab of the lists too long for LDS.
//   rerank_lds<N>         lists of up to kRankLdsMax candidates: one workgroup per query; rescore_sort_emit scores the list
//                         into (score_key << 32 | entity) words in LDS, sorts them and emits the head.  The lists are strictly
//                         ascending, so the entity in the low word breaks ties as the position in the list would.
//   rerank_compact        longer lists: the slab's rows ordered by the counting-sort passes of kernels_rank.h (positions in the
//                         list), mapped back to entities and packed into the ragged output.
//
// The loglinear re-ranker (kernels_ll_rerank.h) runs through the same host chain and shares rerank_compact, but keeps its own
// score-producing kernels, ll_rerank_lds<N> and ll_rerank_gather_slab, beside rerank_lds<N> and rerank_pair_cosines<true>:
// these compute exact dot products with half-waves, those gather from a joint row that already exists.  That difference is
// real; one kernel for both would be a switch around two bodies.
//
// The pair -> query map is a search in indptr, not an uploaded int32 per pair: the map would double the bytes a call sends to
// the device (the candidates themselves are 4 bytes per pair), and at 10 000 x 1 000 pairs that upload costs more than the
// kernel.  The search is one bisection per half-wave (log2 Q reads of an array that stays in L2, every lane the same
// address) at the start of its contiguous run of pairs; every later pair walks on from the row of the one before.
#pragma once
#include "common.h"
#include "kernels_rank.h"
#include "kernels_score_bf16.h"

namespace sert {

constexpr int kRerankPairsPerTrip = 4;                       // table rows in flight per half-wave
constexpr int kRerankTile = 8 * kRerankPairsPerTrip;          // pairs per workgroup and trip

// Work items [j0, j1) of rows r = 0 .. R - 1, row r owning the items [wptr[r], wptr[r + 1]) (wptr[0] <= j0, j1 <= wptr[R]).
// Item j of row r is the pair (query, cand_entities[indptr[query] + j - wptr[r]]), query = row_query ? row_query[r] : r;
// `ents` holds the caller's cand_entities from element ent_base on (sert_scorer_pairs cuts its chunks inside a list; the
// slab form's arrays are chunk-relative and its ent_base is 0).
//   !SLAB  out[j - j0] = the cosine (raw) or (cos + 1) / 2          (sert_scorer_pairs: wptr == indptr)
//    SLAB  out[r * stride + j - wptr[r]] = the cosine              (the padding behind a row's list is the caller's)
template <bool SLAB>
__global__ __launch_bounds__(256) void rerank_pair_cosines(const float* __restrict__ P, const float* __restrict__ E, int d,
                                                           const int32_t* __restrict__ ents, int64_t ent_base,
                                                           const int64_t* __restrict__ indptr, const int64_t* __restrict__ wptr,
                                                           int R, const int32_t* __restrict__ row_query, int64_t j0, int64_t j1,
                                                           float* __restrict__ out, int64_t stride, int raw) {
    const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
    // every half-wave owns one contiguous run of items: the bisection is paid once per half-wave, not once per trip (inside
    // the loop it was a chain of log2 R dependent reads in front of every four row fetches: 1.98 ms instead of 1.10 at
    // 10 000 x 1 000 pairs)
    const int64_t per = ((j1 - j0 + (int64_t)gridDim.x * 8 - 1) / ((int64_t)gridDim.x * 8) + kRerankPairsPerTrip - 1) /
                        kRerankPairsPerTrip * kRerankPairsPerTrip;
    int64_t t = j0 + ((int64_t)blockIdx.x * 8 + half) * per;
    const int64_t tend = min(j1, t + per);
    if (t >= tend) return;
    // the row of item t: the last r with wptr[r] <= t (empty rows behind it share its start and are passed over)
    int lo = 0, hi = R;                           // wptr[lo] <= t < wptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wptr[mid] <= t) lo = mid; else hi = mid;
    }
    int r = lo;
    int64_t rbeg = wptr[r], rend = wptr[r + 1];
    for (; t < tend; t += kRerankPairsPerTrip) {
        const float* prow[kRerankPairsPerTrip];
        const float* erow[kRerankPairsPerTrip];
        int64_t at[kRerankPairsPerTrip];
#pragma unroll
        for (int j = 0; j < kRerankPairsPerTrip; ++j) {
            const int64_t tj = min(t + j, tend - 1);        // (a clamped item repeats the last one and is not stored)
            while (tj >= rend) { ++r; rbeg = rend; rend = wptr[r + 1]; }      // (tj < j1 <= wptr[R]: r stays below R)
            const int q = row_query ? row_query[r] : r;
            const int32_t e = ents[indptr[q] + (tj - rbeg) - ent_base];
            prow[j] = P + (size_t)q * d;
            erow[j] = E + (size_t)e * d;
            at[j] = SLAB ? (int64_t)r * stride + (tj - rbeg) : tj - j0;
        }
        float sc[kRerankPairsPerTrip];
        if (d == 128) {
            float4 x[kRerankPairsPerTrip], y[kRerankPairsPerTrip];
#pragma unroll
            for (int j = 0; j < kRerankPairsPerTrip; ++j) {
                x[j] = *reinterpret_cast<const float4*>(prow[j] + 4 * l);
                y[j] = *reinterpret_cast<const float4*>(erow[j] + 4 * l);
            }
#pragma unroll
            for (int j = 0; j < kRerankPairsPerTrip; ++j) {     // same arithmetic as exact_dot32 at d = 128
                float a = fmaf(x[j].x, y[j].x, 0.f);
                a = fmaf(x[j].y, y[j].y, a); a = fmaf(x[j].z, y[j].z, a); a = fmaf(x[j].w, y[j].w, a);
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
                sc[j] = a;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kRerankPairsPerTrip; ++j) sc[j] = exact_dot32_any(prow[j], erow[j], d, l);
        }
        if (l == 0) {
#pragma unroll
            for (int j = 0; j < kRerankPairsPerTrip; ++j)
                if (t + j < tend) out[at[j]] = (SLAB || raw) ? sc[j] : (sc[j] + 1.0f) / 2.0f;
        }
    }
}

// One workgroup per query of qlist, each with 1 .. N candidates: the kk = out_ptr[q + 1] - out_ptr[q] best of the list to
// idx_out / val_out at out_ptr[q].  N = 8192 is rank_rows_lds<8192>'s 64 KiB of LDS.
template <int N>
__global__ __launch_bounds__(256) void rerank_lds(const float* __restrict__ P, const float* __restrict__ E, int d,
                                                  const int32_t* __restrict__ ents, const int64_t* __restrict__ indptr,
                                                  const int64_t* __restrict__ out_ptr, const int32_t* __restrict__ qlist,
                                                  int32_t* __restrict__ idx_out, float* __restrict__ val_out) {
    __shared__ unsigned long long keys[N];
    const int q = qlist[blockIdx.x];
    const int64_t b = indptr[q];
    const int m = (int)(indptr[q + 1] - b);
    const int kk = (int)(out_ptr[q + 1] - out_ptr[q]);
    for (int i = threadIdx.x; i < m; i += 256) keys[i] = (uint32_t)ents[b + i];
    __syncthreads();
    int sort_n = 2;
    while (sort_n < m) sort_n <<= 1;
    const int64_t o = out_ptr[q];
    rescore_sort_emit<true>(keys, m, sort_n, P + (size_t)q * d, E, d, kk, idx_out + o, val_out + o);
}

// Rows of the slab path after rank_rows_full: pos / val (rows, kkc) = each row's list positions in ranking order and their
// scores.  The first kk of row r, as entities, to the ragged output of its query.  Both re-rankers end their slab path here.
__global__ void rerank_compact(const int32_t* __restrict__ pos, const float* __restrict__ val, int rows, int kkc,
                               const int32_t* __restrict__ row_query, const int32_t* __restrict__ ents,
                               const int64_t* __restrict__ indptr, const int64_t* __restrict__ out_ptr,
                               int32_t* __restrict__ idx_out, float* __restrict__ val_out) {
    const size_t total = (size_t)rows * kkc;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t r = t / kkc, i = t - r * kkc;
        const int q = row_query[r];
        const int64_t o = out_ptr[q] + (int64_t)i;
        if (o >= out_ptr[q + 1]) continue;      // (beyond this query's ranked depth: padding, or a shorter list)
        idx_out[o] = ents[indptr[q] + pos[t]];
        val_out[o] = val[t];
    }
}

}  // namespace sert
