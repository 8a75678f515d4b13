// Retrieval evaluation on the device (include/sert_hip.h: sert_reval_*): the two kernels the evaluator adds to the
// existing projection / scoring / ranking paths.
//   reval_gather_mean  ragged gather + mean of the topics' word rows (the query side of sert/inference.py:161-167)
//   reval_metrics      NDCG / MAP / reciprocal rank / P@5 / relevant-retrieved of every topic's ranking
#pragma once
#include "common.h"
#include "sert_hip.h"

namespace sert {

// metrics_out columns of sert_reval_run: the public enum (include/sert_hip.h)
enum { REVAL_NDCG = SERT_REVAL_NDCG, REVAL_MAP = SERT_REVAL_MAP, REVAL_RECIP_RANK = SERT_REVAL_RECIP_RANK, REVAL_P5 = SERT_REVAL_P5,
       REVAL_NUM_REL_RET = SERT_REVAL_NUM_REL_RET, REVAL_NUM_METRICS = SERT_REVAL_NUM_METRICS };

// avg[q] = (sum_t R_w[tok_t]) / T: one wave per topic, a lane owns VEC consecutive columns at a time.  The rows are added
// IN TOKEN ORDER starting from the first row (fp32 adds cannot contract into FMAs), then ONE correctly rounded division by
// (float)T -- bit for bit numpy's R_w[tokens, :].mean(axis=0), which reduces axis 0 of a C-ordered block row by row and
// divides once.  So the projections, and with them the ranking, are those of the host query path.
// Every token id is < vocab_size and every topic has at least one token (validated by sert_reval_create).
template <int VEC>
__global__ void __launch_bounds__(256) reval_gather_mean(const int32_t* __restrict__ tokens, const int64_t* __restrict__ offsets,
                                                         const float* __restrict__ Rw, int Q, int d, float* __restrict__ avg) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int lane = threadIdx.x & 63;
    const int64_t t0 = offsets[q], t1 = offsets[q + 1];
    const float T = (float)(t1 - t0);
    for (int c = lane * VEC; c < d; c += 64 * VEC) {
        float acc[VEC];
        const float* row = Rw + (size_t)tokens[t0] * d + c;
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = row[v];
        for (int64_t t = t0 + 1; t < t1; ++t) {
            row = Rw + (size_t)tokens[t] * d + c;
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = __fadd_rn(acc[v], row[v]);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) avg[(size_t)q * d + c + v] = __fdiv_rn(acc[v], T);
    }
}

__device__ __forceinline__ double reval_wave_sum(double v) {
    // xor butterfly: the same association on every call, so the figures do not depend on the launch
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per topic walks the topic's ranking idx[q][0 .. kk) in chunks of 64 ranks.  Each lane looks its entity up in the
// topic's judgement list (entity indices ascending: binary search); gains and hit flags are combined across the wave (ballot
// + popcount for the running number of hits, carried from chunk to chunk) and accumulated in float64:
//   ndcg        sum_i gain_i / log2(i + 1) over the kk ranks (i from 1; log2tab[i] = log2(i + 1), float64, from the host),
//               over the topic's ideal DCG (host, float64: it also counts judged entities the model does not know); 0 if that is 0
//   map         sum over the hits of hits_i / i, over num_rel (host; as above); 0 if num_rel is 0
//   recip_rank  1 / rank of the first hit, 0 without one;   P_5  hits among the first five ranks / 5;   num_rel_ret  hits
// A hit is a judged entity with gain > 0.  Topics q0 .. q0 + Qc of the judgement arrays, rows 0 .. Qc of idx.
__global__ void __launch_bounds__(256) reval_metrics(const int32_t* __restrict__ idx, int kk, int Qc, int64_t q0,
                                                     const int64_t* __restrict__ rel_indptr, const int32_t* __restrict__ rel_ent,
                                                     const float* __restrict__ rel_gain, const double* __restrict__ log2tab,
                                                     const double* __restrict__ idcg, const int32_t* __restrict__ num_rel,
                                                     double* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Qc) return;
    const int lane = threadIdx.x & 63;
    const int64_t q = q0 + row;
    const int64_t lo0 = rel_indptr[q], hi0 = rel_indptr[q + 1];
    const int32_t* ranking = idx + (size_t)row * kk;
    double dcg = 0.0, ap = 0.0, rr = 0.0, p5 = 0.0;
    long long hits = 0;
    for (int base = 0; base < kk; base += 64) {
        const int r = base + lane;
        float gain = 0.f;
        if (r < kk) {
            const int32_t e = ranking[r];
            int64_t lo = lo0, hi = hi0;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (rel_ent[mid] < e) lo = mid + 1; else hi = mid;
            }
            if (lo < hi0 && rel_ent[lo] == e) gain = rel_gain[lo];
        }
        const bool hit = gain > 0.f;
        const unsigned long long mask = __ballot(hit);
        const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        const long long hits_here = hits + __popcll(mask & upto);
        const double i = (double)(r + 1);
        dcg += reval_wave_sum(r < kk ? (double)gain / log2tab[r + 1] : 0.0);
        ap += reval_wave_sum(hit ? (double)hits_here / i : 0.0);
        if (rr == 0.0 && mask != 0ull) rr = 1.0 / (double)(base + __ffsll((long long)mask));
        if (base == 0) p5 = (double)__popcll(mask & 31ull) / 5.0;
        hits += __popcll(mask);
    }
    if (lane == 0) {
        double* o = out + (size_t)q * REVAL_NUM_METRICS;
        const double ideal = idcg[q];
        const int32_t nr = num_rel[q];
        o[REVAL_NDCG] = ideal > 0.0 ? dcg / ideal : 0.0;
        o[REVAL_MAP] = nr > 0 ? ap / (double)nr : 0.0;
        o[REVAL_RECIP_RANK] = rr;
        o[REVAL_P5] = p5;
        o[REVAL_NUM_REL_RET] = (double)hits;
    }
}

}  // namespace sert
