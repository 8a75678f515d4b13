// Retrieval evaluation on the device (include/sert_hip.h: sert_reval_*): the kernels the evaluator adds to the
// existing projection / scoring / ranking paths.
//   reval_gather_mean  ragged gather + mean of the topics' word rows (the query side of sert/inference.py:161-167)
//   reval_metrics      NDCG / MAP / reciprocal rank / P@5 / relevant-retrieved of every topic's ranking
//   reval_count_ranks  the ranks of a topic's judged entities by counting over its cosine row (no ranking is made)
//   reval_metrics_from_ranks  the same five figures from those ranks
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

// ---- evaluation at any depth without a sort (sert_reval_create_counted; DESIGN.md, "Evaluation depth without a sort") ----

// an entity's place in the scorer's order as one integer: score_key of its cosine above, its index below.  Ascending in
// this number IS the scorer's order (cosine descending, -0 with +0, NaN last, ties and NaNs by lowest entity index).
__device__ __forceinline__ unsigned long long reval_order_key(float cosine, uint32_t entity) {
    return ((unsigned long long)score_key(cosine) << 32) | entity;
}

__device__ __forceinline__ int reval_wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rank(q, e) = 1 + #{e' in [0, V): order_key(S[q][e'], e') < order_key(S[q][e], e)} for every judged entity e of the topics
// q0 .. q0 + gridDim.x, whose cosines are the rows of S (rows, V).  No sort, nothing of size V is written.
//   grid (rows, splits): block (row, sp) streams the sp-th piece of the row's columns.  TJ of the topic's judged entities at
//   a time (a tile): thread j < TJ fetches the j-th one's cosine and makes its order key, every thread takes the TJ keys into
//   registers (a key of 0 pads a short tile: no order key is below it) and compares each column it streams with all of them,
//   counting in TJ registers; a longer judgement list takes further passes over the piece (then from L2).  Four 16-byte
//   loads per thread are in flight where V % 4 == 0 (VEC; S is 16-byte aligned: then every row is), dwords otherwise.
//   The per-thread counts are summed over the wave, then in integer LDS counters over the workgroup, and added to ranks[]
//   with one integer atomic per (judged entity, piece); piece 0 also adds the 1.  The counts are integers: every order of
//   adding them gives the same rank.  ranks[] (aligned with rel_ent) must be ZERO on entry for the topics of the launch.
//   A topic without judged entities reads nothing and writes nothing.
template <int TJ, bool VEC>
__global__ void __launch_bounds__(256) reval_count_ranks(const float* __restrict__ S, int V, int64_t q0,
                                                         const int64_t* __restrict__ rel_indptr, const int32_t* __restrict__ rel_ent,
                                                         int32_t* __restrict__ ranks) {
    static_assert(TJ <= 64, "one thread per judged entity of a tile, one LDS counter each");
    const int row = blockIdx.x;
    const int64_t lo = rel_indptr[q0 + row], hi = rel_indptr[q0 + row + 1];
    if (lo >= hi) return;        // (the whole workgroup)
    const float* srow = S + (size_t)row * V;
    __shared__ unsigned long long skey[TJ];
    __shared__ int scnt[TJ];
    // this block's columns [c0, c1): whole float4s in the vector form
    constexpr int W = VEC ? 4 : 1;
    const int64_t units = V / W, per = (units + gridDim.y - 1) / gridDim.y;
    const int64_t u0 = per * blockIdx.y, u1 = per * (blockIdx.y + 1);
    const int c0 = (int)((u0 < units ? u0 : units) * W);
    const int c1 = (int)((u1 < units ? u1 : units) * W);
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr unsigned long long kNone = ~0ull;      // (a column past the piece: below no key)
    for (int64_t t0 = lo; t0 < hi; t0 += TJ) {
        const int jn = hi - t0 < TJ ? (int)(hi - t0) : TJ;
        __syncthreads();                             // (the previous tile's counters have been read)
        if (tid < TJ) {
            unsigned long long k = 0ull;
            if (tid < jn) {
                const int32_t e = rel_ent[t0 + tid];
                k = reval_order_key(srow[e], (uint32_t)e);
            }
            skey[tid] = k;
            scnt[tid] = 0;
        }
        __syncthreads();
        unsigned long long key[TJ];
        int cnt[TJ];
#pragma unroll
        for (int j = 0; j < TJ; ++j) { key[j] = skey[j]; cnt[j] = 0; }
        if constexpr (VEC) {
            for (int c = c0 + tid * 4; c < c1; c += 4 * 1024) {
                float4 v[4] = {};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c + u * 1024 < c1) v[u] = *reinterpret_cast<const float4*>(srow + c + u * 1024);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cc = c + u * 1024;
                    const bool in = cc < c1;
                    const unsigned long long k0 = in ? reval_order_key(v[u].x, (uint32_t)cc) : kNone;
                    const unsigned long long k1 = in ? reval_order_key(v[u].y, (uint32_t)cc + 1u) : kNone;
                    const unsigned long long k2 = in ? reval_order_key(v[u].z, (uint32_t)cc + 2u) : kNone;
                    const unsigned long long k3 = in ? reval_order_key(v[u].w, (uint32_t)cc + 3u) : kNone;
#pragma unroll
                    for (int j = 0; j < TJ; ++j)
                        cnt[j] += (int)(k0 < key[j]) + (int)(k1 < key[j]) + (int)(k2 < key[j]) + (int)(k3 < key[j]);
                }
            }
        } else {
            for (int c = c0 + tid; c < c1; c += 4 * 256) {
                float v[4] = {};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c + u * 256 < c1) v[u] = srow[c + u * 256];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cc = c + u * 256;
                    const unsigned long long k0 = cc < c1 ? reval_order_key(v[u], (uint32_t)cc) : kNone;
#pragma unroll
                    for (int j = 0; j < TJ; ++j) cnt[j] += (int)(k0 < key[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int total = reval_wave_sum_int(cnt[j]);
            if (lane == 0 && total != 0) atomicAdd(&scnt[j], total);
        }
        __syncthreads();
        if (tid < jn) {
            const int add = scnt[tid] + (blockIdx.y == 0 ? 1 : 0);
            if (add != 0) atomicAdd(&ranks[t0 + tid], add);
        }
    }
}

// The five columns of reval_metrics from the RANKS of a topic's judged entities (reval_count_ranks) instead of its ranking:
// one wave per topic, lane l takes the judged entities l, l + 64, ... of the topic's list.  With kk the depth, and only
// entities of rank <= kk counting:
//   ndcg        sum of (double)gain / log2tab[rank] (whatever the gain's sign, as reval_metrics adds it), over the ideal DCG; 0 if that is 0
//   map         sum over the hits (gain > 0) of h / rank, h = the topic's hits of rank <= this one's -- counted among the
//               hits, an integer -- over num_rel; 0 if that is 0
//   recip_rank  1 / the smallest rank of a hit, 0 without one;   P_5  hits of rank <= 5, over 5;   num_rel_ret  hits
// ORDER OF THE FLOAT64 SUMS: judgement-list order.  Each lane adds its terms in ascending list position starting from 0.0,
// then the 64 partial sums meet in the xor butterfly of reval_wave_sum (32, 16, ... 1).  The order depends on the topic's
// list alone -- not on the launch, the slab the topic fell into or the other topics.
// The hits of rank <= r are counted by a walk over the whole list per hit: J^2 steps for a list of J (a qrel set judges a
// handful of entities per topic).  Topics q0 .. q0 + Qc; ranks / rel_gain aligned with rel_ent.
__global__ void __launch_bounds__(256) reval_metrics_from_ranks(const int32_t* __restrict__ ranks, int kk, int Qc, int64_t q0,
                                                                const int64_t* __restrict__ rel_indptr,
                                                                const float* __restrict__ rel_gain, const double* __restrict__ log2tab,
                                                                const double* __restrict__ idcg, const int32_t* __restrict__ num_rel,
                                                                double* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Qc) return;
    const int lane = threadIdx.x & 63;
    const int64_t q = q0 + row;
    const int64_t lo = rel_indptr[q], hi = rel_indptr[q + 1];
    double dcg = 0.0, ap = 0.0;
    int hits = 0, top5 = 0, first = 0x7fffffff;
    for (int64_t j = lo + lane; j < hi; j += 64) {
        const int r = ranks[j];
        const float gain = rel_gain[j];
        if (r > kk) continue;
        dcg += (double)gain / log2tab[r];
        if (!(gain > 0.f)) continue;
        hits += 1;
        top5 += r <= 5 ? 1 : 0;
        first = min(first, r);
        int h = 0;
        for (int64_t i = lo; i < hi; ++i) h += (rel_gain[i] > 0.f && ranks[i] <= r) ? 1 : 0;
        ap += (double)h / (double)r;
    }
    dcg = reval_wave_sum(dcg);
    ap = reval_wave_sum(ap);
    hits = reval_wave_sum_int(hits);
    top5 = reval_wave_sum_int(top5);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (lane == 0) {
        double* o = out + (size_t)q * REVAL_NUM_METRICS;
        const double ideal = idcg[q];
        const int32_t nr = num_rel[q];
        o[REVAL_NDCG] = ideal > 0.0 ? dcg / ideal : 0.0;
        o[REVAL_MAP] = nr > 0 ? ap / (double)nr : 0.0;
        o[REVAL_RECIP_RANK] = first != 0x7fffffff ? 1.0 / (double)first : 0.0;
        o[REVAL_P5] = (double)top5 / 5.0;
        o[REVAL_NUM_REL_RET] = (double)hits;
    }
}

}  // namespace sert
