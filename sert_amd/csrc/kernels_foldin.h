// Folding unseen entities into a trained vectorspace model (host/api_foldin.inc; DESIGN.md, "Folding in unseen
// entities"), gfx950.
//
// The word table, the projection and the V_e trained entity rows are FROZEN; only the N new rows E learn, with the NCE
// objective of the vectorspace step over the extended table Ext = concat(R_e, E) (new entity e is row V_e + e).  The
// projections T = tanh(h W + b) of the fold-in instances therefore never change: they are computed once, at upload, by the
// model's own forward (vs_gather_mean + the projection GEMM).  A step is
//   foldin_nce            the loss kernel's row body (kernels_vs.h: nce_rows16 / nce_rows_wave, the body of vs_nce /
//                         vs_nce_scalar) over a two-part table, WITHOUT the da it writes for the layers below (nothing
//                         below the projection learns); TRAIN leaves coef[i, j] and a KEY per pair: cand - V_e for a pair
//                         that hits a new row, the sentinel N for one that hits a frozen row
//   csort_pass            stable sort of the B (1 + z) (key, pair) entries (kernels_sort.h, as it is)
//   foldin_chunk_reduce   the body of egrad_chunk_reduce (kernels_egrad.h: chunk_reduce_rows) in the form that stops at the
//                         sentinel: the sentinel run -- most of the pairs -- is the END of the sorted order, so a chunk that
//                         starts inside it leaves after one load
//   egrad_fixup(_wg)      the carries of the runs that cross chunks, over the N new rows only (kernels_egrad.h, as it is)
// The three launches behind the loss kernel are the model's host chain (host/lazy_segsum.inc: EntityChain) over this
// handle's buffers.
//   adam_l2               Adam + L2 + sum of squares over E (kernels_opt.h, as it is), finalize_loss
// Order-fixed throughout, no floating-point atomic: a fold-in is bit-reproducible.
// A REFRESH handle (sert_foldin_create_refresh: trained rows that gained documents learn too) runs the same step with
// foldin_nce_map / foldin_nce_map_scalar in place of the loss kernel -- the trainable rows are slots found through a table --
// and N := the number of slots; see below.
#pragma once
#include "common.h"
#include "kernels_egrad.h"
#include "kernels_vs.h"

namespace sert {

// the row of Ext a candidate id names: frozen rows first, the new rows behind them
__device__ __forceinline__ const float* foldin_row(const float* __restrict__ Re, const float* __restrict__ E, int Ve, int e,
                                                   int de) {
    return e < Ve ? Re + (size_t)e * de : E + (size_t)(e - Ve) * de;
}

// The candidate policy (kernels_vs.h, nce_rows16) of the two-part table: the positive is new row y[i], a negative any row of
// Ext; the key of a pair is its new row, or the sentinel N for a frozen one.
struct FoldinTwoPart {
    const int32_t* __restrict__ yi;
    const int32_t* __restrict__ nrow;
    int Ve, e;
    __device__ __forceinline__ FoldinTwoPart(const int32_t* __restrict__ y, const int32_t* __restrict__ neg, int i, int z, int Ve_)
        : yi(y + i), nrow(neg + (size_t)i * z), Ve(Ve_), e(0) {}
    __device__ __forceinline__ void issue(int j) { e = (j == 0) ? Ve + *yi : nrow[j - 1]; }
    __device__ __forceinline__ void commit() {}
    __device__ __forceinline__ const float* row(const float* __restrict__ Re, const float* __restrict__ E, int de) const {
        return foldin_row(Re, E, Ve, e, de);
    }
    __device__ __forceinline__ int key(int N) const { return e >= Ve ? e - Ve : N; }
};

// vs_nce's row layout (nce_rows16): 16 lanes per instance, lane l owns the float4 column chunks l, l + 16, ...; one candidate
// after the other, so any z >= 1.  T: the (B, d_e) projections of THIS batch (the host passes the batch's first row).
//   u_j = <Ext[c_j], clip(t)>, s_j = clip(sigmoid(u_j)), loss = -(log s_0 + sum_{j>0} log(1 - s_j))
//   TRAIN: coef[i, j] = d loss / d u_j * w_i / B (inclusive clip mask), key[i, j] = c_j >= V_e ? c_j - V_e : N
//   rowloss[i] = (TRAIN ? w_i : 1) * loss; wg_loss[blockIdx.x] = the workgroup's sixteen row losses added in row order
template <int NCH, bool TRAIN>
__global__ __launch_bounds__(256) void foldin_nce(const float* __restrict__ T, const float* __restrict__ Re,
                                                  const float* __restrict__ E, const int32_t* __restrict__ y,
                                                  const int32_t* __restrict__ neg, const float* __restrict__ w,
                                                  float* __restrict__ coef, int32_t* __restrict__ key,
                                                  float* __restrict__ rowloss, int B, int z, int de, int Ve, int N,
                                                  float inv_batch, float* __restrict__ wg_loss) {
    const int i_raw = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = i_raw < B;
    const int i = valid ? i_raw : B - 1;
    nce_rows16<NCH, TRAIN, false>(T, Re, E, FoldinTwoPart(y, neg, i, z, Ve), w, nullptr, coef, key, rowloss, i, valid, z, de, N,
                                  inv_batch, wg_loss);
}

// Any d_e (d_e % 4 != 0), the way vs_nce_scalar covers it (nce_rows_wave): one wave per instance, scalar columns.
template <int NPL, bool TRAIN>
__global__ __launch_bounds__(256) void foldin_nce_scalar(const float* __restrict__ T, const float* __restrict__ Re,
                                                         const float* __restrict__ E, const int32_t* __restrict__ y,
                                                         const int32_t* __restrict__ neg, const float* __restrict__ w,
                                                         float* __restrict__ coef, int32_t* __restrict__ key,
                                                         float* __restrict__ rowloss, int B, int z, int de, int Ve, int N,
                                                         float inv_batch) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    nce_rows_wave<NPL, TRAIN, false>(T, Re, E, FoldinTwoPart(y, neg, i, z, Ve), w, nullptr, coef, key, rowloss, i, z, de, N,
                                     inv_batch);
}

// ---- a trainable table that is any subset of the extended table (sert_foldin_create_refresh) ----
// The N trainable rows E are SLOTS: refreshed trained rows first, new rows behind.  slot_of (V_e + num_new int32, built once
// at create) holds the slot of a row of the extended table, or -1 for a frozen one.  foldin_nce_map / foldin_nce_map_scalar are
// foldin_nce / foldin_nce_scalar with another candidate policy (FoldinAhead) -- how a candidate finds its row and key:
//   negative e:  s = slot_of[e]; row = s >= 0 ? E + s d_e : Re + e d_e; key = s >= 0 ? s : N
//   positive:    y[i] IS a slot: row = E + y[i] d_e, key = y[i] -- no lookup
// so the snapshot's stale copy of a refreshed row is never read.  The lookup is a dependent 4-byte load in front of the row
// fetch; z is a run-time value, so the lookups cannot all sit in registers ahead of the loop.  They run one candidate ahead
// instead: while candidate j's row is fetched, the slot of candidate j + 1 and the id of candidate j + 2 are already in
// flight (FoldinAhead; the reads past the last candidate are clamped onto it).  The arithmetic is the one row body's: with no
// refreshed row the two forms hold the same bits.

// the rows of E that are trained rows: E[s] = Re[ids[s]] (create only)
__global__ __launch_bounds__(256) void foldin_take_rows(const float* __restrict__ Re, const int32_t* __restrict__ ids,
                                                        float* __restrict__ E, int64_t rows, int de) {
    const int64_t total = rows * de;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = k / de;
        E[k] = Re[(size_t)ids[s] * de + (k - s * de)];
    }
}

// the candidates of one instance, looked up ahead of their use.  At the top of iteration j: s = the slot of candidate j (the
// positive's y for j = 0), e = its id (unused for j = 0), (e1, s1) = candidate j + 1, e2 = the id of candidate j + 2.
struct FoldinAhead {
    const int32_t* __restrict__ nrow;
    const int32_t* __restrict__ slot_of;
    int z, e, s, e1, s1, e2;
    __device__ __forceinline__ FoldinAhead(const int32_t* __restrict__ nrow_, const int32_t* __restrict__ slot_of_, int z_, int yi)
        : nrow(nrow_), slot_of(slot_of_), z(z_), e(0), s(yi) {
        e1 = nrow[0];                    // (z >= 1)
        e2 = nrow[min(1, z - 1)];
        s1 = slot_of[e1];
    }
    // issued in front of candidate j's row fetch; `commit` after the candidate's arithmetic
    int e3, s2;
    __device__ __forceinline__ void issue(int j) {
        e3 = nrow[min(j + 2, z - 1)];
        s2 = slot_of[e2];
    }
    __device__ __forceinline__ void commit() { e = e1; s = s1; e1 = e2; s1 = s2; e2 = e3; }
    __device__ __forceinline__ const float* row(const float* __restrict__ Re, const float* __restrict__ E, int de) const {
        return s >= 0 ? E + (size_t)s * de : Re + (size_t)e * de;
    }
    __device__ __forceinline__ int key(int N) const { return s >= 0 ? s : N; }
};

template <int NCH, bool TRAIN>
__global__ __launch_bounds__(256) void foldin_nce_map(const float* __restrict__ T, const float* __restrict__ Re,
                                                      const float* __restrict__ E, const int32_t* __restrict__ slot_of,
                                                      const int32_t* __restrict__ y, const int32_t* __restrict__ neg,
                                                      const float* __restrict__ w, float* __restrict__ coef,
                                                      int32_t* __restrict__ key, float* __restrict__ rowloss, int B, int z,
                                                      int de, int N, float inv_batch, float* __restrict__ wg_loss) {
    const int i_raw = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = i_raw < B;
    const int i = valid ? i_raw : B - 1;
    nce_rows16<NCH, TRAIN, false>(T, Re, E, FoldinAhead(neg + (size_t)i * z, slot_of, z, y[i]), w, nullptr, coef, key, rowloss, i,
                                  valid, z, de, N, inv_batch, wg_loss);
}

template <int NPL, bool TRAIN>
__global__ __launch_bounds__(256) void foldin_nce_map_scalar(const float* __restrict__ T, const float* __restrict__ Re,
                                                             const float* __restrict__ E, const int32_t* __restrict__ slot_of,
                                                             const int32_t* __restrict__ y, const int32_t* __restrict__ neg,
                                                             const float* __restrict__ w, float* __restrict__ coef,
                                                             int32_t* __restrict__ key, float* __restrict__ rowloss, int B,
                                                             int z, int de, int N, float inv_batch) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    nce_rows_wave<NPL, TRAIN, false>(T, Re, E, FoldinAhead(neg + (size_t)i * z, slot_of, z, y[i]), w, nullptr, coef, key, rowloss,
                                     i, z, de, N, inv_batch);
}

// egrad_chunk_reduce over keys sorted ascending whose LAST run is the sentinel (key == sentinel: a pair on a frozen row): the
// same body (kernels_egrad.h: chunk_reduce_rows, SENTINEL = true).  A chunk whose first key is the sentinel lies wholly inside
// that run and leaves after that one load; the chunk the run begins in reduces its leading live pairs only and ends its last
// live run there (no carry into the sentinel).  So the sentinel run is neither accumulated nor fixed up, and the work is
// proportional to the pairs that hit new rows.  The live runs have the association of egrad_chunk_reduce by construction;
// head / tail / run_start / run_end as there, for keys < sentinel (egrad_fixup over `sentinel` rows finishes).  T: this
// batch's projections.
template <int VEC, int NCH>
__global__ __launch_bounds__(256) void foldin_chunk_reduce(
    const int32_t* __restrict__ keys, const int32_t* __restrict__ pairs,
    const float* __restrict__ coef, const float* __restrict__ T, int total, int zp1, int de, int sentinel,
    float* __restrict__ G, float* __restrict__ head, float* __restrict__ tail,
    int32_t* __restrict__ run_start, int32_t* __restrict__ run_end) {
    chunk_reduce_rows<VEC, NCH, true>(keys, pairs, coef, T, total, zp1, de, sentinel, G, head, tail, run_start, run_end);
}

}  // namespace sert
