// Folding unseen entities into a trained loglinear model (include/sert_hip_ll_foldin.h; host: host/api_ll_foldin.inc), gfx950.
// The logits of the V_e trained entities for a word never change: Zold (|D|, V_e) holds them for the upload's distinct words,
// and a step computes logits of the N new columns only.  The loss terms are stated in loss_terms.h and only CALLED here
// (ll_label_term, logp_inside / ll_masked / ll_dz; clip_logp is common.h's).  Every sum has a fixed order: no atomics.
#pragma once
#include "common.h"
#include "loss_terms.h"

namespace sert {

// Once per handle that refreshes trained columns (sert_ll_foldin_create_refresh): one pass over the model's W (d, V_e) and
// b (V_e), row d of the pass being b.  Element (k, e) goes to internal column c = internal_of[e] (ll_label_remap.h): a frozen
// column c < V_f to the compact Wf (d, V_f) / bf (V_f), a refreshed one to slot c - V_f of the trainable Wt (d, Nt) / bt (Nt).
// Consecutive threads read consecutive e of one row; internal_of is a bijection of [0, V_e) onto [0, V_f + R), so every
// output element has exactly one writer, and the new columns [R, Nt) of Wt / bt are not touched.  Wf / bf may be null when
// V_f = 0: no column is below 0.
__global__ __launch_bounds__(256) void llf_compact(const float* __restrict__ W, const float* __restrict__ b,
                                                   const int32_t* __restrict__ internal_of, float* __restrict__ Wf,
                                                   float* __restrict__ bf, float* __restrict__ Wt, float* __restrict__ bt,
                                                   int d, int Ve, int Vf, int Nt) {
    const int64_t total = ((int64_t)d + 1) * Ve;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i / Ve), e = (int)(i - (int64_t)k * Ve);
        const int c = internal_of[e];
        const float v = k < d ? W[i] : b[e];
        if (c < Vf) {
            if (k < d) Wf[(size_t)k * Vf + c] = v; else bf[c] = v;
        } else {
            if (k < d) Wt[(size_t)k * Nt + (c - Vf)] = v; else bt[c - Vf] = v;
        }
    }
}

// Once per upload: stat[r] = (max_e Zold[r, e], sum_e exp(Zold[r, e] - max)) over the frozen entities.  One workgroup per row;
// the maximum first, so that an entity switched off (a bias of -inf) adds exp(-inf) = 0 and no inf - inf is ever formed.
__global__ __launch_bounds__(256) void llf_row_stat(const float* __restrict__ Zold, int V, float2* __restrict__ stat) {
    __shared__ float red[4];
    const float* row = Zold + (size_t)blockIdx.x * V;
    float mx = -INFINITY;
    for (int e = threadIdx.x; e < V; e += 256) mx = fmaxf(mx, row[e]);
    mx = block_max_256(mx, red);
    float se = 0.f;
    for (int e = threadIdx.x; e < V; e += 256) se += expf(row[e] - mx);
    se = block_sum_256(se, red);
    if (threadIdx.x == 0) stat[blockIdx.x] = make_float2(mx, se);
}

// Per step, one wave per distinct word u of the batch: the word's frozen (max, sum) merged with its N new logits into
// lse[u] = log sum over all V_e + N entities; Zn[u, :] becomes the LOG-probabilities of the new columns.
__global__ __launch_bounds__(256) void llf_lse(float* __restrict__ Zn, const float2* __restrict__ stat,
                                               const int32_t* __restrict__ Lb, float* __restrict__ lse, int U, int N) {
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= U) return;        // (whole waves leave: the wave reductions below see 64 active lanes)
    float* z = Zn + (size_t)u * N;
    const float2 st = stat[Lb[u]];
    float mx = st.x;
    for (int j = lane; j < N; j += 64) mx = fmaxf(mx, z[j]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int j = lane; j < N; j += 64) se += expf(z[j] - mx);
    se = wave_sum(se) + st.y * expf(st.x - mx);
    const float l = mx + logf(se);
    for (int j = lane; j < N; j += 64) z[j] -= l;
    if (lane == 0) lse[u] = l;
}

// The row kernel: one workgroup per instance i of the batch.
//   pass A  J_e = sum_t clip(log P_te) over the frozen entities (Zold rows of the window's words, lanes over e) and the new
//           columns (logpn), an online (max, sum exp) of J per thread merged in a fixed tree, J_y, Q_y, the row's loss
//   pass B  (TRAIN) the same rows again: dJ_e = Q_e (dQ_e - Q_y dQ_y), r_t = sum_e mask_te dJ_e in NMAX registers per
//           thread, then dZ[token, j] = mask dJ_j - P_tj r_t for the N new columns only
// tok: the (B, n) slots of the tokens in the batch's word list Lb; Lb[u]: the word's row of Zold.  n <= NMAX <= 32.
template <bool TRAIN, int NMAX>
__global__ __launch_bounds__(256) void llf_row(const float* __restrict__ Zold, const float* __restrict__ logpn,
                                               const float* __restrict__ lse, const int32_t* __restrict__ Lb,
                                               const int32_t* __restrict__ tok, const int32_t* __restrict__ y,
                                               const float* __restrict__ w, float* __restrict__ rowloss,
                                               float* __restrict__ dZ, int n, int Ve, int N, float inv_batch) {
    __shared__ float red[4];
    __shared__ unsigned long long s_off[32];    // element offset of token t's row of Zold (64 bits: the cache may pass 2 GiB)
    __shared__ unsigned s_new[32];              // ... and of its row of logpn
    __shared__ float s_lse[32], s_r[32];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float LOGLO = logf(SERT_CLIP_LO), LOGHI = logf(SERT_CLIP_HI);
    if (tid < n) {
        const int u = tok[(size_t)i * n + tid];
        s_off[tid] = (unsigned long long)Lb[u] * (unsigned long long)Ve;
        s_new[tid] = (unsigned)u * (unsigned)N;
        s_lse[tid] = lse[u];
    }
    __syncthreads();
    const int yi = y[i];
    // ---- pass A ----
    float mx = -INFINITY, se = 0.f, jy = 0.f;
    auto online = [&](float a) {
        if (a > mx) { se = se * expf(mx - a) + 1.0f; mx = a; }
        else se += expf(a - mx);
    };
    for (int e = tid; e < Ve; e += 256) {
        float a = 0.f;
        for (int t = 0; t < n; ++t) a += clip_logp(Zold[s_off[t] + e] - s_lse[t], LOGLO, LOGHI);
        online(a);
    }
    for (int j = tid; j < N; j += 256) {
        float a = 0.f;
        for (int t = 0; t < n; ++t) a += clip_logp(logpn[s_new[t] + j], LOGLO, LOGHI);
        online(a);
        if (j == yi) jy = a;
    }
    const float M = block_max_256(mx, red);
    const float S = block_sum_256(se * expf(mx - M), red);     // (a thread without an element: 0 * exp(-inf) = 0)
    jy = block_sum_256(jy, red);
    const float wi = w ? w[i] : 1.0f;
    const float g = wi * inv_batch;
    float ylog, qdq;
    ll_label_term<TRAIN>(expf(jy - M) / S, 1.0f, g, ylog, qdq);
    if (tid == 0) rowloss[i] = wi * -ylog;
    if (!TRAIN) return;
    // ---- pass B ----
    float r[NMAX];
#pragma unroll
    for (int t = 0; t < NMAX; ++t) r[t] = 0.f;
    for (int e = tid; e < Ve; e += 256) {
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) { lp[t] = Zold[s_off[t] + e] - s_lse[t]; a += clip_logp(lp[t], LOGLO, LOGHI); }
        const float dj = -(expf(a - M) / S) * qdq;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) r[t] += ll_masked(lp[t], dj, LOGLO, LOGHI);
    }
    for (int j = tid; j < N; j += 256) {
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) { lp[t] = logpn[s_new[t] + j]; a += clip_logp(lp[t], LOGLO, LOGHI); }
        float dj = -(expf(a - M) / S) * qdq;
        if (j == yi) dj += qdq;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) r[t] += ll_masked(lp[t], dj, LOGLO, LOGHI);
    }
#pragma unroll
    for (int t = 0; t < NMAX; ++t) {
        if (t < n) {               // (n is uniform: every thread takes the same barriers)
            const float rt = block_sum_256(r[t], red);
            if (tid == 0) s_r[t] = rt;
        }
    }
    __syncthreads();
    for (int j = tid; j < N; j += 256) {
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) { lp[t] = logpn[s_new[t] + j]; a += clip_logp(lp[t], LOGLO, LOGHI); }
        float dj = -(expf(a - M) / S) * qdq;
        if (j == yi) dj += qdq;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) dZ[((size_t)i * n + t) * N + j] = ll_dz(lp[t], dj, s_r[t], LOGLO, LOGHI);
    }
}

// The row kernel for label ROWS (sert_ll_foldin_upload_csr): instance i's labels are the CSR row indptr[i] .. indptr[i + 1] of
// (indices, data) over the V_e + N columns, strictly increasing; column e < V_e is frozen entity e -- a label only --, column
// V_e + j new entity j.  The launch shape, the LDS tables and pass A are llf_row's; the label is no longer one column:
//   pass A   (M, S) of the joint over all V_e + N columns
//   labels   thread tid takes entries l0 + tid, l0 + tid + 256, ..: J_e gathered from the cache (e < V_e) or from logpn,
//            q = exp(J_e - M) / S, ll_label_term; the row's loss and s = sum_l Q_l dQ_l in the fixed tree.  TRAIN: the entry's
//            Q dQ goes to labfix[l] (per entry of the upload, as the model's: no cap on a row's labels) and its share
//            mask_t Q dQ of r_t to the owning thread's registers -- frozen and new columns alike
//   pass B   (TRAIN) the dense part dJ_e = -Q_e s of every column into r_t, then dZ[token, j] for the N new columns with
//            dJ_j = -Q_j s + labfix of the row's entry at column V_e + j, where it has one: the columns are sorted, so the
//            new-side entries are the row's tail [lt, l1), and the thread of column j looks its entry up by bisection --
//            one writer per element, no order to fix
// indptr is the batch's (indptr + row0); its values are offsets into the UPLOAD's indices / data / labfix.
template <bool TRAIN, int NMAX>
__global__ __launch_bounds__(256) void llf_row_csr(const float* __restrict__ Zold, const float* __restrict__ logpn,
                                                   const float* __restrict__ lse, const int32_t* __restrict__ Lb,
                                                   const int32_t* __restrict__ tok, const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices, const float* __restrict__ data,
                                                   const float* __restrict__ w, float* __restrict__ rowloss, float* labfix,
                                                   float* __restrict__ dZ, int n, int Ve, int N, float inv_batch) {
    __shared__ float red[4];
    __shared__ unsigned long long s_off[32];
    __shared__ unsigned s_new[32];
    __shared__ float s_lse[32], s_r[32];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float LOGLO = logf(SERT_CLIP_LO), LOGHI = logf(SERT_CLIP_HI);
    if (tid < n) {
        const int u = tok[(size_t)i * n + tid];
        s_off[tid] = (unsigned long long)Lb[u] * (unsigned long long)Ve;
        s_new[tid] = (unsigned)u * (unsigned)N;
        s_lse[tid] = lse[u];
    }
    __syncthreads();
    const int64_t l0 = indptr[i], l1 = indptr[i + 1];
    // ---- pass A ----
    float mx = -INFINITY, se = 0.f;
    auto online = [&](float a) {
        if (a > mx) { se = se * expf(mx - a) + 1.0f; mx = a; }
        else se += expf(a - mx);
    };
    for (int e = tid; e < Ve; e += 256) {
        float a = 0.f;
        for (int t = 0; t < n; ++t) a += clip_logp(Zold[s_off[t] + e] - s_lse[t], LOGLO, LOGHI);
        online(a);
    }
    for (int j = tid; j < N; j += 256) {
        float a = 0.f;
        for (int t = 0; t < n; ++t) a += clip_logp(logpn[s_new[t] + j], LOGLO, LOGHI);
        online(a);
    }
    const float M = block_max_256(mx, red);
    const float S = block_sum_256(se * expf(mx - M), red);
    const float wi = w ? w[i] : 1.0f;
    const float g = wi * inv_batch;
    // ---- the label entries ----
    float r[NMAX];
#pragma unroll
    for (int t = 0; t < NMAX; ++t) r[t] = 0.f;
    float loss = 0.f, sdq = 0.f;
    for (int64_t l = l0 + tid; l < l1; l += 256) {
        const int e = indices[l];
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) {
                lp[t] = e < Ve ? Zold[s_off[t] + e] - s_lse[t] : logpn[s_new[t] + (e - Ve)];
                a += clip_logp(lp[t], LOGLO, LOGHI);
            }
        float ylog, qdq;
        ll_label_term<TRAIN>(expf(a - M) / S, data[l], g, ylog, qdq);
        loss -= ylog;
        if (TRAIN) {
            sdq += qdq;
            labfix[l] = qdq;
#pragma unroll
            for (int t = 0; t < NMAX; ++t)
                if (t < n) r[t] += ll_masked(lp[t], qdq, LOGLO, LOGHI);
        }
    }
    loss = block_sum_256(loss, red);
    if (tid == 0) rowloss[i] = wi * loss;
    if (!TRAIN) return;
    sdq = block_sum_256(sdq, red);
    // ---- pass B ----
    for (int e = tid; e < Ve; e += 256) {
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) { lp[t] = Zold[s_off[t] + e] - s_lse[t]; a += clip_logp(lp[t], LOGLO, LOGHI); }
        const float dj = -(expf(a - M) / S) * sdq;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) r[t] += ll_masked(lp[t], dj, LOGLO, LOGHI);
    }
    for (int j = tid; j < N; j += 256) {
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) { lp[t] = logpn[s_new[t] + j]; a += clip_logp(lp[t], LOGLO, LOGHI); }
        const float dj = -(expf(a - M) / S) * sdq;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) r[t] += ll_masked(lp[t], dj, LOGLO, LOGHI);
    }
#pragma unroll
    for (int t = 0; t < NMAX; ++t) {
        if (t < n) {               // (n is uniform: every thread takes the same barriers)
            const float rt = block_sum_256(r[t], red);
            if (tid == 0) s_r[t] = rt;
        }
    }
    __syncthreads();               // (s_r; and every labfix entry of the row, written above by its owner, is visible)
    // the row's tail: its first entry on a new column (the same bisection in every thread)
    int64_t lt = l0;
    for (int64_t hi = l1; lt < hi;) {
        const int64_t mid = lt + ((hi - lt) >> 1);
        if (indices[mid] < Ve) lt = mid + 1; else hi = mid;
    }
    for (int j = tid; j < N; j += 256) {
        float lp[NMAX], a = 0.f;
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) { lp[t] = logpn[s_new[t] + j]; a += clip_logp(lp[t], LOGLO, LOGHI); }
        float dj = -(expf(a - M) / S) * sdq;
        int64_t lo = lt;
        for (int64_t hi = l1; lo < hi;) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (indices[mid] < Ve + j) lo = mid + 1; else hi = mid;
        }
        if (lo < l1 && indices[lo] == Ve + j) dj += labfix[lo];
#pragma unroll
        for (int t = 0; t < NMAX; ++t)
            if (t < n) dZ[((size_t)i * n + t) * N + j] = ll_dz(lp[t], dj, s_r[t], LOGLO, LOGHI);
    }
}

// dZu[u, :] = the sum of the dZ rows of word u's tokens, in ascending token order (ptr / pos: the batch's CSR of token
// positions per word, built on the host at upload).  One thread per (u, j).
__global__ __launch_bounds__(256) void llf_word_sum(const float* __restrict__ dZ, const int32_t* __restrict__ ptr,
                                                    const int32_t* __restrict__ pos, float* __restrict__ dZu, int U, int N) {
    const int64_t total = (int64_t)U * N;
    for (int64_t k = blockIdx.x * (int64_t)256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
        const int u = (int)(k / N), j = (int)(k - (int64_t)u * N);
        float a = 0.f;
        for (int q = ptr[u]; q < ptr[u + 1]; ++q) a += dZ[(size_t)pos[q] * N + j];
        dZu[k] = a;
    }
}

}  // namespace sert
