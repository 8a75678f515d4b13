// Folding unseen WORDS into a trained loglinear model (include/sert_hip_ll_wfold.h; host: host/api_ll_wfold.inc), gfx950.
// A token's distribution depends on its word only: L_t = log softmax(row_t W + b).  The rows of the upload's distinct frozen
// words never change (the frozen table Lf, computed once per upload), the Nw rows of the new words are recomputed every step
// (the step table Ln).  The loss terms are stated in loss_terms.h and only CALLED here (ll_label_term, ll_masked, ll_dz;
// clip_logp is common.h's).  Every sum has a fixed order: no atomics.
#pragma once
#include "common.h"
#include "loss_terms.h"

namespace sert {

enum { LLW_FORM_REG = 1, LLW_FORM_STREAM = 2 };   // (= SERT_LL_WFOLD_FORM_*, include/sert_hip_debug.h)

// The row kernel: one workgroup of 256 threads per instance i of the batch, entities across the lanes.
//   slot    (B, n) per position: >= 0 row of the frozen table Lf, < 0 new word ~slot = row of the step table Ln.  The window's
//           n rows are addressed through LDS as 64-bit ELEMENT offsets (the frozen table may pass 4 GiB) plus the table bit.
//   pass A  J_e = sum_t clip_logp(row_t[e]); an online (max, sum exp) per thread, merged in llf_row's fixed block tree -- the
//           maximum first, so that no inf - inf is formed --; J_y, ll_label_term, rowloss[i] = w_i * -log clip(Q_y)
//   pass B  (TRAIN) dJ_e = -Q_e qdq (+ qdq at e = y) written to DJ[i, e]
// FORM_REG (V_e <= 1024): J stays in four registers per thread between the passes -- vec: elements 4 tid .. 4 tid + 3 (one
// 16-byte load per row), else elements tid + 256 k.  FORM_STREAM: pass A stores J_e to DJ[i, e], pass B reads it back and
// overwrites it in place; the same thread reads and writes the same address, so no fence is needed.  Either way a table row
// is read once.  vec (V_e % 4 == 0, a launch-wide constant): 16-byte loads and stores; every row of Lf, Ln and DJ then
// starts on 16 bytes.  The kernel does not know which tokens are new beyond the table they are read from.
template <bool TRAIN, int FORM>
__global__ __launch_bounds__(256) void llw_row(const float* __restrict__ Lf, const float* __restrict__ Ln,
                                               const int32_t* __restrict__ slot, const int32_t* __restrict__ y,
                                               const float* __restrict__ w, float* __restrict__ rowloss, float* DJ, int n, int Ve,
                                               int vec, float inv_batch) {
    __shared__ float red[4];
    __shared__ unsigned long long s_off[32];
    __shared__ int s_new[32];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float LOGLO = logf(SERT_CLIP_LO), LOGHI = logf(SERT_CLIP_HI);
    if (tid < n) {
        const int s = slot[(size_t)i * n + tid];
        s_new[tid] = s < 0;
        s_off[tid] = (unsigned long long)(s < 0 ? ~s : s) * (unsigned long long)Ve;
    }
    __syncthreads();
    const int yi = y[i];
    float* dj_row = DJ + (size_t)i * Ve;
    auto row_of = [&](int t) -> const float* { return (s_new[t] ? Ln : Lf) + s_off[t]; };
    float mx = -INFINITY, se = 0.f, jy = 0.f;
    auto online = [&](float a) {
        if (a > mx) { se = se * expf(mx - a) + 1.0f; mx = a; }
        else se += expf(a - mx);
    };
    float J[4] = {0.f, 0.f, 0.f, 0.f};
    // ---- pass A ----
    if (FORM == LLW_FORM_REG) {
        if (vec) {
            const int e0 = 4 * tid;
            if (e0 < Ve) {
                for (int t = 0; t < n; ++t) {
                    const float4 x = *reinterpret_cast<const float4*>(row_of(t) + e0);
                    J[0] += clip_logp(x.x, LOGLO, LOGHI); J[1] += clip_logp(x.y, LOGLO, LOGHI);
                    J[2] += clip_logp(x.z, LOGLO, LOGHI); J[3] += clip_logp(x.w, LOGLO, LOGHI);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    online(J[k]);
                    if (e0 + k == yi) jy = J[k];
                }
            }
        } else {
            for (int t = 0; t < n; ++t) {
                const float* row = row_of(t);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = tid + 256 * k;
                    if (e < Ve) J[k] += clip_logp(row[e], LOGLO, LOGHI);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = tid + 256 * k;
                if (e < Ve) {
                    online(J[k]);
                    if (e == yi) jy = J[k];
                }
            }
        }
    } else if (vec) {
        for (int e0 = 4 * tid; e0 < Ve; e0 += 1024) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 0; t < n; ++t) {
                const float4 x = *reinterpret_cast<const float4*>(row_of(t) + e0);
                a.x += clip_logp(x.x, LOGLO, LOGHI); a.y += clip_logp(x.y, LOGLO, LOGHI);
                a.z += clip_logp(x.z, LOGLO, LOGHI); a.w += clip_logp(x.w, LOGLO, LOGHI);
            }
            online(a.x); online(a.y); online(a.z); online(a.w);
            if (yi >= e0 && yi < e0 + 4) jy = yi == e0 ? a.x : yi == e0 + 1 ? a.y : yi == e0 + 2 ? a.z : a.w;
            if (TRAIN) *reinterpret_cast<float4*>(dj_row + e0) = a;
        }
    } else {
        for (int e = tid; e < Ve; e += 256) {
            float a = 0.f;
            for (int t = 0; t < n; ++t) a += clip_logp(row_of(t)[e], LOGLO, LOGHI);
            online(a);
            if (e == yi) jy = a;
            if (TRAIN) dj_row[e] = a;
        }
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
    auto dj_of = [&](float j, int e) {
        const float dj = -(expf(j - M) / S) * qdq;
        return e == yi ? dj + qdq : dj;
    };
    if (FORM == LLW_FORM_REG) {
        if (vec) {
            const int e0 = 4 * tid;
            if (e0 < Ve)
                *reinterpret_cast<float4*>(dj_row + e0) =
                    make_float4(dj_of(J[0], e0), dj_of(J[1], e0 + 1), dj_of(J[2], e0 + 2), dj_of(J[3], e0 + 3));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = tid + 256 * k;
                if (e < Ve) dj_row[e] = dj_of(J[k], e);
            }
        }
    } else if (vec) {
        for (int e0 = 4 * tid; e0 < Ve; e0 += 1024) {
            const float4 a = *reinterpret_cast<const float4*>(dj_row + e0);
            *reinterpret_cast<float4*>(dj_row + e0) =
                make_float4(dj_of(a.x, e0), dj_of(a.y, e0 + 1), dj_of(a.z, e0 + 2), dj_of(a.w, e0 + 3));
        }
    } else {
        for (int e = tid; e < Ve; e += 256) dj_row[e] = dj_of(dj_row[e], e);
    }
}

// The row kernel for label ROWS (sert_ll_wfold_upload_csr): instance i's labels are the CSR row indptr[i] .. indptr[i + 1] of
// (indices, data) over the V_e trained entities, strictly increasing -- a word fold-in has no new column.  The launch shape,
// the LDS table, both forms, vec and pass A are llw_row's; the label is no longer one column:
//   pass A   J_e and (M, S) as in llw_row; a table row is read once
//   labels   thread tid takes entries l0 + tid, l0 + tid + 256, ..: J_e re-formed by gathering the window's n rows at column
//            indices[l] in pass A's t order (the owner thread's bits), q = exp(J_e - M) / S, ll_label_term; the row's loss and
//            s = sum_l Q_l dQ_l in the fixed block tree.  TRAIN: the entry's Q dQ goes to labfix[l] (per entry of the upload,
//            as the entity fold-in's and the model's: no cap on a row's labels)
//   pass B   (TRAIN) the dense dJ_e = -Q_e s to DJ[i, e] (FORM_REG: from the registers; FORM_STREAM: in place), a workgroup
//            barrier, then the thread of entry l adds labfix[l] to DJ[i, indices[l]]: the columns of a row are strictly
//            increasing, so every element has one writer behind the barrier -- no order to fix, no atomic
// indptr is the batch's (indptr + row0); its values are offsets into the UPLOAD's indices / data / labfix.  A row without an
// entry is legal (loss 0, DJ row zero), so is a stored 0.
template <bool TRAIN, int FORM>
__global__ __launch_bounds__(256) void llw_row_csr(const float* __restrict__ Lf, const float* __restrict__ Ln,
                                                   const int32_t* __restrict__ slot, const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices, const float* __restrict__ data,
                                                   const float* __restrict__ w, float* __restrict__ rowloss, float* labfix,
                                                   float* DJ, int n, int Ve, int vec, float inv_batch) {
    __shared__ float red[4];
    __shared__ unsigned long long s_off[32];
    __shared__ int s_new[32];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float LOGLO = logf(SERT_CLIP_LO), LOGHI = logf(SERT_CLIP_HI);
    if (tid < n) {
        const int s = slot[(size_t)i * n + tid];
        s_new[tid] = s < 0;
        s_off[tid] = (unsigned long long)(s < 0 ? ~s : s) * (unsigned long long)Ve;
    }
    __syncthreads();
    const int64_t l0 = indptr[i], l1 = indptr[i + 1];
    float* dj_row = DJ + (size_t)i * Ve;
    auto row_of = [&](int t) -> const float* { return (s_new[t] ? Ln : Lf) + s_off[t]; };
    float mx = -INFINITY, se = 0.f;
    auto online = [&](float a) {
        if (a > mx) { se = se * expf(mx - a) + 1.0f; mx = a; }
        else se += expf(a - mx);
    };
    float J[4] = {0.f, 0.f, 0.f, 0.f};
    // ---- pass A ----
    if (FORM == LLW_FORM_REG) {
        if (vec) {
            const int e0 = 4 * tid;
            if (e0 < Ve) {
                for (int t = 0; t < n; ++t) {
                    const float4 x = *reinterpret_cast<const float4*>(row_of(t) + e0);
                    J[0] += clip_logp(x.x, LOGLO, LOGHI); J[1] += clip_logp(x.y, LOGLO, LOGHI);
                    J[2] += clip_logp(x.z, LOGLO, LOGHI); J[3] += clip_logp(x.w, LOGLO, LOGHI);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) online(J[k]);
            }
        } else {
            for (int t = 0; t < n; ++t) {
                const float* row = row_of(t);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = tid + 256 * k;
                    if (e < Ve) J[k] += clip_logp(row[e], LOGLO, LOGHI);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (tid + 256 * k < Ve) online(J[k]);
        }
    } else if (vec) {
        for (int e0 = 4 * tid; e0 < Ve; e0 += 1024) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 0; t < n; ++t) {
                const float4 x = *reinterpret_cast<const float4*>(row_of(t) + e0);
                a.x += clip_logp(x.x, LOGLO, LOGHI); a.y += clip_logp(x.y, LOGLO, LOGHI);
                a.z += clip_logp(x.z, LOGLO, LOGHI); a.w += clip_logp(x.w, LOGLO, LOGHI);
            }
            online(a.x); online(a.y); online(a.z); online(a.w);
            if (TRAIN) *reinterpret_cast<float4*>(dj_row + e0) = a;
        }
    } else {
        for (int e = tid; e < Ve; e += 256) {
            float a = 0.f;
            for (int t = 0; t < n; ++t) a += clip_logp(row_of(t)[e], LOGLO, LOGHI);
            online(a);
            if (TRAIN) dj_row[e] = a;
        }
    }
    const float M = block_max_256(mx, red);
    const float S = block_sum_256(se * expf(mx - M), red);     // (a thread without an element: 0 * exp(-inf) = 0)
    const float wi = w ? w[i] : 1.0f;
    const float g = wi * inv_batch;
    // ---- the label entries ----
    float loss = 0.f, sdq = 0.f;
    for (int64_t l = l0 + tid; l < l1; l += 256) {
        const int e = indices[l];
        float a = 0.f;
        for (int t = 0; t < n; ++t) a += clip_logp(row_of(t)[e], LOGLO, LOGHI);
        float ylog, qdq;
        ll_label_term<TRAIN>(expf(a - M) / S, data[l], g, ylog, qdq);
        loss -= ylog;
        if (TRAIN) {
            sdq += qdq;
            labfix[l] = qdq;
        }
    }
    loss = block_sum_256(loss, red);
    if (tid == 0) rowloss[i] = wi * loss;
    if (!TRAIN) return;
    sdq = block_sum_256(sdq, red);
    // ---- pass B ----
    auto dj_of = [&](float j) { return -(expf(j - M) / S) * sdq; };
    if (FORM == LLW_FORM_REG) {
        if (vec) {
            const int e0 = 4 * tid;
            if (e0 < Ve)
                *reinterpret_cast<float4*>(dj_row + e0) = make_float4(dj_of(J[0]), dj_of(J[1]), dj_of(J[2]), dj_of(J[3]));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = tid + 256 * k;
                if (e < Ve) dj_row[e] = dj_of(J[k]);
            }
        }
    } else if (vec) {
        for (int e0 = 4 * tid; e0 < Ve; e0 += 1024) {
            const float4 a = *reinterpret_cast<const float4*>(dj_row + e0);
            *reinterpret_cast<float4*>(dj_row + e0) = make_float4(dj_of(a.x), dj_of(a.y), dj_of(a.z), dj_of(a.w));
        }
    } else {
        for (int e = tid; e < Ve; e += 256) dj_row[e] = dj_of(dj_row[e]);
    }
    __syncthreads();               // (the dense row, and every labfix entry of the row, are visible to the workgroup)
    for (int64_t l = l0 + tid; l < l1; l += 256) dj_row[indices[l]] += labfix[l];
}

// Behind the segmented sum S[v, :] = sum over the occurrences of new word v in the batch of DJ[row, :] (a word twice in a
// window counts its row twice; an absent word's row is zero): one wave per new word, over ALL Nw rows.
//   Rsum_v = <mask_v, S_v>, lane-strided in a fixed order plus wave_sum;  S_v <- mask_v S_v - P_v Rsum_v, in place
// (ll_masked / ll_dz on Ln[v, :], the log-probabilities of the step table).  A zero row stays zero.
__global__ __launch_bounds__(256) void llw_finish(const float* __restrict__ Ln, float* __restrict__ S, int Nw, int Ve) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= Nw) return;       // (whole waves leave: the wave reduction below sees 64 active lanes)
    const float LOGLO = logf(SERT_CLIP_LO), LOGHI = logf(SERT_CLIP_HI);
    const float* lp = Ln + (size_t)v * Ve;
    float* s = S + (size_t)v * Ve;
    float r = 0.f;
    for (int e = lane; e < Ve; e += 64) r += ll_masked(lp[e], s[e], LOGLO, LOGHI);
    r = wave_sum(r);
    for (int e = lane; e < Ve; e += 64) s[e] = ll_dz(lp[e], s[e], r, LOGLO, LOGHI);
}

}  // namespace sert
