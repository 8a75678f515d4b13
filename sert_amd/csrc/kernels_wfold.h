// Folding unseen WORDS into a trained vectorspace model (include/sert_hip_wfold.h; host: host/api_wfold.inc; the index:
// wfold_index.h; DESIGN.md, "Folding unseen words into a vectorspace model"), gfx950.
//
// The V_w trained word rows, the projection and the whole entity table are FROZEN; only the Nw new word rows Nv learn.  The
// projection is linear below the tanh, so with P = Nv W (Nw, d_e), tok (M, n) the new word of every position (-1: frozen) and
// A0 = hf W + b computed once at upload (hf: the window mean with the new positions counted as zero rows)
//   a_i = A0_i + (sum over the positions j with tok_ij >= 0, ascending, of P[tok_ij]) / n
// and the step needs no per-instance GEMM.  A step is
//   launch_gemm            P = Nv W                                                        (gemm.h, as it is)
//   wfold_project          T = tanh(a) for the B rows of the batch                         (here)
//   vs_nce / vs_nce_scalar the model's loss kernel on T: DA, rowloss, the loss partials   (kernels_vs.h, as it is)
//   segsum_rows / segsum_rows_scalar over the batch's inverted index new word -> batch rows: S[v] = (sum of DA rows) / n
//                          (kernels_seg.h, as they are: the item format and the row width fit)
//   launch_gemm            G = S W^T
//   adam_l2, finalize_loss (kernels_opt.h, as they are)
// The factor 1/n: once per instance here (the finished sum of an instance's P rows is divided by n, as vs_gather_mean divides
// its window sum), once per word in the gradient (segsum_rows divides a word's finished sum by its divisor n).
// Order-fixed throughout, no floating-point atomic: a word fold-in is bit-reproducible.
#pragma once
#include "common.h"
#include "gemm.h"   // (fast_tanh: the projection epilogue's tanh, so that T holds what the model's forward would)

namespace sert {

// One thread per (batch row, VEC-wide column chunk), VEC = 4 (d_e % 4 == 0) or 1: consecutive lanes read consecutive pieces
// of one row of A0 and of one row of P.  P is small and hot in L2 (Nw d_e floats: 512 kB at 1024 words of width 128); most
// positions are frozen, so a position costs its 4-byte token and a uniform-enough branch.  A0, tok: the rows of THIS batch
// (the host passes the batch's first row).  T (B, d_e).
template <int VEC>
__global__ __launch_bounds__(256) void wfold_project(const float* __restrict__ A0, const int32_t* __restrict__ tok,
                                                     const float* __restrict__ P, float* __restrict__ T, int B, int n, int de) {
    const int chunks = de / VEC;
    const int64_t total = (int64_t)B * chunks;
    const float fn = (float)n;
    for (int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (int64_t)gridDim.x * blockDim.x) {
        const int row = (int)(tid / chunks);
        const int c = (int)(tid - (int64_t)row * chunks) * VEC;
        const int32_t* tr = tok + (size_t)row * n;
        const size_t o = (size_t)row * de + c;
        if (VEC == 4) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < n; ++k) {
                const int v = tr[k];
                if (v < 0) continue;
                const float4 p = *reinterpret_cast<const float4*>(P + (size_t)v * de + c);
                s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
            }
            const float4 a = *reinterpret_cast<const float4*>(A0 + o);
            *reinterpret_cast<float4*>(T + o) = make_float4(fast_tanh(a.x + s.x / fn), fast_tanh(a.y + s.y / fn),
                                                            fast_tanh(a.z + s.z / fn), fast_tanh(a.w + s.w / fn));
        } else {
            float s = 0.f;
            for (int k = 0; k < n; ++k) {
                const int v = tr[k];
                if (v >= 0) s += P[(size_t)v * de + c];
            }
            T[o] = fast_tanh(A0[o] + s / fn);
        }
    }
}

// upload only: the ids the frozen forward gathers (a new position reads the zero row appended behind the V_w trained rows)
// and the new word of every position (-1: frozen).  count = rows * n positions.
__global__ __launch_bounds__(256) void wfold_split_ids(const int32_t* __restrict__ x, uint32_t* __restrict__ frozen_ids,
                                                       int32_t* __restrict__ tok, int64_t count, int Vw) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) {
        const int32_t id = x[k];
        frozen_ids[k] = (uint32_t)(id < Vw ? id : Vw);
        tok[k] = id < Vw ? -1 : id - Vw;
    }
}

}  // namespace sert
