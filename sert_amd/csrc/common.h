// Shared by the gfx950 kernels of libsert_hip.so and their host code: the environment switches (knob / variant_knob), the
// error plumbing (SERT_FAIL / SERT_HIP / SERT_TRY), device allocation (dmalloc, DevBuf), and the device helpers -- wave and workgroup reductions, ranking keys,
// the reference's clips and sigmoid, the write-through stores.  How a kernel is started is launch.h; how it is timed,
// host/timing.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

// ---- environment switches -----------------------------------------------------------------------------------
// The PRODUCT library reads twenty documented variables, through knob(); each is exercised by a test
// ("Environment"):
//   SERT_DP_EXCHANGE  SERT_AR_CHUNKS  SERT_STREAMS  SERT_SIDE_HEAVY  SERT_RE_DEFER  SERT_GEMM_FP32  SERT_NO_TOUCHED
//   SERT_SCORE_MATERIALISE  SERT_SCORE_FP32  SERT_LL_NODEDUP  SERT_LL_DW_SIDE  SERT_DENSE_HEAVY  SERT_FS_TILE_ROWS
//   SERT_EGRAD_SORT  SERT_ROCTX  SERT_EVENT_FENCE  SERT_LAZY_SKIP (0: dense_update_lazy instead of dense_update_skip)
//   SERT_LAZY_MAX (largest touched fraction of a batch whose word-table update is lazy; default 0.5 behind an announced
//   next batch, min(that, 0.35) without one)  SERT_LL_RANK_BUDGET (device bytes per chunk of sert_ll_rank_queries / _candidates)
//   SERT_SCORE_RANK_BUDGET (device bytes per query chunk of sert_scorer_rank)
// Round 6 moved the measured-and-lost opt-ins of round 5 behind variant_knob() and their kernels into csrc/variants/:
// SERT_PROJ_FUSED, SERT_GATHER_HOT, SERT_EGRAD_RANGES, SERT_SEG_BUNDLE (and SERT_BWD_FUSED's kernel).
// Everything else -- A/B variants that lost, cross-check paths of earlier rounds, tuning sweeps, timing
// knock-outs -- is read through variant_knob(), which is the environment only in a library built with
// -DSERT_VARIANTS (tools/build_variant.sh variants -DSERT_VARIANTS; run the suite against it with SERT_LIB=...)
// and a constant nullptr in the product build: those branches fold away.  59 names are read that way; the
// training step's schedule experiments that no test and no tool named were retired (HISTORY.md section 5).
// The knobs of the vectorspace step's SCHEDULE (SERT_SIDE_HEAVY, SERT_RE_DEFER; variants: SERT_EXT_EVENTS, SERT_FORK_LATE, SERT_FORK_AT,
// SERT_EARLY_BUCKET, SERT_NO_EARLY_BUCKET, SERT_EARLY_SORT, SERT_NO_EARLY_SORT, SERT_DW_FIRST, SERT_DP_LATE, SERT_NO_TAIL,
// SERT_EGRAD_GROUP_SUM, SERT_BWD_FUSED) are read in ONE place, vs_knobs() (host/step_vectorspace.inc), into VsKnobs (step_plan.h),
// where vs_plan_step turns them and the step's facts into the plan every launch site follows.
#include <stdlib.h>
static inline const char* knob(const char* name) { return getenv(name); }
#ifdef SERT_VARIANTS
static inline const char* variant_knob(const char* name) { return getenv(name); }
#else
static inline const char* variant_knob(const char*) { return nullptr; }
#endif

namespace sert {

constexpr int kWave = 64;  // CDNA wavefront width (hard-coded: warpSize folds to 64 on gfx950)

// ---- error plumbing (messages surface through sert_last_error()) ----------
extern thread_local std::string g_last_error;

inline int fail(const char* file, int line, const std::string& msg) {
    char buf[64];
    snprintf(buf, sizeof buf, "%s:%d: ", file, line);
    g_last_error = std::string(buf) + msg;
    return 1;
}

#define SERT_FAIL(msg) return ::sert::fail(__FILE__, __LINE__, (msg))
#define SERT_HIP(expr)                                                              \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess)                                                       \
            return ::sert::fail(__FILE__, __LINE__,                                 \
                                std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define SERT_TRY(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

// ---- device memory (host side) ---------------------------------------------
template <typename T>
inline int dmalloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) return 0;
    SERT_HIP(hipMalloc((void**)p, count * sizeof(T)));
    return 0;
}
// A grow-only device array: room for `cap` elements at `p`.  reserve(n) keeps the array when it is large enough; otherwise
// the old one is freed first, and what it held is gone.  It does not synchronise: the caller has nothing queued that still
// reads the old array.  After a reserve that FAILED the array is {nullptr, 0} -- never a freed pointer, never a capacity
// without memory behind it -- so the owner stays usable: the next reserve simply allocates again.  No destructor: the owner
// frees with release(), on the device it chose (sert_scorer_destroy).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;               // elements
    int reserve(int64_t n) {
        if (cap >= n) return 0;
        release();
        SERT_TRY(dmalloc(&p, (size_t)n));
        cap = n;
        return 0;
    }
    void release() {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// ---- wave-level reductions -------------------------------------------------
// DPP row operations (pure VALU, ~1 issue each) reduce each 16-lane row, four
// v_readlane + scalar ops combine the rows: no LDS round trips (the generic
// __shfl_xor lowers to ds_bpermute, ~50 cycles of dependent latency per step).
// Every lane of the wave must be active; every lane receives the result.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over each aligned group of 16 lanes (one DPP "row")
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]  (xor 1)
    v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]  (xor 2)
    v += dpp_mov<0x124>(v);   // row_ror:4
    v += dpp_mov<0x128>(v);   // row_ror:8
    return v;
}
// lane u of each aligned group of sixteen lanes, to all sixteen of the group (DPP row_newbcast: one VALU issue; u a constant
// after unrolling)
__device__ __forceinline__ int row16_bcast(int v, int u) {
    switch (u & 15) {
#define SERT_ROW_BCAST(U) case U: return __builtin_amdgcn_update_dpp(0, v, 0x150 + U, 0xF, 0xF, true);
        SERT_ROW_BCAST(0) SERT_ROW_BCAST(1) SERT_ROW_BCAST(2) SERT_ROW_BCAST(3) SERT_ROW_BCAST(4) SERT_ROW_BCAST(5)
        SERT_ROW_BCAST(6) SERT_ROW_BCAST(7) SERT_ROW_BCAST(8) SERT_ROW_BCAST(9) SERT_ROW_BCAST(10) SERT_ROW_BCAST(11)
        SERT_ROW_BCAST(12) SERT_ROW_BCAST(13) SERT_ROW_BCAST(14)
        default: return __builtin_amdgcn_update_dpp(0, v, 0x15F, 0xF, 0xF, true);
#undef SERT_ROW_BCAST
    }
}
__device__ __forceinline__ float row16_bcast(float v, int u) { return __int_as_float(row16_bcast(__float_as_int(v), u)); }
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x124>(v));
    v = fmaxf(v, dpp_mov<0x128>(v));
    return v;
}
__device__ __forceinline__ float read_lane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float wave_sum(float v) {
    v = row16_sum(v);
    return (read_lane(v, 0) + read_lane(v, 16)) + (read_lane(v, 32) + read_lane(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = row16_max(v);
    return fmaxf(fmaxf(read_lane(v, 0), read_lane(v, 16)), fmaxf(read_lane(v, 32), read_lane(v, 48)));
}

// Block-wide sum for blockDim.x == 256 (4 waves). `red` is >= 4 floats of LDS.
// Result valid in every thread.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// NW-wave workgroup variants (red: NW floats of LDS)
template <int NW>
__device__ __forceinline__ float block_sum_n(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float a = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) a += red[i];
    return a;
}
template <int NW>
__device__ __forceinline__ float block_max_n(float v, float* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float a = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) a = fmaxf(a, red[i]);
    return a;
}
__device__ __forceinline__ float block_max_256(float v, float* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// Order-preserving map float -> uint32 such that ascending uint == DESCENDING float.
__device__ __forceinline__ uint32_t desc_key(float f) {
    uint32_t u = __float_as_uint(f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending map
    return ~u;                                        // flip => descending
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
    uint32_t u = ~k;
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}

// desc_key under the cosine scorer's order ("One ranking order"): -0 takes +0's key, so that the two tie and the
// lowest entity index decides, and a NaN of either sign takes the last key, after every number (key_to_float gives a NaN back
// for it).  List entries of that key still sort before the ~0 padding of the bitonic sorts: their low word is an entity index.
__device__ __forceinline__ uint32_t score_key(float f) {
    if (f != f) return 0xffffffffu;
    const uint32_t u = __float_as_uint(f);
    return u == 0x80000000u ? 0x7fffffffu : desc_key(f);
}
// the key a row is ordered by (topk_rows, kernels_score.h; the full rankings, kernels_rank.h): the scorer's (score_key: -0
// ties with +0, NaN last) or, RAW, the loglinear ranker's plain one
template <bool RAW>
__device__ __forceinline__ uint32_t rank_key(float x) { return RAW ? desc_key(x) : score_key(x); }
// the same on a key that desc_key made of a number (the fp32 filter's lists hold no NaN: `v >= thr` is false for one)
__device__ __forceinline__ uint32_t score_key_of_desc_key(uint32_t k) { return k == 0x80000000u ? 0x7fffffffu : k; }

// clip bounds of the reference as fp32 constants: 1e-7 and float32(1 - 1e-7)
// = 1 - 2^-23 (sert/models.py:200, :290, :900, :1067-1068)
#define SERT_CLIP_LO 1e-7f
#define SERT_CLIP_HI 0.99999988079071044921875f

// clip(t, -(1-eps), 1-eps) (sert/models.py:1065-1068) and clip(s, eps, 1-eps) (:900, :290) as numpy and Theano compute them: a
// NaN stays a NaN (fminf / fmaxf return the OTHER operand for one -- a NaN probability became 1e-7 and its loss finite).
__device__ __forceinline__ float clip_unit(float t) {
    return t > SERT_CLIP_HI ? SERT_CLIP_HI : (t < -SERT_CLIP_HI ? -SERT_CLIP_HI : t);
}
__device__ __forceinline__ float clip_prob(float s) {
    return s > SERT_CLIP_HI ? SERT_CLIP_HI : (s < SERT_CLIP_LO ? SERT_CLIP_LO : s);
}
// The same clip of a LOG-probability, clip(log p, log eps, log(1-eps)) = log clip(p, eps, 1-eps) (sert/models.py:200): the
// loglinear loss kernels (kernels_ll.h) keep the token distributions in the log domain.  A NaN stays a NaN here too -- as
// fminf(fmaxf(..)) it became log(1e-7), the row's J, Q and loss stayed finite while the backward filled W and b with NaN,
// and the epoch loop's non-finite check never fired.  For every other input the result is lo, hi or x itself, the bits the
// min/max form gave (-inf, the log of a zero probability, clips to lo).
__device__ __forceinline__ float clip_logp(float lp, float lo, float hi) {
    return lp > hi ? hi : (lp < lo ? lo : lp);
}

// T.nnet.sigmoid, float32 C implementation of Theano 0.8.2 [upstream]:
// x < -88 -> 0 ; x > 15 -> 1 ; else 1/(1+exp(-x))
__device__ __forceinline__ float theano_sigmoid(float x) {
    if (x < -88.0f) return 0.0f;
    if (x > 15.0f) return 1.0f;
    return 1.0f / (1.0f + expf(-x));
}

// ---- 16-byte WRITE-THROUGH stores (sc1) ---------------------------------------------------------------------------
// A plain (or nt) store leaves its line dirty in the XCD's L2 until the release at the end of the launch writes every
// dirty line back in one piece, while the queue does nothing else; an sc1 store sends the line on as it is written and
// drops it from that L2 (a later reader of the bytes then finds them beyond its XCD's L2).  Which of the step's streaming
// outputs go out this way is a compile-time choice, one bit of SERT_WT_STORES per kernel family (DESIGN.md section 3;
// measured with tools/build_variant.sh NAME -DSERT_WT_STORES=0x.. , profiles/r11_experiments.txt).  Same bytes, same
// values: only the flavour of the store instruction differs.
//   * Through the buffer-store builtin (cache policy bit 4 = sc1 on gfx94x / gfx95x), so that the compiler tracks the
//     store in vmcnt: a first version issued it from inline assembly, which let the compiler overwrite the data registers
//     while the store was still reading them (round 4).
//   * The descriptor is built from `base`, which must be wave-uniform (a kernel argument: it then lives in SGPRs); the
//     per-lane byte offset is 32 bits wide, and the descriptor's range is no guard: the CALLER stores only from lanes
//     that stored before.  store16<BIT> takes any element offset and sends the pieces that lie 2 GiB or more behind
//     `base` through the plain store, so no shape the library accepts is cut off.
typedef float sert_wt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16_wt(float* base, unsigned byte_off, const float4& v) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0xffffffff, 0x00020000);
    sert_wt_f4 x = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(x, rs, (int)byte_off, 0, /*sc1*/ 1 << 4);
}
enum {
    kWtGather = 0x01,   // vs_gather_mean / vs_gather_mean_tail: H
    kWtNce = 0x02,      // vs_nce / vs_nce_regs: DA
    kWtSeg = 0x04,      // the word-gradient tree (kernels_seg.h): final rows, partial rows, the heavy words' partial rows
    kWtParam = 0x08,    // adam_l2 / dense_update_lazy / dense_update_skip: p
    kWtState = 0x10,    // ... m and v (in place of their nt stores)
    kWtEgrad = 0x20,    // egrad_acc: the partial entity-gradient tables (side queue)
};
// Default: H and the tree's rows (round 11, C2: -2.5 % per step, every run of the change ahead of every run of the parent,
// no other record of bench.py --full slower).  Not p (C2 another -0.3 %, inside the noise, and the W3C loglinear settings
// +1.1 % in every run), not DA (equal), not the partial entity-gradient tables (equal), not m / v (slower than their nt
// stores: 0.2127 -> 0.2157).  profiles/r11_experiments.txt.
#ifndef SERT_WT_STORES
#define SERT_WT_STORES 0x05
#endif
// The lane's piece through store16_wt if it lies less than 2 GiB behind `base`; false (nothing stored) otherwise.  The guard
// is per lane and in the kernel on purpose, not a check on the host: the tables these stores walk may be larger than
// 2 GiB (the library accepts them), and a host check could only refuse such a model or pick another kernel for it.  Here the
// far pieces of a large tensor take the store they always took and every piece below 2 GiB is written through; the cost is
// one compare and a second store form in the kernel (registers: profiles/r11_experiments.txt, item 0).  No shape of the
// test suite reaches the far side (a tensor of 2 GiB and more); it is the parent's plain store, unchanged.
__device__ __forceinline__ bool store16_wt_near(float* base, size_t elem_off, const float4& v) {
    if (elem_off >= ((size_t)1 << 29)) return false;
    store16_wt(base, (unsigned)elem_off * 4u, v);
    return true;
}
template <int BIT>
__device__ __forceinline__ void store16(float* base, size_t elem_off, const float4& v) {
    if constexpr ((SERT_WT_STORES & BIT) != 0) {
        if (store16_wt_near(base, elem_off, v)) return;
    }
    *reinterpret_cast<float4*>(base + elem_off) = v;
}
// the optimiser state: streaming (nt) unless its bit asks for write-through; -DSERT_ADAM_NO_NT: plain
__device__ __forceinline__ void store16_state(float* base, size_t elem_off, const float4& v) {
    if constexpr ((SERT_WT_STORES & kWtState) != 0) {
        if (store16_wt_near(base, elem_off, v)) return;
    }
#ifndef SERT_ADAM_NO_NT
    sert_wt_f4 t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<sert_wt_f4*>(base + elem_off));
#else
    *reinterpret_cast<float4*>(base + elem_off) = v;
#endif
}

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace sert
