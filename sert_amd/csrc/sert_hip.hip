// libsert_hip.so -- C ABI (include/sert_hip.h) over the gfx950 kernels.
// Host orchestration of one training / evaluation / prediction step: the body of
// the reference's compiled Theano functions (sert/models.py:581-608).
#include <dlfcn.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "common.h"
#include "launch.h"
#include "gemm.h"
#include "gemm_x3.h"
#ifdef SERT_VARIANTS   // opt-in variants that lost their A/B (csrc/variants/; tools/build_variant.sh -DSERT_VARIANTS)
#include "variants/gemm_bwd_fused.h"
#include "variants/gemm_big.h"
#include "variants/gemm_x3_bres.h"
#include "variants/score_filter_ring.h"
#include "variants/gemm_strip.h"
#include "variants/gemm_stream.h"
#include "variants/gemm_direct.h"
#endif
#include "kernels_score_bf16.h"
#include "kernels_egrad.h"
#include "kernels_ll.h"
#include "kernels_ll_rank.h"
#include "kernels_ll_rerank.h"
#include "kernels_membench.h"
#include "kernels_opt.h"
#include "kernels_rank.h"
#include "kernels_rerank.h"
#include "kernels_reval.h"
#include "kernels_score.h"
#include "kernels_seg.h"
#include "kernels_sort.h"
#include "kernels_vs.h"
#include "kernels_foldin.h"
#include "kernels_ll_foldin.h"
#include "kernels_wfold.h"
#include "kernels_ll_wfold.h"
#include "wfold_index.h"
#include "ll_label_remap.h"
#ifdef SERT_VARIANTS
#include "variants/kernels_gather_hot.h"
#include "variants/kernels_seg_bundled.h"
#include "variants/kernels_egrad_ranges.h"
#include "variants/kernels_proj.h"   // (after kernels_vs.h / gemm_x3.h: gather + mean-pool + projection in one persistent launch, measured slower)
#endif
#include "model.h"

namespace sert {
thread_local std::string g_last_error;

// ---- RCCL, loaded lazily (single-GPU runs never touch it) --------------------
struct UniqueId {
    char internal[SERT_COMM_ID_BYTES];
};
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, /*ncclUniqueId by value*/ UniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*ReduceScatter)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static Rccl g_rccl;

static int rccl_load() {
    if (g_rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1",
                           "/opt/rocm/lib/librccl.so"};
    void* lib = nullptr;
    for (const char* n : names) {
        lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    if (!lib) SERT_FAIL(std::string("cannot dlopen librccl: ") + dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(lib, "ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(lib, "ncclAllReduce");
    g_rccl.ReduceScatter = (decltype(g_rccl.ReduceScatter))dlsym(lib, "ncclReduceScatter");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(lib, "ncclAllGather");
    g_rccl.Send = (decltype(g_rccl.Send))dlsym(lib, "ncclSend");
    g_rccl.Recv = (decltype(g_rccl.Recv))dlsym(lib, "ncclRecv");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(lib, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(lib, "ncclGroupEnd");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce ||
        !g_rccl.ReduceScatter || !g_rccl.AllGather || !g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart ||
        !g_rccl.GroupEnd)
        SERT_FAIL("librccl is missing ncclGetUniqueId/ncclCommInitRank/ncclCommDestroy/ncclAllReduce/"
                  "ncclReduceScatter/ncclAllGather/ncclSend/ncclRecv/ncclGroupStart/ncclGroupEnd");
    g_rccl.lib = lib;
    return 0;
}
#define SERT_NCCL(expr)                                                                       \
    do {                                                                                      \
        int _r = (expr);                                                                      \
        if (_r != 0)                                                                          \
            SERT_FAIL(std::string(#expr) + ": " +                                             \
                      (g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "rccl error"));    \
    } while (0)

// ---- small helpers -----------------------------------------------------------
// (dmalloc and the grow-only DevBuf: common.h)
template <typename T>
static int dzalloc(T** p, size_t count, hipStream_t s) {
    SERT_TRY(dmalloc(p, count));
    if (count) SERT_HIP(hipMemsetAsync(*p, 0, count * sizeof(T), s));
    return 0;
}
static inline int grid_for(int64_t work_items, int block = 256, int cap = 256 * 8) {
    int64_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
static inline size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// vectorspace-shaped parameters (R_e, projection W/b): both the reference's NCE
// model and the additive full-softmax variant
static bool is_vs(const sert_model* m) { return m->cfg.kind != SERT_KIND_LOGLINEAR; }
static bool is_fs(const sert_model* m) { return m->cfg.kind == SERT_KIND_VECTORSPACE_SOFTMAX; }
// drop whatever a previous training call ran ahead for the next one (sert_hint_next_batch)
static void discard_run_ahead(sert_model* m) {
    if (m->spec_fb_batch >= 0) ++m->state_counts[0];
    if (m->spec_fb_batch >= 0 && m->stream2 && m->ev_join) {
        // a discarded run-ahead may still be busy on the side stream (its entity chain is only
        // joined by the update that will now never come): order the main stream behind it
        // before anything reuses the buffers it reads and writes
        (void)hipEventRecord(m->ev_join, m->stream2);
        (void)hipStreamWaitEvent(m->stream, m->ev_join, 0);
    }
    m->spec_fb_batch = -1;
}
static int ensure_rw_current(sert_model* m, int64_t batch, int64_t t_applied = -1);
static bool egrad_writes_every_row(const sert_model* m);
static void invalidate_speculation(sert_model* m) {
    discard_run_ahead(m);
    (void)ensure_rw_current(m, -1);   // (whatever comes next -- new parameters, another step counter, new data -- sees every row current)
    if (m->re_pending) {       // (a deferred entity-table update: see settle_entity_update)
        (void)hipStreamWaitEvent(m->stream, m->ev_re, 0);
        m->re_pending = false;
        ++m->state_counts[3];
    }
    m->re_sq_for[0] = m->re_sq_for[1] = -1;
    m->projected_batch = -1;
    m->neg_alt_step = -1;      // (step counter, seed-relevant state or data may change)
    m->rw_pred_ok = false;     // (the rows' predicted shares of sum(p^2) are trajectories of THESE parameters and THIS step counter)
}

#include "host/timing.inc"

#include "host/lazy_segsum.inc"

#include "host/data_parallel.inc"

#include "host/step_vectorspace.inc"

#include "host/step_softmax_loglinear.inc"

#include "host/optimizer_and_loss.inc"

#include "host/rank_rows.inc"

#include "host/rank_lists.inc"   // (behind rank_rows.inc, in front of its two callers api_scorer_rerank.inc / api_ll_rerank.inc)

}  // namespace sert

using namespace sert;

// =============================== C ABI ===========================================
extern "C" {

#include "host/api_model.inc"

#include "host/api_data_train.inc"

#include "host/api_scorer.inc"

#include "host/api_ll_rank.inc"

#include "host/api_scorer_rank.inc"

#include "host/api_scorer_rerank.inc"

#include "host/api_ll_rerank.inc"

#include "host/api_reval.inc"

#include "host/foldin_common.inc"   // (in front of its four callers api_foldin.inc / api_ll_foldin.inc / api_wfold.inc / api_ll_wfold.inc)

#include "host/api_foldin.inc"

#include "host/api_ll_foldin.inc"

#include "host/api_wfold.inc"

#include "host/api_ll_wfold.inc"

#include "host/api_comm.inc"

#include "host/api_debug.inc"

}  // extern "C"


#ifdef SR_TIMELINE
extern "C" int sert_debug_read(void* out, size_t bytes) {
    (void)hipDeviceSynchronize();
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sert::sr_dbg), bytes, 0, hipMemcpyDeviceToHost);
}
#endif
