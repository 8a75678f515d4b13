// The schedule of the vectorspace training step, as a value.
//
// Which queue every launch of the backward and of the update goes to, in what order, which kernel's completion carries the
// fork and who joins whom is decided HERE, once per step, by one pure function of a plain struct of facts:
//   VsStepFacts  everything the schedule depends on (host/step_vectorspace.inc: vs_step_facts fills it from the model)
//   VsStepPlan   the decisions (sert_model::plan; the step's host code issues what it says and tests nothing else)
//   vs_plan_step the function between them
// Host only: no HIP, no model -- tests/test_step_plan_cpu.py pins the plan of every schedule through
// sert_debug_vs_plan_for (include/sert_hip_debug.h) without a GPU.  Both structs are rows of int32_t in the order of that
// header's SERT_VS_FACT_* / SERT_VS_PLAN_* indices, so that the hook is a copy.
#pragma once
#include <stdint.h>
#include "../../include/sert_hip_debug.h"

namespace sert {

// The knobs of the schedule, read once per process (host/step_vectorspace.inc: vs_knobs).  SERT_SIDE_HEAVY and SERT_RE_DEFER
// are product knobs (knob()); the others exist in a variants build only (variant_knob(): constants in the product build).
struct VsKnobs {
    int32_t ext_events = 1;       // SERT_EXT_EVENTS=0: plain hipEventRecord behind a kernel instead of its completion signal
    int32_t fork_late = 1;        // SERT_FORK_LATE=0: the fork right behind the NCE kernel with dW on the main queue
    int32_t fork_at = 0;          // SERT_FORK_AT: 0 unset, 1 "nce...", 2 "nce_dw"
    int32_t side_heavy = 1;       // SERT_SIDE_HEAVY: 0 off, 1 big entity tables, 2 small ones too
    int32_t re_defer = 1;         // SERT_RE_DEFER=0: no entity-table update behind the tail
    int32_t early_bucket = -1;    // SERT_EARLY_BUCKET: -1 unset (by batch size), 0 off, 1 on
    int32_t no_early_bucket = 0;  // SERT_NO_EARLY_BUCKET
    int32_t early_sort = 0;       // SERT_EARLY_SORT=1: whatever the size of dh
    int32_t no_early_sort = 0;    // SERT_NO_EARLY_SORT
    int32_t dw_first = -1;        // SERT_DW_FIRST: -1 unset (by size of dh), 0 never, 2 always
    int32_t dp_late = 1;          // SERT_DP_LATE=0: the main queue joins the side queue in a data-parallel step too
    int32_t no_tail = 0;          // SERT_NO_TAIL: the split-K combine and the W, b update as launches of their own
    int32_t egrad_group_sum = 0;  // SERT_EGRAD_GROUP_SUM: egrad_group_sum sums the row groups' tables, not the optimiser
    int32_t bwd_fused = 0;        // SERT_BWD_FUSED=1: dh and dW's partial slabs in one launch where the shape allows
};

struct VsStepFacts {
    int32_t kind = 0;             // SERT_KIND_*
    int32_t host_ar = 0, comm = 0;   // data parallel over the host transport / over a communicator
    int32_t timing = 0;           // timing.enabled (mode 1: every kernel group alone on the main queue)
    int32_t nstreams = 2;
    int32_t n_re = 0;             // elements of R_e (saturated at INT32_MAX)
    int32_t big_re = 0, big_w = 0;   // pt_big[1], pt_big[2]: a streaming optimiser launch of its own
    int32_t keep_grads = 0;
    int32_t batch = 0, word_dim = 0, entity_dim = 0, num_negatives = 0;
    int32_t has_entities = 0;     // num_entities > 0
    int32_t sort_free = 0;        // the sort-free entity chain (epart != nullptr)
    int32_t cand_early = 0;       // the early sort's key buffer exists
    int32_t neg_side_ready = 0;   // this step's negatives were drawn on the side queue during the previous step
    int32_t has_labels = 0;
    int32_t next_neg_drawn = 0;   // neg_alt_step == step + 1
    int32_t dh_strip = 0;         // variants build: the dh GEMM is the strip kernel (launched without a completion event)
    int32_t bwd_fused_shape = 0;  // variants build: shape and scratch admit vs_bwd_fused
    VsKnobs k;
    bool dp() const { return host_ar || comm; }
};
static_assert(sizeof(VsStepFacts) == SERT_VS_FACT_COUNT * sizeof(int32_t), "VsStepFacts is the row of SERT_VS_FACT_* (sert_hip_debug.h)");

struct VsStepPlan {
    // ---- the fork
    int32_t fork_at = SERT_VS_FORK_NONE;   // the kernel behind which the side queue starts its chain
    int32_t fork_carried = 0;     // that kernel's own completion signal is ev_fork (CarriedEvent) ...
    int32_t fork_recorded = 0;    // ... or, behind the loss kernel, hipEventRecord(ev_fork) on the main queue: where the side queue meets
                                  // the fork in front of the pieces (side_meets_fork), else at the head of the entity chain
    int32_t dh_event = SERT_VS_EVENT_NONE;   // what the end of the dh GEMM marks: ev_fork, ev_dense or nothing
    int32_t dh_carried = 0;       // by its completion signal (else a hipEventRecord behind it)
    // ---- the four pieces of the backward
    int32_t order[4] = {SERT_VS_PIECE_ENTITY, SERT_VS_PIECE_DENSE, SERT_VS_PIECE_DH, SERT_VS_PIECE_WORD_SUM};
    int32_t entity_queue = SERT_VS_QUEUE_MAIN, dense_queue = SERT_VS_QUEUE_MAIN;
    int32_t side_meets_fork = 0;  // the side queue waits for ev_fork in front of the pieces
    int32_t entity_waits_fork = 0;   // the entity chain's queue waits for ev_fork at its head
    int32_t dense_event = SERT_VS_EVENT_NONE;   // what the dense gradients record behind themselves: ev_dense (the tail waits for
                                  // it), ev_join3 (a third queue: it met ev_fork first, the main queue waits at the end) or nothing
    int32_t bwd_fused = 0;        // variants build: the dh launch is vs_bwd_fused, the dense gradients only combine its slabs
    // ---- early work on the side queue, in front of its fork wait
    int32_t bucket_early = 0, sort_early = 0;
    int32_t draw_next_neg = 0;    // the next step's negatives
    // ---- joins
    int32_t lazy_join = 0;        // the main queue never waits for the entity chain (for the record: the launch sites read what follows
                                  // from it -- end_join, dh_event, small_order)
    int32_t end_join = 0;         // the main queue joins the side queue (ev_join) at the end of the backward
    int32_t dp_late_join = 0;     // the communication queue does, in front of the small all-reduce (allreduce_rest)
    // ---- dW's split-K combine and dR_e
    int32_t combine_in_tail = 0;  // the combine rides in the tail launch with the W, b update and the loss
    int32_t re_in_parts = 0;      // dR_e stays the row groups' tables (the small-tensor optimiser adds them)
    // ---- the update
    int32_t side_small = 0;       // the small tensors are updated on the side queue
    int32_t small_order = SERT_VS_EVENT_NONE;   // what orders the side queue in front of them: nothing, ev_dense, ev_opt_fork
    int32_t split_small = 0;      // W, b in a launch of their own on the main queue, R_e on the side queue (not where the tail updates W, b)
    int32_t defer_re = 0;         // a big R_e streams behind the tail's join
    int32_t defer_small = 0;      // a small R_e is not joined by the tail (while the previous step left its sums of squares)
    int32_t re_on_side = 0;       // a big R_e streams on the side queue
};
static_assert(sizeof(VsStepPlan) == SERT_VS_PLAN_COUNT * sizeof(int32_t), "VsStepPlan is the row of SERT_VS_PLAN_* (sert_hip_debug.h)");

inline VsStepPlan vs_plan_step(const VsStepFacts& f) {
    VsStepPlan p;
    const VsKnobs& k = f.k;
    const bool dp = f.dp(), timing = f.timing != 0;
    const bool two = !timing && f.nstreams >= 2;        // a side queue is in use at all
    // Full softmax: the whole backward on the main queue; only the small tensors are updated on the side queue, forked
    // and joined around them.  (Loglinear: host/step_softmax_loglinear.inc decides for itself, ll_dw_side.)
    if (f.kind == SERT_KIND_VECTORSPACE_SOFTMAX && !dp && two) {
        p.side_small = 1;
        p.small_order = SERT_VS_EVENT_OPT_FORK;
    }
    if (f.kind != SERT_KIND_VECTORSPACE) return p;
    const bool ext = k.ext_events != 0;
    const bool re_small = f.n_re <= (1 << 22);
    const int64_t dh_bytes = (int64_t)f.batch * f.word_dim * (int64_t)sizeof(float);
    // Single GPU, BIG entity table (more than 2^22 elements: the sorted entity-gradient chain and a streaming
    // optimiser launch of its own -- C4): the main stream keeps nothing but the critical chain
    //   loss -> dh GEMM -> segmented sum -> word-table optimiser -> tail,
    // the side stream takes, forked on the loss kernel,
    //   entity chain -> entity-table optimiser -> dW GEMM,
    // and is joined in front of the tail.  The MFMA-bound dW (off the critical path: it only feeds the tail)
    // and the 0.96 GB of the entity table's optimiser then run BESIDE the 750 us the word table streams,
    // instead of in front of and behind it.  SERT_SIDE_HEAVY=0 restores dW in front of dh on the main stream
    // and both optimiser launches behind the join; 2: small entity tables too.
    const bool side_heavy = k.side_heavy > 0 && ext && !dp && !timing && f.nstreams == 2 && (f.big_re || k.side_heavy > 1) &&
                            !f.big_w && !f.keep_grads;
    // Single GPU, two streams: ONE fork per step, behind the dh GEMM (the last reader of W): the side
    // stream then takes the entity chain, dW / db and the small-tensor optimiser in a row with no
    // further event, the main stream keeps loss -> dh -> segmented sum -> word-table optimiser.
    // Every cross-queue event costs its queue ~5-7 us (the kernel that carries a completion signal
    // ends with a cache write-back): two per step instead of three.  SERT_FORK_LATE=0 restores the
    // fork right behind the NCE kernel with dW on the main stream.
    const bool fork_late = k.fork_late && !side_heavy && ext && !dp && !timing && f.nstreams == 2 && re_small;
    // Where the one fork of the late-fork schedule sits: behind the dh GEMM (default) or, SERT_FORK_AT=nce,
    // behind the NCE kernel -- W and b are updated on the main stream, so nothing on the side stream
    // has to wait for the last reader of W any more, and the entity chain then runs beside the
    // MFMA-bound dh / dW GEMMs instead of beside the cache-bound segmented sum.
    const bool fork_nce = fork_late && k.fork_at >= 1;
    // On a single GPU the only consumer of dR_e is the small-tensor optimiser, which runs on
    // the side stream right behind the entity chain: the main stream then never waits for
    // that chain, and the word-table optimiser starts straight after segsum instead of
    // idling ~12 us on a cross-queue dependency.
    const bool lazy_join = !dp && !timing && f.nstreams == 2 && (re_small || side_heavy);
    // dh and dW (+ db) of the projection in one launch (variants/gemm_bwd_fused.h) where the shape allows it.
    // opt-in (SERT_BWD_FUSED=1): measured EQUAL to the two gemm.h launches at C2 (57.5 us against 29.3 + 29.2;
    // step 0.3030 against 0.3046 ms, inside the run-to-run spread) -- the fused kernel keeps the matrix pipe as
    // busy as they do (48 %), it only saves a launch and half of the partial slabs
    const bool fused_bwd = k.bwd_fused && f.bwd_fused_shape && f.nstreams < 3 && !side_heavy;

    // ---- early work: in front of the side queue's fork wait, beside gather / projection / loss
    // Round 6: the PARTITION of this step's (pair, entity) keys by entity range (egrad_bucket, 19 us at C2) needs the
    // labels and the negatives only -- not the loss kernel's coefficients -- and this step's negatives were drawn on the
    // side stream during the previous step (neg_side_ready): it goes out in front of the fork as well.  The chain behind
    // the fork is then egrad_acc alone: it starts 19 us earlier and ends that much earlier beside the word table's update
    // (profiles/r06_experiments.txt, item 1).
    // Measured (tools/experiments/r06_early_bucket.sh, r06_fork_nce_early.sh; three rounds each on one box, ms/step early / behind
    // the fork): batch 32768 0.1426-0.1466 / 0.1515-0.1552 (-5.5 %), 65536 0.2404-0.2427 / 0.2404-0.2426 (equal: egrad_acc ends
    // 29 us earlier, the tree beside it stretches by 5), 16384 0.1182-0.1213 / 0.1170-0.1184 (+1.5 %), 8192 0.0977-0.1000 /
    // 0.0938-0.0966 (+3-5 %: there the partition beside the forward delays the loss kernel and the update): from batch 32768.
    // SERT_EARLY_BUCKET=0 / 1 (variants build) forces it off / on.
    const bool want_bucket = k.early_bucket >= 0 ? k.early_bucket != 0 : f.batch >= 32768;
    const bool keys_ready = f.num_negatives > 0 && f.neg_side_ready && f.has_labels;
    p.bucket_early = !k.no_early_bucket && want_bucket && fork_late && f.sort_free && keys_ready;
    // ... and the same for the SORTED entity chain of a larger entity table (V_e > 2048: the reference's product-search
    // settings, C4): the stable counting sort of the (entity, pair) keys -- six of the chain's eight launches.
    // Measured (tools/experiments/r06_early_sort.sh, r06_early_sort_sizes.sh; two to three rounds each on one box; ms/step beside the
    // forward / inside the chain): the reference's product-search settings (batch 4096, V_e 32768, d_w 300) 0.1669-0.1689 / 0.1696-0.1727,
    // the same at batch 1024 0.1434-0.1443 / 0.1513-0.1527; d = 128, V_e 32768: batch 16384 0.1514-0.1529 / 0.1717-0.1727 (-12 %), 32768
    // 0.2034-0.2049 / 0.2255-0.2279, 65536 0.3227-0.3253 / 0.3434-0.3457; V_e 100000: batch 65536 at d = 128 0.4099-0.4140 / 0.4319-0.4355,
    // d = 300: batch 16384 0.705-0.714 / 0.709-0.717, 32768 0.865-0.920 / 0.906-0.954 -- but C4 itself (batch 65536, d = 300) 1.404-1.411 /
    // 1.360-1.364: there the chunked reduce (865 MB of row fetches) then starts beside the word gradient's tree (680 MB of them) instead of
    // beside the update, and the tree takes 389 us instead of 125.  Taken while dh, the tree's source, is below 64 MB.
    // SERT_EARLY_SORT=1 (variants build) forces it, SERT_NO_EARLY_SORT=1 switches it off.
    p.sort_early = (k.early_sort || dh_bytes < ((int64_t)64 << 20)) && !k.no_early_sort && !f.sort_free && f.cand_early && !dp && two &&
                   keys_ready && f.has_entities;

    // ---- dW / db: which queue, and where in its chain
    // SERT_FORK_AT=nce_dw: ... and the side stream starts with dW, db and the loss partials -- beside the dh GEMM (both
    // 512-workgroup MFMA launches that leave half the matrix pipe idle on their own) -- and only then takes the entity chain,
    // which then runs beside the segmented sum as in the default schedule.
    // (!big_w: a projection matrix large enough for a streaming update of its own is updated on the main stream, which
    //  would then have to wait for the side stream's dW)
    const bool dw_side_ok = lazy_join && !fused_bwd && !f.big_w;
    const bool fork_nce_dw = fork_nce && k.fork_at == 2 && dw_side_ok;
    // Single GPU, late fork: dW, db (and the loss partials) only feed the tail.  FIRST on the side stream -- in front of the
    // entity chain, beside the segmented sum -- they leave the main stream's dependency chain (loss -> dh -> segmented sum
    // -> word-table update -> tail) 20 us shorter; the tail waits for their event, which is long complete by then.
    // Measured (tools/experiments/r04_dw_first*.sh, C2 dims): batch 4096 0.1176 -> 0.1092 ms, 8192 0.130 -> 0.116, 16384 0.1566 ->
    // 0.1429, 32768 0.191 -> 0.175; at 65536 0.2720 -> 0.2745 -- there dW streams its 67 MB beside the first level of the
    // segmented sum, whose 33.5 MB of dh rows then no longer stay in the Infinity Cache.  Taken while dh is at or below 24 MB.
    // Round 6: the entity keys' partition goes out first of all on the side stream, in front of the fork wait (bucket_early) --
    // and where it does, dW / db first on the side stream pays at EVERY batch size: the chain behind the fork is then dW + egrad_acc,
    // the main stream goes from dh straight into the tree.  tools/experiments/r06_dw_first_again.sh, three rounds on one box, ms/step,
    // dW on the main stream / first on the side stream: batch 65536 0.2375-0.2390 / 0.2244-0.2261 (-5.4 %; with the partition behind the
    // fork, as in round 5: 0.2381-0.2404 / 0.2346-0.2360), 131072 0.4190-0.4222 / 0.4040-0.4142.
    // (sort_free: the sort-free entity chain of small entity tables.  Behind the counting sort of a larger one the side stream is
    //  the longer of the two already: the reference's product-search settings, V_e = 32768, 205.8 -> 214.5 us with dW in front)
    const bool dw_side_first = fork_nce_dw ||
                               (k.dw_first != 0 && fork_late && !fork_nce && dw_side_ok &&
                                (k.dw_first == 2 || ((dh_bytes <= ((int64_t)24 << 20) || p.bucket_early) && f.sort_free)));
    // Data parallel over an asynchronous communicator: nothing on the main stream needs what the side stream produces
    // (dR_e, and -- issued there too -- dW, db and the loss sum) before the all-reduce of the replicated remainder, and
    // that runs on the communication stream.  So the communication stream joins the side stream (allreduce_rest), the main
    // stream goes from the segmented sum straight to the hand-over of the word rows and their update: 40 us of dW GEMM,
    // combine and loss sum leave the critical path (C2, world of one: 0.329 -> 0.29 ms)
    const bool dp_late = k.dp_late && dp && !f.host_ar && f.comm && !timing && f.nstreams == 2;

    // ---- the fork and the event of the dh GEMM
    // (the loss kernel carries ev_fork wherever the fork is not the late one, data parallel and three queues included;
    //  entity_dim % 4: the kernels that have always carried it)
    const bool nce_carries = ext && (!fork_late || fork_nce) && two && f.entity_dim % 4 == 0;
    // (the end of the dh GEMM: from there on the main stream has produced dW, db and the loss partials AND is done
    //  READING W -- the side stream may update the small tensors)
    if (lazy_join && !fork_nce) {
        p.dh_event = fork_late ? SERT_VS_EVENT_FORK : SERT_VS_EVENT_DENSE;
        p.dh_carried = ext && !f.dh_strip;
    }
    if (fork_late && !fork_nce) {
        p.fork_at = SERT_VS_FORK_DH;
        p.fork_carried = p.dh_carried;
    } else {
        // (one queue or timing mode: nothing forks, the entity chain still records the event)
        p.fork_at = two ? SERT_VS_FORK_LOSS : SERT_VS_FORK_NONE;
        p.fork_carried = nce_carries;
        p.fork_recorded = !nce_carries;
        // (nce_dw, dp_late: the side queue meets the fork in front of dW; the entity chain behind it follows in queue order --
        //  but the data-parallel one waits for the event once more, as it always has)
        p.side_meets_fork = fork_nce_dw || dp_late;
        p.entity_waits_fork = two && !dw_side_first;
    }
    // The NEXT step's negatives (Philox position = the step counter after this step's update) are drawn while the side
    // stream still idles in front of the late fork (host/step_vectorspace.inc: vs_dh_gemm)
    p.draw_next_neg = p.fork_at == SERT_VS_FORK_DH && f.sort_free && f.num_negatives > 0 && !f.next_neg_drawn;

    // ---- queues and order
    p.entity_queue = two ? SERT_VS_QUEUE_SIDE : SERT_VS_QUEUE_MAIN;
    // Third stream: dW and dh are both 512-workgroup launches (2 waves per SIMD, too few to hide their own latencies) --
    // side by side they fill each other's bubbles.  (side_heavy: on the side stream behind the entity chain)
    p.dense_queue = (side_heavy || dp_late || dw_side_first) ? SERT_VS_QUEUE_SIDE
                    : (!timing && f.nstreams >= 3)           ? SERT_VS_QUEUE_THIRD
                                                             : SERT_VS_QUEUE_MAIN;
    p.dense_event = dw_side_first ? SERT_VS_EVENT_DENSE : p.dense_queue == SERT_VS_QUEUE_THIRD ? SERT_VS_EVENT_JOIN3 : SERT_VS_EVENT_NONE;
    p.bwd_fused = fused_bwd;
    enum { E = SERT_VS_PIECE_ENTITY, H = SERT_VS_PIECE_DH, D = SERT_VS_PIECE_DENSE, S = SERT_VS_PIECE_WORD_SUM };
    auto order = [&p](int a, int b, int c, int d) { p.order[0] = a; p.order[1] = b; p.order[2] = c; p.order[3] = d; };
    if (side_heavy) order(E, H, S, D);        // entity: side, forked on the loss kernel; dh, sum: main; dW: side, behind the chain
    else if (fork_nce_dw) order(H, D, E, S);  // dW: side, beside the dh GEMM; entity: side, behind dW
    else if (fork_nce) order(E, H, D, S);     // entity: side, forked on the loss kernel
    else if (fork_late && dw_side_first) order(H, D, E, S);   // dh's completion is the step's one fork; dW: side, in front of the chain
    else if (fork_late) order(H, E, D, S);    // dW: main (W and b are then updated on the main stream too)
    // data parallel: the word-table gradient first, so that its exchange (rows' all-to-all or
    // reduce-scatter) overlaps dW and the entity chain (dW in front of the segmented sum instead:
    // 0.362 -> 0.370 ms with a world of one -- the hand-over then sits bare on the critical path).
    // dp_late: the side stream takes dW, db and the loss sum FIRST (beside dh and the segmented sum), then the entity chain:
    // behind that chain they ran beside the word table's Adam, three times as long, and the small all-reduce --
    // which waits for them -- ended 35 us after the Adam (0.330 ms; this order: 0.29).
    // The data-parallel step is bound by the HOST (some 45 runtime calls + three collectives per step: round-5 API
    // trace, tools/experiments/r05_hip_trace.sh with SERT_FORCE_COMM=1): the launches go out in order of
    // criticality -- the main stream's dh GEMM first; issued behind the six side-stream launches it started 27 us
    // after the loss kernel had finished (C2, world of one).
    else if (dp_late) order(H, D, E, S);
    else if (dp) order(E, H, S, D);
    else if (fused_bwd) order(E, H, D, S);    // (dh and the dW partials in one launch)
    else order(E, D, H, S);                   // single GPU: the MFMA-bound dW beside the latency-bound sort of the side stream

    // ---- joins
    p.lazy_join = lazy_join;
    p.dp_late_join = dp_late;
    p.end_join = !lazy_join && !dp_late && two;

    // ---- dW's combine, dR_e
    // single GPU: the combine rides in the step's tail launch (vs_tail) with the W, b update and the loss finalisation
    // (side_heavy, dW first: the partial slabs come from the side stream, which the tail waits for)
    p.combine_in_tail = !k.no_tail && !dp && p.dense_queue != SERT_VS_QUEUE_THIRD && !f.big_w &&
                        (int64_t)f.word_dim * f.entity_dim + f.entity_dim < ((int64_t)1 << 31);
    // Single GPU: the only reader of dR_e is the small-tensor optimiser, which adds the row
    // groups' tables itself (same order) -- no launch for the sum.  Data parallel: the all-reduce needs the summed table.
    p.re_in_parts = f.sort_free && !dp && !f.big_re && !k.egrad_group_sum;

    // ---- the update (host/optimizer_and_loss.inc)
    // single GPU: the small tensors are updated on the side stream WHILE the word table streams on the main one
    p.side_small = !dp && two;
    // Late fork: everything the small tensors need was issued on the side stream itself; dW / db were produced on the main
    // stream, dR_e on the side stream -- W and b are updated on the main stream (by the tail, or a launch of their own), R_e
    // on the side stream, no event between.
    p.small_order = !p.side_small ? SERT_VS_EVENT_NONE : !lazy_join ? SERT_VS_EVENT_OPT_FORK : fork_late ? SERT_VS_EVENT_NONE : SERT_VS_EVENT_DENSE;
    p.split_small = p.side_small && fork_late && !p.combine_in_tail;
    // side-heavy schedule: the entity table is updated BEHIND the join of the tail, and so is a SMALL entity table
    // behind the late fork (host/optimizer_and_loss.inc has the measurements)
    const bool may_defer = k.re_defer && p.side_small && p.combine_in_tail && !f.keep_grads;
    p.defer_re = may_defer && side_heavy && f.big_re;
    p.defer_small = may_defer && !p.defer_re && !f.big_re && fork_late && f.n_re > 0;
    p.re_on_side = p.side_small && side_heavy && f.big_re;
    return p;
}

}  // namespace sert
