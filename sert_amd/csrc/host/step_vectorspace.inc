// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): the vectorspace step: negatives, projection, loss, backward and its two-queue schedule.

// ---- the vectorspace step -----------------------------------------------------
static int reduce_rowloss(sert_model* m, hipStream_t st);

static int vs_negatives(sert_model* m, const int64_t* negatives, uint64_t stream_pos, hipStream_t st) {
    const auto& c = m->cfg;
    const int64_t count = (int64_t)c.batch_size * c.num_negatives;
    if (count == 0) return 0;
    if (negatives) {
        // (parity path: the device sampler cannot produce an id outside [0, V_e))
        const int64_t Ve = c.num_entities;
        for (int64_t i = 0; i < count; ++i)
            if (negatives[i] < 0 || negatives[i] >= Ve) SERT_FAIL("negative sample out of range [0, num_entities)");
        SERT_HIP(hipMemcpyAsync(m->neg_stage, negatives, count * sizeof(int64_t),
                                hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(convert_i64_to_i32, dim3(grid_for(count)), dim3(256), 0, st,
                           m->neg_stage, m->neg, count);
    } else {
        const int64_t global_offset = (int64_t)m->rank * count;
        // Philox stream position: even = training draws, odd = evaluation draws
        // (the reference keeps two independent RandomStreams, models.py:745-752).
        hipLaunchKernelGGL(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0,
                           st, m->neg, count, global_offset, (uint32_t)c.num_entities,
                           c.seed, stream_pos);
    }
    return 0;
}

// A deferred tail (optimizer_and_loss) that no gather launch carried: the plain vs_tail, now.  In front of anything that
// reads W or b, and before the host waits for the step's loss.
static void flush_pending_tail(sert_model* m) {
    if (!m->tail_pending) return;
    m->tail_pending = false;
    ScopedTimer t(m, TG_FINALIZE);
    ++m->tail_counts[0];
    hipLaunchKernelGGL((vs_tail<false>), dim3(m->tail_nb), dim3(1024), 0, m->stream, m->tail_args);
}

// gather + mean-pool + projection: needs neither the negatives nor the gradient buffers
static int vs_project(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, dw = c.word_dim, de = c.entity_dim;
    const size_t row0 = (size_t)batch_index * B;
    // gather + mean-pool + projection in ONE launch where the shape allows it (kernels_proj.h: d_w, d_e <= 128, window <= 10):
    // the h and the t of the two launches below, bit for bit where they run gemm_x3.  OPT-IN, SERT_PROJ_FUSED=1 (read at
    // sert_create, VARIANTS BUILD ONLY since round 6): round 5 measured it slower than the two launches at C2 and equal at 8192
    // rows.  SERT_GEMM_FP32=1 (the fused kernel multiplies on the bf16 pipe) keeps the two launches too.
#ifdef SERT_VARIANTS
    if (m->proj_fused && gemm_x3_enabled() && vs_project_fused_ok(B, n, dw, de, m->n_rw)) {
        flush_pending_tail(m);
        if (m->T_alt) std::swap(m->T, m->T_alt);     // (see below: this projection goes to the other buffer)
        ScopedTimer t(m, TG_GATHER);
        SERT_ID_DISPATCH(c.id_bytes, {
            const IdT* X = (const IdT*)ds.x + row0 * n;
            hipLaunchKernelGGL((vs_project_x3<IdT>), dim3(vs_project_grid(B, m->num_cus)), dim3(PJ_THREADS), 0, m->stream, X, (const float*)m->rw,
                               (const float*)m->W, (const float*)m->b, m->H, m->T, B, n, dw, de);
        });
        return 0;
    }
#endif
    {
        ScopedTimer t(m, TG_GATHER);
        SERT_ID_DISPATCH(c.id_bytes, {
            const IdT* X = (const IdT*)ds.x + row0 * n;
            // the batch's hot rows from LDS (kernels_vs.h: vs_gather_mean_hot; training batches with an index and dense words).
            // OPT-IN in a VARIANTS BUILD, SERT_GATHER_HOT=1 (read at upload: the slot bytes exist only then): same h bit for bit, measured SLOWER --
            // profiles/r05_experiments.txt, item 32.
#ifdef SERT_VARIANTS
            const int nhot = (ds.idx_tok_slot && (size_t)batch_index < ds.dense_cnt_of.size()) ? ds.dense_cnt_of[(size_t)batch_index] : 0;
            if (dw % 4 == 0 && nhot > 0 && (size_t)nhot * dw * sizeof(float) <= 48 * 1024) {
                flush_pending_tail(m);
                hipLaunchKernelGGL((vs_gather_mean_hot<IdT>), dim3(std::min<int64_t>(grid_for((int64_t)B * dw / 4, 256, 1 << 20), 8 * m->num_cus)),
                                   dim3(256), (size_t)nhot * dw * sizeof(float), m->stream, X, (const uint8_t*)ds.idx_tok_slot + row0 * n,
                                   (const int32_t*)ds.idx_dense_words + (size_t)batch_index * kHeavyMax, nhot, (const float*)m->rw, m->H, B, n, dw);
            } else
#endif
            if (dw % 4 == 0 && m->tail_pending) {
                // the previous step's tail: the leading workgroups of this launch (kernels_vs.h: vs_gather_mean_tail)
                m->tail_pending = false;
                ++m->tail_counts[1];
                hipLaunchKernelGGL((vs_gather_mean_tail<IdT>), dim3(m->tail_nb + grid_for((int64_t)B * dw / 4, 256, 1 << 20)),
                                   dim3(256), 0, m->stream, X, m->rw, m->H, B, n, dw, m->tail_args, (unsigned)m->tail_nb);
            } else if (dw % 4 == 0) {
                hipLaunchKernelGGL((vs_gather_mean<IdT, 4>), dim3(grid_for((int64_t)B * dw / 4, 256, 1 << 20)),
                                   dim3(256), 0, m->stream, X, m->rw, m->H, B, n, dw);
            } else {
                flush_pending_tail(m);
                hipLaunchKernelGGL((vs_gather_mean<IdT, 1>), dim3(grid_for((int64_t)B * dw, 256, 1 << 20)),
                                   dim3(256), 0, m->stream, X, m->rw, m->H, B, n, dw);
            }
        });
    }
    // The entity-gradient chain of the PREVIOUS step reads that step's projection rows on the side stream, and the main stream
    // no longer joins that stream at the end of a step (only the next LOSS kernel waits for it, settle_entity_update): this
    // projection goes to the other buffer.  (One buffer was a race the schedule merely kept from happening -- at C2 the
    // chain ends 15 us before the step does; small batches with the chain longer than the rest of the step lost it.)
    if (m->T_alt) std::swap(m->T, m->T_alt);
    {
        ScopedTimer t(m, TG_GEMM_FWD);
        // t = tanh(h.W + b)   (models.py:1057-1061)
#ifdef SERT_VARIANTS
        if (gemm_strip_ok(B, de, dw, dw, de, false, m->H, m->W))
            launch_gemm_strip<false, EPI_BIAS_TANH>(m->stream, m->H, m->W, m->T, m->b, B, de, dw, dw, de, de);
        else
#endif
            launch_gemm<false, false, EPI_BIAS_TANH>(m->stream, m->H, m->W, m->T, m->b, B, de, dw, dw,
                                                     de, de);
    }
    return 0;
}

// Events that mark the end of ONE kernel ride on that kernel's completion signal
// (SERT_EXT_EVENTS=0: plain hipEventRecord behind it, ~7 us of queue stall each).
static bool ext_events() {
    static const bool on = !(variant_knob("SERT_EXT_EVENTS") && atoi(variant_knob("SERT_EXT_EVENTS")) == 0);
    return on;
}

// Single GPU, two streams: ONE fork per step, behind the dh GEMM (the last reader of W): the side
// stream then takes the entity chain, dW / db and the small-tensor optimiser in a row with no
// further event, the main stream keeps loss -> dh -> segmented sum -> word-table optimiser.
// Every cross-queue event costs its queue ~5-7 us (the kernel that carries a completion signal
// ends with a cache write-back): two per step instead of three.  SERT_FORK_LATE=0 restores the
// fork right behind the NCE kernel with dW on the main stream.
static bool side_heavy_mode(const sert_model* m);

static bool fork_late_mode(const sert_model* m) {
    static const bool on = !(variant_knob("SERT_FORK_LATE") && atoi(variant_knob("SERT_FORK_LATE")) == 0);
    return on && !side_heavy_mode(m) && ext_events() && !is_dp(m) && !m->timing.enabled && m->nstreams == 2 &&
           m->n_re <= ((size_t)1 << 22) && m->cfg.kind == SERT_KIND_VECTORSPACE;
}

// Where the one fork of fork_late_mode sits: behind the dh GEMM (default) or, SERT_FORK_AT=nce,
// behind the NCE kernel -- W and b are updated on the main stream, so nothing on the side stream
// has to wait for the last reader of W any more, and the entity chain then runs beside the
// MFMA-bound dh / dW GEMMs instead of beside the cache-bound segmented sum.
static bool fork_at_nce(const sert_model* m) {
    static const bool on = variant_knob("SERT_FORK_AT") && !strncmp(variant_knob("SERT_FORK_AT"), "nce", 3);
    return on && fork_late_mode(m);
}
// SERT_FORK_AT=nce_dw: ... and the side stream starts with dW, db and the loss partials -- beside the dh GEMM (both
// 512-workgroup MFMA launches that leave half the matrix pipe idle on their own) -- and only then takes the entity chain,
// which then runs beside the segmented sum as in the default schedule.
static bool fork_at_nce_dw(const sert_model* m) {
    static const bool on = variant_knob("SERT_FORK_AT") && !strcmp(variant_knob("SERT_FORK_AT"), "nce_dw");
    return on && fork_at_nce(m);
}

// Single GPU, BIG entity table (more than 2^22 elements: the sorted entity-gradient chain and a streaming
// optimiser launch of its own -- C4): the main stream keeps nothing but the critical chain
//   loss -> dh GEMM -> segmented sum -> word-table optimiser -> tail,
// the side stream takes, forked on the loss kernel,
//   entity chain -> entity-table optimiser -> dW GEMM,
// and is joined in front of the tail.  The MFMA-bound dW (off the critical path: it only feeds the tail)
// and the 0.96 GB of the entity table's optimiser then run BESIDE the 750 us the word table streams,
// instead of in front of and behind it.  SERT_SIDE_HEAVY=0 restores dW in front of dh on the main stream
// and both optimiser launches behind the join.
static bool side_heavy_mode(const sert_model* m) {
    static const int level = knob("SERT_SIDE_HEAVY") ? atoi(knob("SERT_SIDE_HEAVY")) : 1;   // 2: small entity tables too
    return level > 0 && ext_events() && !is_dp(m) && !m->timing.enabled && m->nstreams == 2 && (m->pt_big[1] || level > 1) &&
           !m->pt_big[2] && m->cfg.kind == SERT_KIND_VECTORSPACE && !m->cfg.keep_grads;
}

// NCE score / loss / gradient coefficients
template <bool TRAIN>
static int vs_loss(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, de = c.entity_dim;
    const size_t row0 = (size_t)batch_index * B;
    {
        ScopedTimer t(m, TG_LOSS);
        const int32_t* y = ds.y + row0;
        const float* w = TRAIN ? ds.w + row0 : nullptr;
        const float inv_batch = 1.0f / (float)c.global_batch_size;
        dim3 block(256);
        // training with a side stream: the fork event of the backward pass is this kernel's own
        // completion signal (common.h: SERT_LAUNCH)
        m->fork_bound = false;
        if (de > 512) SERT_FAIL("entity_dim > 512 is not supported");   // (before an event is armed)
        if (TRAIN && ext_events() && (!fork_late_mode(m) || fork_at_nce(m)) && !m->timing.enabled && m->nstreams >= 2 && de % 4 == 0) {
            set_stop_event(m->ev_fork);
            m->fork_bound = true;
        }
        if (de % 4 == 0) {
            const int nch = cdiv(de / 4, 16);
            dim3 grid(cdiv(B, 16));
#define SERT_NCE_CASE(N)                                                                     \
    case N:                                                                                  \
        SERT_LAUNCH((vs_nce<N, TRAIN>), grid, block, 0, m->stream, m->T, m->re, y,          \
                           m->neg, w, m->DA, m->coef, m->cand, m->rowloss, B,               \
                           c.num_negatives, de, inv_batch, TRAIN ? m->red_loss : (float*)nullptr); \
        break;
#define SERT_NCE_REGS(N, C)                                                                  \
    SERT_LAUNCH((vs_nce_regs<N, TRAIN, C>), grid, block, 0, m->stream, m->T, m->re, y,       \
                       m->neg, w, m->DA, m->coef, m->cand, m->rowloss, B, c.num_negatives,   \
                       de, inv_batch, TRAIN ? m->red_loss : (float*)nullptr)
            static const bool no_regs = variant_knob("SERT_NCE_PER_CANDIDATE") != nullptr;
            const int nc = c.num_negatives + 1;
            // (d_e = 300, five float4 per lane and candidate: 256 VGPRs + AGPR spills, one wave per SIMD --
            //  191 us against 169 us for the per-candidate kernel at C4: the limit stays at four)
            if (!no_regs && nch <= 4 && nc <= 12) {
                // every candidate row of a row in registers (kernels_vs.h: vs_nce_regs)
                const int key = nch * 2 + (nc > 6 ? 1 : 0);
                switch (key) {
                    case 2: SERT_NCE_REGS(1, 6); break;
                    case 3: SERT_NCE_REGS(1, 12); break;
                    case 4: SERT_NCE_REGS(2, 6); break;
                    case 5: SERT_NCE_REGS(2, 12); break;
                    case 6: SERT_NCE_REGS(3, 6); break;
                    case 7: SERT_NCE_REGS(3, 12); break;
                    case 8: SERT_NCE_REGS(4, 6); break;
                    default: SERT_NCE_REGS(4, 12); break;
                }
            } else
            switch (nch) {
                SERT_NCE_CASE(1) SERT_NCE_CASE(2) SERT_NCE_CASE(3) SERT_NCE_CASE(4)
                SERT_NCE_CASE(5) SERT_NCE_CASE(6) SERT_NCE_CASE(7) SERT_NCE_CASE(8)
                default: SERT_FAIL("entity_dim > 512 is not supported");
            }
#undef SERT_NCE_REGS
#undef SERT_NCE_CASE
            set_stop_event(nullptr);   // (never leave an armed event behind a launch that did not happen)
            // (training: the kernel left one loss partial per workgroup in red_loss)
            m->nce_loss_partials = TRAIN ? cdiv(B, 16) : 0;
        } else {
            m->nce_loss_partials = 0;
            const int npl = cdiv(de, 64);
            dim3 grid(cdiv(B, 4));
#define SERT_NCE_CASE(N)                                                                     \
    case N:                                                                                  \
        hipLaunchKernelGGL((vs_nce_scalar<N, TRAIN>), grid, block, 0, m->stream, m->T,      \
                           m->re, y, m->neg, w, m->DA, m->coef, m->cand, m->rowloss, B,     \
                           c.num_negatives, de, inv_batch);                                  \
        break;
            switch (npl) {
                SERT_NCE_CASE(1) SERT_NCE_CASE(2) SERT_NCE_CASE(3) SERT_NCE_CASE(4)
                SERT_NCE_CASE(5) SERT_NCE_CASE(6) SERT_NCE_CASE(7) SERT_NCE_CASE(8)
                default: SERT_FAIL("entity_dim > 512 is not supported");
            }
#undef SERT_NCE_CASE
        }
    }
    return 0;
}

// dh and dW (+ db) of the projection in one launch (gemm_bwd_fused.h) where the shape allows it
static bool bwd_fused_applies(const sert_model* m) {
    // opt-in (SERT_BWD_FUSED=1): measured EQUAL to the two gemm.h launches at C2 (57.5 us against 29.3 + 29.2;
    // step 0.3030 against 0.3046 ms, inside the run-to-run spread) -- the fused kernel keeps the matrix pipe as
    // busy as they do (48 %), it only saves a launch and half of the partial slabs
#ifdef SERT_VARIANTS
    static const bool on = variant_knob("SERT_BWD_FUSED") && atoi(variant_knob("SERT_BWD_FUSED")) != 0;
    return on && m->cfg.kind == SERT_KIND_VECTORSPACE && m->cfg.word_dim == FB_D && m->cfg.entity_dim == FB_D &&
           m->cfg.batch_size >= 1024 && m->nstreams < 3 && (size_t)256 * (FB_D * FB_D + FB_D) <= m->part_count;
#else
    (void)m;
    return false;      // (the kernel lives in csrc/variants/gemm_bwd_fused.h: not in the product library)
#endif
}

// Few (pair, entity) keys over a table too large for the sort-free LDS path: the one-launch range kernel instead of
// sort + chunked reduce + fix-up (eight launches).  The scan costs ranges x pairs id reads: capped at 64 M (~256 MB out of L2).
// OPT-IN in a VARIANTS BUILD (SERT_EGRAD_RANGES=1 at sert_create): 32 us alone against 67 for the eight launches at the product-search settings,
// but the STEP does not move (0.202-0.207 against 0.199-0.203 ms: that chain is not what the step waits for; round 5).
#ifdef SERT_VARIANTS
static bool egrad_ranges_ok(const sert_model* m, int total) {
    const long long ranges = cdiv(m->cfg.num_entities, kERange);
    return m->egrad_ranges && !m->egrad_force_sort && !m->epart && m->cfg.entity_dim % 4 == 0 && total <= (1 << 20) && ranges * (long long)total <= (64ll << 20);
}
#endif

static int vs_backward(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, dw = c.word_dim, de = c.entity_dim;
    const size_t row0 = (size_t)batch_index * B;
    const bool fork_late = fork_late_mode(m);
    const bool fork_nce = fork_late && fork_at_nce(m);
    const bool side_heavy = side_heavy_mode(m);
    const bool fused_bwd = bwd_fused_applies(m) && !side_heavy;
#ifdef SERT_VARIANTS
    const int fused_grid = std::min(256, cdiv(B, FB_ROWS));   // one workgroup per CU, or per strip if there are fewer
#else
    const int fused_grid = 0;
#endif
    m->bucket_early = false;
    for (int32_t& v : m->eg_plan) v = 0;
    auto early_bucket = [&]() -> int {
        // Round 6: the PARTITION of this step's (pair, entity) keys by entity range (egrad_bucket, 19 us at C2) needs the
        // labels and the negatives only -- not the loss kernel's coefficients -- and this step's negatives were drawn on this
        // very stream during the previous step (neg_side_ready): it goes out in front of the fork as well and runs beside
        // gather / projection / loss.  The chain behind the fork is then egrad_acc alone: it starts 19 us earlier and ends
        // that much earlier beside the word table's update (profiles/r06_experiments.txt, item 1).
        static const bool no_early_bucket = variant_knob("SERT_NO_EARLY_BUCKET") != nullptr;
        m->bucket_early = false;
        // Measured (tools/experiments/r06_early_bucket.sh, r06_fork_nce_early.sh; three rounds each on one box, ms/step early / behind
        // the fork): batch 32768 0.1426-0.1466 / 0.1515-0.1552 (-5.5 %), 65536 0.2404-0.2427 / 0.2404-0.2426 (equal: egrad_acc ends
        // 29 us earlier, the tree beside it stretches by 5), 16384 0.1182-0.1213 / 0.1170-0.1184 (+1.5 %), 8192 0.0977-0.1000 /
        // 0.0938-0.0966 (+3-5 %: there the partition beside the forward delays the loss kernel and the update): from batch 32768.
        // SERT_EARLY_BUCKET=0 / 1 (variants build) forces it off / on.
        static const int early_knob = variant_knob("SERT_EARLY_BUCKET") ? atoi(variant_knob("SERT_EARLY_BUCKET")) : -1;
        const bool want_early = early_knob >= 0 ? early_knob != 0 : B >= 32768;
        if (!no_early_bucket && want_early && fork_late && !is_dp(m) && !m->timing.enabled && m->epart && c.kind == SERT_KIND_VECTORSPACE &&
            c.num_negatives > 0 && m->neg_side_ready && ds.y) {
            ScopedTimer t(m, TG_SORT, m->stream2);
            hipLaunchKernelGGL(egrad_bucket, dim3(m->eg_num_sub), dim3(512), 0, m->stream2, (const int32_t*)nullptr, B, c.num_negatives + 1,
                               m->eg_sub_rows, m->eg_er_shift, m->eg_ranges, m->eg_entries, m->eg_offs,
                               (const int32_t*)ds.y + row0, (const int32_t*)m->neg);
            m->bucket_early = true;
        }
        return 0;
    };
    // ... and the same for the SORTED entity chain of a larger entity table (V_e > 2048: the reference's product-search settings, C4):
    // the stable counting sort of the (entity, pair) keys -- six of the chain's eight launches -- needs the labels and the negatives
    // only.  With the negatives drawn ahead on this stream it goes out in front of the fork wait and runs beside gather / projection /
    // loss; behind the fork the chain is the chunked reduce + the fix-up.  (The first histogram pass also clears the per-entity run
    // bounds: nothing of the previous step reads them any more -- its fix-up precedes this in the stream.)
    m->sort_early = false;
    auto early_sort = [&]() -> int {
        // Measured (tools/experiments/r06_early_sort.sh, r06_early_sort_sizes.sh; two to three rounds each on one box; ms/step beside the
        // forward / inside the chain): the reference's product-search settings (batch 4096, V_e 32768, d_w 300) 0.1669-0.1689 / 0.1696-0.1727,
        // the same at batch 1024 0.1434-0.1443 / 0.1513-0.1527; d = 128, V_e 32768: batch 16384 0.1514-0.1529 / 0.1717-0.1727 (-12 %), 32768
        // 0.2034-0.2049 / 0.2255-0.2279, 65536 0.3227-0.3253 / 0.3434-0.3457; V_e 100000: batch 65536 at d = 128 0.4099-0.4140 / 0.4319-0.4355,
        // d = 300: batch 16384 0.705-0.714 / 0.709-0.717, 32768 0.865-0.920 / 0.906-0.954 -- but C4 itself (batch 65536, d = 300) 1.404-1.411 /
        // 1.360-1.364: there the chunked reduce (865 MB of row fetches) then starts beside the word gradient's tree (680 MB of them) instead of
        // beside the update, and the tree takes 389 us instead of 125.  Taken while dh, the tree's source, is below 64 MB.
        // SERT_EARLY_SORT=1 (variants build) forces it, SERT_NO_EARLY_SORT=1 switches it off.
        static const bool off = variant_knob("SERT_NO_EARLY_SORT") != nullptr;
        static const bool force = variant_knob("SERT_EARLY_SORT") && atoi(variant_knob("SERT_EARLY_SORT")) != 0;
        if (!force && (size_t)B * dw * sizeof(float) >= ((size_t)64 << 20)) return 0;
        if (off || m->epart || !m->cand_early || is_dp(m) || m->timing.enabled || m->nstreams < 2 || c.kind != SERT_KIND_VECTORSPACE ||
            c.num_negatives <= 0 || !m->neg_side_ready || !ds.y || c.num_entities <= 0)
            return 0;
        const int total = B * (c.num_negatives + 1);
        ScopedTimer t(m, TG_SORT, m->stream2);
        hipLaunchKernelGGL(vs_build_cand, dim3(grid_for(total)), dim3(256), 0, m->stream2, (const int32_t*)ds.y + row0, (const int32_t*)m->neg, B,
                           c.num_negatives, m->cand_early);
        SERT_TRY(entity_key_sort(m, total, m->stream2, m->cand_early));
        m->sort_early = true;
        return 0;
    };
    auto entity_grad = [&]() -> int {
        // fork: this chain only depends on the NCE kernel and is independent of the
        // GEMMs / word-table reduction below, so it runs on the side stream
        // (timing mode measures every kernel alone: everything stays on the main stream)
        hipStream_t st = (m->timing.enabled || m->nstreams < 2) ? m->stream : m->stream2;
        if ((!fork_late || fork_nce) && !m->dw_side_first) {   // (nce_dw: the side stream has met the fork already)
            if (!m->fork_bound) SERT_HIP(hipEventRecord(m->ev_fork, m->stream));
            m->fork_bound = false;
            if (st != m->stream) SERT_HIP(hipStreamWaitEvent(st, m->ev_fork, 0));
        }
        const int total = B * (c.num_negatives + 1);
        const int V = c.num_entities;
        m->re_in_parts = false;
        if (m->epart) {
            // small entity vocabulary: no global sort -- pairs bucketed by entity range per sub-group,
            // then row groups x entity ranges with the accumulators in LDS (kernels_egrad.h)
            const int de4 = de / 4, c1 = c.num_negatives + 1;
            const size_t lds = (size_t)4 * 16 * de * sizeof(float);
            const int grid = 8 * cdiv(m->eg_groups, 8) * m->eg_ranges;
            if (!m->bucket_early) {     // (else: the partition ran beside the forward, see dh_gemm below)
                ScopedTimer t(m, TG_SORT, st);
                hipLaunchKernelGGL(egrad_bucket, dim3(m->eg_num_sub), dim3(512), 0, st, m->cand, B, c1, m->eg_sub_rows,
                                   m->eg_er_shift, m->eg_ranges, m->eg_entries, m->eg_offs, (const int32_t*)nullptr,
                                   (const int32_t*)nullptr);
            }
            {
                ScopedTimer t(m, TG_EGRAD, st);
#define SERT_EL_ARGS m->eg_entries, m->eg_offs, m->coef, m->T, c1, de, V, m->eg_sub_rows, m->eg_num_sub, \
                     m->eg_subs_per_group, m->eg_groups, m->eg_ranges, m->epart
                hipLaunchKernelGGL((egrad_acc<2>), dim3(grid), dim3(256), lds, st, SERT_EL_ARGS);
                m->eg_plan[0] = SERT_EGRAD_PATH_BUCKET;
                m->eg_plan[1] = m->eg_sub_rows; m->eg_plan[2] = m->eg_num_sub; m->eg_plan[3] = m->eg_subs_per_group;
                m->eg_plan[4] = m->eg_groups; m->eg_plan[5] = m->eg_ranges;
#undef SERT_EL_ARGS
            }
            // Single GPU: the only reader of dR_e is the small-tensor optimiser, which adds the row
            // groups' tables itself (same order) -- no launch for the sum.  Data parallel: the
            // all-reduce needs the summed table.
            static const bool no_fold = variant_knob("SERT_EGRAD_GROUP_SUM") != nullptr;
            m->re_in_parts = !is_dp(m) && !m->pt_big[1] && !no_fold;
            if (!m->re_in_parts) {
                ScopedTimer t(m, TG_EFIX, st);
                const size_t table4 = (size_t)V * de4;
                hipLaunchKernelGGL(egrad_group_sum, dim3(grid_for((int64_t)table4)), dim3(256), 0, st, m->epart, m->eg_groups,
                                   table4, m->g_re);
                m->eg_plan[6] = 1;
            }
#ifdef SERT_VARIANTS
        } else if (egrad_ranges_ok(m, total)) {
            // few pairs over a mid-size table: one workgroup per range of 32 entities, no sort (variants/kernels_egrad_ranges.h)
            ScopedTimer t(m, TG_EGRAD, st);
            hipLaunchKernelGGL(egrad_ranges, dim3(cdiv(V, kERange)), dim3(256), 0, st, (const int32_t*)m->cand, (const float*)m->coef,
                               (const float*)m->T, total, c.num_negatives + 1, de, V, m->g_re);
#endif
        } else {
        // dR_e: stable sort of the (entity, pair) keys, chunked reduce, carry fix-up
        if (!m->sort_early) {       // (else: the keys were sorted beside the forward, see early_sort below)
            ScopedTimer t(m, TG_SORT, st);
            SERT_TRY(entity_key_sort(m, total, st));
        }
        const int chunks = cdiv(total, kEChunk);
        m->eg_plan[0] = SERT_EGRAD_PATH_SORTED;
        dim3 cgrid(cdiv(chunks, 16)), fgrid(cdiv(V, 4)), blk(256);
#define SERT_EG_ARGS m->cand_sorted, m->pair_sorted, m->coef, m->T, total, c.num_negatives + 1, de, \
                     m->g_re, m->ehead, m->etail, m->run_start, m->run_end
        {
            ScopedTimer t(m, TG_EGRAD, st);
            if (de % 4 == 0) {
                const int nch = cdiv(de / 4, 16);
                if (nch <= 1)      { hipLaunchKernelGGL((egrad_chunk_reduce<4, 1>), cgrid, blk, 0, st, SERT_EG_ARGS); m->eg_plan[9] = 4; m->eg_plan[10] = 1; }
                else if (nch <= 2) { hipLaunchKernelGGL((egrad_chunk_reduce<4, 2>), cgrid, blk, 0, st, SERT_EG_ARGS); m->eg_plan[9] = 4; m->eg_plan[10] = 2; }
                else if (nch <= 5) { hipLaunchKernelGGL((egrad_chunk_reduce<4, 5>), cgrid, blk, 0, st, SERT_EG_ARGS); m->eg_plan[9] = 4; m->eg_plan[10] = 5; }
                else               { hipLaunchKernelGGL((egrad_chunk_reduce<4, 8>), cgrid, blk, 0, st, SERT_EG_ARGS); m->eg_plan[9] = 4; m->eg_plan[10] = 8; }
            } else {
                hipLaunchKernelGGL((egrad_chunk_reduce<1, 4>), cgrid, blk, 0, st, SERT_EG_ARGS);
                m->eg_plan[9] = 1; m->eg_plan[10] = 4;
            }
        }
        {
            ScopedTimer t(m, TG_EFIX, st);
            const bool few = V < 256 && de <= 512;   // few entities: one workgroup per entity (long runs)
            if (de % 4 == 0) {
                if (few) {
                    hipLaunchKernelGGL((egrad_fixup_wg<4>), dim3(V), blk, 0, st, m->run_start, m->run_end, V, de,
                                       m->ehead, m->etail, m->g_re);
                    m->eg_plan[11] = SERT_EGRAD_FIXUP_WORKGROUP;
                } else {
                    hipLaunchKernelGGL((egrad_fixup<4>), fgrid, blk, 0, st, m->run_start, m->run_end, V, de,
                                       m->ehead, m->etail, m->g_re);
                    m->eg_plan[11] = SERT_EGRAD_FIXUP_WAVE;
                }
            } else if (few) {
                hipLaunchKernelGGL((egrad_fixup_wg<1>), dim3(V), blk, 0, st, m->run_start, m->run_end, V, de,
                                   m->ehead, m->etail, m->g_re);
                m->eg_plan[11] = SERT_EGRAD_FIXUP_WORKGROUP;
            } else {
                hipLaunchKernelGGL((egrad_fixup<1>), fgrid, blk, 0, st, m->run_start, m->run_end, V, de,
                                   m->ehead, m->etail, m->g_re);
                m->eg_plan[11] = SERT_EGRAD_FIXUP_WAVE;
            }
        }
#undef SERT_EG_ARGS
        }   // sorted path
        return 0;
    };
    bool dense_bound = false;
    auto dh_gemm = [&]() -> int {
        {
            // dh = da.W^T
            ScopedTimer t(m, TG_GEMM_DX);
#ifdef SERT_VARIANTS
            const bool strip = gemm_strip_ok(B, dw, de, de, de, true, m->DA, m->W);
#else
            const bool strip = false;
#endif
            // (ev_dense below: the completion signal of this GEMM, not a barrier packet behind it)
            dense_bound = m->lazy_join && ext_events() && !strip && !fork_nce;
            if (dense_bound) set_stop_event(fork_late ? m->ev_fork : m->ev_dense);
#ifdef SERT_VARIANTS
            if (fused_bwd) {
                // dh, the per-workgroup partial slabs of dW and their column sums (db): one launch
                static const bool attr_set = hipFuncSetAttribute((const void*)vs_bwd_fused, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                 (int)vs_bwd_fused_lds_bytes()) == hipSuccess;
                if (!attr_set) { set_stop_event(nullptr); SERT_FAIL("cannot reserve the LDS of vs_bwd_fused"); }
                BwdFusedArgs fa;
                fa.DA = m->DA; fa.H = m->H; fa.W = m->W; fa.DH = m->DH; fa.part = m->part; fa.B = B;
                fa.stride = (size_t)FB_D * FB_D + FB_D;
                SERT_LAUNCH(vs_bwd_fused, dim3(fused_grid), dim3(FB_THREADS), vs_bwd_fused_lds_bytes(), m->stream, fa);
            } else
            if (strip)
                launch_gemm_strip<true, EPI_STORE>(m->stream, m->DA, m->W, m->DH, nullptr, B, dw, de, de, de, dw);
            else
#endif
                launch_gemm<false, true, EPI_STORE>(m->stream, m->DA, m->W, m->DH, nullptr, B, dw, de, de,
                                                    de, dw);
            set_stop_event(nullptr);
        }
        // From here on the main stream has produced dW, db and the loss partials AND is done
        // READING W (the dh GEMM): the side stream may update the small tensors.
        if (m->lazy_join && !dense_bound && !fork_nce) SERT_HIP(hipEventRecord(fork_late ? m->ev_fork : m->ev_dense, m->stream));
        if (fork_late && !fork_nce && !is_dp(m) && !m->timing.enabled && m->epart && c.kind == SERT_KIND_VECTORSPACE &&
            c.num_negatives > 0 && m->neg_alt_step != m->step + 1) {
            // The NEXT step's negatives (Philox position = the step counter after this step's update) are drawn NOW,
            // while the side stream still idles in front of the fork -- beside this step's gather / projection / loss
            // kernels -- instead of at the end of the step between the entity chain and the R_e update, where the
            // 5 us launch stretched to 18 us beside the word table's Adam and sat on the path to the tail (round 4:
            // the side chain ended 2.5 us AFTER the main stream's Adam).  neg_alt is free: this step's own negatives
            // were swapped into `neg` at its start.  Ordered before the next step's loss kernel by this stream's
            // order and the end-of-step join (ev_small).
            const int64_t count = (int64_t)c.batch_size * c.num_negatives;
            hipLaunchKernelGGL(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0, m->stream2, m->neg_alt, count,
                               (int64_t)m->rank * count, (uint32_t)c.num_entities, c.seed, (uint64_t)(m->step + 1) * 2);
            m->neg_alt_step = m->step + 1;
        }
        if (fork_late && !fork_nce) SERT_HIP(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
        return 0;
    };
    auto word_table_sum = [&]() -> int {
        {
            ScopedTimer t(m, TG_SCATTER);
            // dR_w[X[i,k],:] += dh[i,:] / n
            SERT_TRY(word_grad_segsum(m, ds, batch_index, m->DH, (float)n));
        }
        return allreduce_word_grad(m);
    };
    auto dense_grad = [&]() -> int {
        // dW = h^T.da (reduction over the batch: split-K, order-fixed combine);
        // db = sum_i da_i rides along as the column sums of the da operand.
        // Third stream: dW and dh are both 512-workgroup launches (2 waves per SIMD, too
        // few to hide their own latencies) -- side by side they fill each other's bubbles.
        hipStream_t sd = (m->timing.enabled || m->nstreams < 3) ? m->stream : m->stream3;
        // (side_heavy: on the side stream behind the entity chain, see side_heavy_mode)
        if (side_heavy && m->lazy_join) sd = m->stream2;
        if (m->dp_late_join || m->dw_side_first) sd = m->stream2;
        if (sd != m->stream && sd != m->stream2 && !fork_late) SERT_HIP(hipStreamWaitEvent(sd, m->ev_fork, 0));
        // ~1024 workgroup items in all, at most 512 slabs (the optimum at one output tile: 512 slabs
        // of 128 rows) and at least 64 rows per slab.  With nine output tiles (d = 300) that is 114
        // slabs at batch >= 16384 and 64 at 4096 -- 512 / 256 slabs made the combine read up to 92 MB
        // of partials (sweep in DESIGN.md section 7.5).
        static const int user_splits = [] { const char* e = variant_knob("SERT_DW_SPLITS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();
        int auto_splits = std::max(1, std::min(std::min(512, cdiv(1024, cdiv(dw, GM) * cdiv(de, GN))), B / 64));
        // the bf16-pipe kernel (gemm_x3.h) runs one workgroup per (k range, 160-column tile; one tile up to 128 x 128): one
        // workgroup per CU -- 256 slabs at C2 (0.2745 -> 0.2697 ms against 512; 128: 0.285), 128 at C4 (1.595 -> 1.579 ms)
        const int x3_splits = std::max(1, std::min(256 / ((dw <= 128 && de <= 128) ? 1 : cdiv(de, 160)), B / 64));
        if (gemm_x3_enabled() && x3_shape_ok(true, false, m->H, m->DA, dw, de, B, dw, de, x3_splits))
            auto_splits = x3_splits;
        const int want_splits = user_splits ? user_splits : auto_splits;
        int splits = std::min(want_splits, cdiv(B, GK));
        int kper = (int)round_up(cdiv(B, splits), GK);
        splits = cdiv(B, kper);
        const size_t mn = (size_t)dw * de;
        const size_t stride = mn + de;
        if (fused_bwd) {
            // (the partial slabs were written by vs_bwd_fused, behind which this runs)
            splits = fused_grid;
            if (sd != m->stream) SERT_FAIL("internal: the fused backward needs dW's combine on the main stream");
        } else
#ifdef SERT_VARIANTS
        if (gemm_strip_ok(B, de, dw, dw, de, false, m->H, m->DA) && dw % 32 == 0 && de % 4 == 0) {
            // strip kernel: every workgroup accumulates its contiguous strips' h^T.da (+ column sums)
            ScopedTimer t(m, TG_GEMM_DW);
            static const int want_wgs = variant_knob("SERT_STRIP_DW_WGS") ? atoi(variant_knob("SERT_STRIP_DW_WGS")) : 512;   // tuning knob
            const int strips = cdiv(B, SG_ROWS);
            const int spw = std::max(1, cdiv(strips, std::min(want_wgs, 1024)));
            splits = cdiv(strips, spw);
            hipLaunchKernelGGL(gemm_strip_tn, dim3(splits), dim3(256), 0, sd, (const float*)m->H, (const float*)m->DA, B,
                               dw, de, dw, de, spw, m->part, stride);
        } else
#endif
        {
            ScopedTimer t(m, TG_GEMM_DW);
            launch_gemm<true, false, EPI_STORE, true>(sd, m->H, m->DA, m->part, nullptr, dw, de,
                                                      B, dw, de, de, splits, kper, stride);
        }
        // single GPU: the combine rides in the step's tail launch (vs_tail) with the W, b update and
        // the loss finalisation
        static const bool no_tail = variant_knob("SERT_NO_TAIL") != nullptr;   // cross-check knob
        m->tail_splits = 0;
        // (side_heavy: the partial slabs come from the side stream, which is joined in front of the tail)
        if (!no_tail && !is_dp(m) && (sd == m->stream || ((side_heavy || m->dw_side_first) && sd == m->stream2)) &&
            m->cfg.kind == SERT_KIND_VECTORSPACE && !m->pt_big[2] &&
            mn + de < ((size_t)1 << 31)) {
            m->tail_splits = splits;
            m->tail_stride = stride;
        } else {
            ScopedTimer t(m, TG_SPLITK);
            launch_reduce_partials(sd, m->part,
                               splits, stride, stride, m->g_w, mn, m->g_b);
        }
        // the loss partials only depend on the NCE kernel too
        SERT_TRY(reduce_rowloss(m, sd));
        if (m->dw_side_first) SERT_HIP(hipEventRecord(m->ev_dense, sd));   // (the tail waits for this, not for the chain behind it)
        if (sd != m->stream && sd != m->stream2 && !fork_late) SERT_HIP(hipEventRecord(m->ev_join3, sd));
        return 0;
    };
    // On a single GPU the only consumer of dR_e is the small-tensor optimiser, which runs on
    // the side stream right behind the entity chain: the main stream then never waits for
    // that chain, and the word-table optimiser starts straight after segsum instead of
    // idling ~12 us on a cross-queue dependency.
    m->lazy_join = !is_dp(m) && !m->timing.enabled && m->nstreams == 2 && (m->n_re <= ((size_t)1 << 22) || side_heavy);
    m->side_heavy = side_heavy;
    // Data parallel over an asynchronous communicator: nothing on the main stream needs what the side stream produces
    // (dR_e, and -- issued there too -- dW, db and the loss sum) before the all-reduce of the replicated remainder, and
    // that runs on the communication stream.  So the communication stream joins the side stream (allreduce_rest), the main
    // stream goes from the segmented sum straight to the hand-over of the word rows and their update: 40 us of dW GEMM,
    // combine and loss sum leave the critical path (C2, world of one: 0.329 -> 0.29 ms)
    // Single GPU, late fork: dW, db (and the loss partials) only feed the tail.  FIRST on the side stream -- in front of the
    // entity chain, beside the segmented sum -- they leave the main stream's dependency chain (loss -> dh -> segmented sum
    // -> word-table update -> tail) 20 us shorter; the tail waits for their event, which is long complete by then.
    static const bool dw_first_off = variant_knob("SERT_DW_FIRST") && atoi(variant_knob("SERT_DW_FIRST")) == 0;
    // Measured (tools/experiments/r04_dw_first*.sh, C2 dims): batch 4096 0.1176 -> 0.1092 ms, 8192 0.130 -> 0.116, 16384 0.1566 ->
    // 0.1429, 32768 0.191 -> 0.175; at 65536 0.2720 -> 0.2745 -- there dW streams its 67 MB beside the first level of the
    // segmented sum, whose 33.5 MB of dh rows then no longer stay in the Infinity Cache.  Taken while dh is below 24 MB.
    static const bool dw_first_always = variant_knob("SERT_DW_FIRST") && atoi(variant_knob("SERT_DW_FIRST")) == 2;
    // (!pt_big[2]: a projection matrix large enough for a streaming update of its own is updated on the main stream, which
    //  would then have to wait for the side stream's dW)
    const bool fork_nce_dw = fork_nce && fork_at_nce_dw(m) && !side_heavy && m->lazy_join && !fused_bwd && !m->pt_big[2] && m->nstreams == 2;
    // Round 6: the entity keys' partition goes out first of all on the side stream, in front of the fork wait (early_bucket above) --
    // and where it does, dW / db first on the side stream pays at EVERY batch size: the chain behind the fork is then dW + egrad_acc,
    // the main stream goes from dh straight into the tree.  tools/experiments/r06_dw_first_again.sh, three rounds on one box, ms/step,
    // dW on the main stream / first on the side stream: batch 65536 0.2375-0.2390 / 0.2244-0.2261 (-5.4 %; with the partition behind the
    // fork, as in round 5: 0.2381-0.2404 / 0.2346-0.2360), 131072 0.4190-0.4222 / 0.4040-0.4142.
    SERT_TRY(early_bucket());
    SERT_TRY(early_sort());
    m->dw_side_first = fork_nce_dw ||
                       (!dw_first_off && fork_late && !fork_nce && !side_heavy && m->lazy_join && !fused_bwd &&
                        !m->pt_big[2] && c.kind == SERT_KIND_VECTORSPACE &&
                        (dw_first_always || (((size_t)B * dw * sizeof(float) <= ((size_t)24 << 20) || m->bucket_early) && m->epart)));
    // (m->epart: the sort-free entity chain of small entity tables.  Behind the counting sort of a larger one the side stream is
    //  the longer of the two already: the reference's product-search settings, V_e = 32768, 205.8 -> 214.5 us with dW in front)
    static const bool dp_late_off = variant_knob("SERT_DP_LATE") && atoi(variant_knob("SERT_DP_LATE")) == 0;
    const bool dp_late = !dp_late_off && is_dp(m) && !m->host_ar && m->comm && !m->timing.enabled && m->nstreams == 2 && !side_heavy && !fork_nce &&
                         !fork_late;
    m->dp_late_join = dp_late;
    if (side_heavy) {
        SERT_TRY(entity_grad());       // side, forked on the loss kernel's completion
        SERT_TRY(dh_gemm());           // main (its completion is ev_dense)
        SERT_TRY(word_table_sum());    // main
        SERT_TRY(dense_grad());        // side, behind the entity chain
    } else if (fork_nce && fork_nce_dw) {
        if (!m->fork_bound) SERT_HIP(hipEventRecord(m->ev_fork, m->stream));
        m->fork_bound = false;
        SERT_HIP(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
        SERT_TRY(dh_gemm());           // main
        SERT_TRY(dense_grad());        // side, beside the dh GEMM
        SERT_TRY(entity_grad());       // side, behind dW
        SERT_TRY(word_table_sum());    // main
    } else if (fork_nce) {
        SERT_TRY(entity_grad());       // side, forked on the NCE kernel's completion
        SERT_TRY(dh_gemm());
        SERT_TRY(dense_grad());
        SERT_TRY(word_table_sum());
    } else if (fork_late) {
        SERT_TRY(dh_gemm());           // main; its completion is the step's one fork
        if (m->dw_side_first) SERT_TRY(dense_grad());   // side, in front of the entity chain
        SERT_TRY(entity_grad());       // side
        if (!m->dw_side_first) SERT_TRY(dense_grad());  // main (W and b are then updated on the main stream too)
        SERT_TRY(word_table_sum());    // main
    } else if (is_dp(m)) {
        // data parallel: the word-table gradient first, so that its exchange (rows' all-to-all or
        // reduce-scatter) overlaps dW and the entity chain (dW in front of the segmented sum instead:
        // 0.362 -> 0.370 ms with a world of one -- the hand-over then sits bare on the critical path)
        if (dp_late) {
            // the side stream takes dW, db and the loss sum FIRST (beside dh and the segmented sum), then the entity chain:
            // behind that chain they ran beside the word table's Adam, three times as long, and the small all-reduce --
            // which waits for them -- ended 35 us after the Adam (0.330 ms; this order: 0.29)
            if (!m->fork_bound) SERT_HIP(hipEventRecord(m->ev_fork, m->stream));   // (else: the loss kernel's own completion signal)
            SERT_HIP(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
            // The data-parallel step is bound by the HOST (some 45 runtime calls + three collectives per step: round-5 API
            // trace, tools/experiments/r05_hip_trace.sh with SERT_FORCE_COMM=1): the launches go out in order of
            // criticality -- the main stream's dh GEMM first; issued behind the six side-stream launches it started 27 us
            // after the loss kernel had finished (C2, world of one).
            SERT_TRY(dh_gemm());
            SERT_TRY(dense_grad());
            m->fork_bound = true;          // (the fork is recorded: the entity chain only has to follow in stream order)
            SERT_TRY(entity_grad());
            SERT_TRY(word_table_sum());
        } else {
            SERT_TRY(entity_grad());
            SERT_TRY(dh_gemm());
            SERT_TRY(word_table_sum());
            SERT_TRY(dense_grad());
        }
    } else if (fused_bwd) {
        SERT_TRY(entity_grad());
        SERT_TRY(dh_gemm());           // (dh and the dW partials in one launch)
        SERT_TRY(dense_grad());
        SERT_TRY(word_table_sum());
    } else {
        // single GPU: the MFMA-bound dW beside the latency-bound sort of the side stream
        SERT_TRY(entity_grad());
        SERT_TRY(dense_grad());
        SERT_TRY(dh_gemm());           // (records ev_dense behind the dX GEMM)
        SERT_TRY(word_table_sum());
    }
    // join the entity-gradient chain (and the dense gradients of a third stream)
    if (!m->lazy_join && !m->dp_late_join && !m->timing.enabled && m->nstreams >= 2) {
        SERT_HIP(hipEventRecord(m->ev_join, m->stream2));
        SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_join, 0));
    }
    if (!m->timing.enabled && m->nstreams >= 3) SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_join3, 0));
    return 0;
}
