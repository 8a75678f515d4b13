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
        launch(convert_i64_to_i32, dim3(grid_for(count)), dim3(256), 0, st,
               m->neg_stage, m->neg, count);
    } else {
        const int64_t global_offset = (int64_t)m->rank * count;
        // Philox stream position: even = training draws, odd = evaluation draws
        // (the reference keeps two independent RandomStreams, models.py:745-752).
        launch(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0,
               st, m->neg, count, global_offset, (uint32_t)c.num_entities,
               c.seed, stream_pos, nullptr, 0, nullptr, 0);
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
    launch((vs_tail<false>), dim3(m->tail_nb), dim3(1024), 0, m->stream, m->tail_args);
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
            launch((vs_project_x3<IdT>), dim3(vs_project_grid(B, m->num_cus)), dim3(PJ_THREADS), 0, m->stream, X, (const float*)m->rw,
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
                launch((vs_gather_mean_hot<IdT>), dim3(std::min<int64_t>(grid_for((int64_t)B * dw / 4, 256, 1 << 20), 8 * m->num_cus)),
                       dim3(256), (size_t)nhot * dw * sizeof(float), m->stream, X, (const uint8_t*)ds.idx_tok_slot + row0 * n,
                       (const int32_t*)ds.idx_dense_words + (size_t)batch_index * kHeavyMax, nhot, (const float*)m->rw, m->H, B, n, dw);
            } else
#endif
            if (dw % 4 == 0 && m->tail_pending) {
                // the previous step's tail: the leading workgroups of this launch (kernels_vs.h: vs_gather_mean_tail)
                m->tail_pending = false;
                ++m->tail_counts[1];
                launch((vs_gather_mean_tail<IdT>), dim3(m->tail_nb + grid_for((int64_t)B * dw / 4, 256, 1 << 20)),
                       dim3(256), 0, m->stream, X, m->rw, m->H, B, n, dw, m->tail_args, (unsigned)m->tail_nb);
            } else {
                if (dw % 4 != 0) flush_pending_tail(m);
                gather_mean(m->stream, X, m->rw, m->H, B, n, dw);
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

// The schedule's knobs, read once per process (step_plan.h: VsKnobs)
static const VsKnobs& vs_knobs() {
    static const VsKnobs k = [] {
        VsKnobs k;
        auto num = [](const char* e, int unset) { return e ? atoi(e) : unset; };
        k.ext_events = num(variant_knob("SERT_EXT_EVENTS"), 1) != 0;
        k.fork_late = num(variant_knob("SERT_FORK_LATE"), 1) != 0;
        const char* at = variant_knob("SERT_FORK_AT");
        k.fork_at = !at || strncmp(at, "nce", 3) ? 0 : strcmp(at, "nce_dw") ? 1 : 2;
        k.side_heavy = num(knob("SERT_SIDE_HEAVY"), 1);
        k.re_defer = num(knob("SERT_RE_DEFER"), 1) != 0;
        k.early_bucket = num(variant_knob("SERT_EARLY_BUCKET"), -1);
        k.no_early_bucket = variant_knob("SERT_NO_EARLY_BUCKET") != nullptr;
        k.early_sort = num(variant_knob("SERT_EARLY_SORT"), 0) != 0;
        k.no_early_sort = variant_knob("SERT_NO_EARLY_SORT") != nullptr;
        const int dw_first = num(variant_knob("SERT_DW_FIRST"), -1);
        k.dw_first = (dw_first == 0 || dw_first == 2) ? dw_first : -1;
        k.dp_late = num(variant_knob("SERT_DP_LATE"), 1) != 0;
        k.no_tail = variant_knob("SERT_NO_TAIL") != nullptr;   // cross-check knob
        k.egrad_group_sum = variant_knob("SERT_EGRAD_GROUP_SUM") != nullptr;
        k.bwd_fused = num(variant_knob("SERT_BWD_FUSED"), 0) != 0;
        return k;
    }();
    return k;
}

// Events that mark the end of ONE kernel ride on that kernel's completion signal
// (SERT_EXT_EVENTS=0: plain hipEventRecord behind it, ~7 us of queue stall each).
static bool ext_events() { return vs_knobs().ext_events != 0; }

// Everything the schedule of a training step depends on (step_plan.h), at the head of step_forward_backward
static VsStepFacts vs_step_facts(const sert_model* m, const DataSplit& ds, bool neg_side_ready) {
    const auto& c = m->cfg;
    VsStepFacts f;
    f.kind = c.kind;
    f.host_ar = m->host_ar != nullptr; f.comm = m->comm != nullptr;
    f.timing = m->timing.enabled; f.nstreams = m->nstreams;
    f.n_re = (int32_t)std::min<size_t>(m->n_re, INT32_MAX);
    f.big_re = m->pt_big[1]; f.big_w = m->pt_big[2];
    f.keep_grads = c.keep_grads != 0;
    f.batch = c.batch_size; f.word_dim = c.word_dim; f.entity_dim = c.entity_dim; f.num_negatives = c.num_negatives;
    f.has_entities = c.num_entities > 0;
    f.sort_free = m->epart != nullptr; f.cand_early = m->cand_early != nullptr;
    f.neg_side_ready = neg_side_ready; f.has_labels = ds.y != nullptr;
    f.next_neg_drawn = m->neg_alt_step == m->step + 1;
#ifdef SERT_VARIANTS
    if (c.kind == SERT_KIND_VECTORSPACE) {
        f.dh_strip = gemm_strip_ok(c.batch_size, c.word_dim, c.entity_dim, c.entity_dim, c.entity_dim, true, m->DA, m->W);
        // (the kernel lives in csrc/variants/gemm_bwd_fused.h: not in the product library)
        f.bwd_fused_shape = c.word_dim == FB_D && c.entity_dim == FB_D && c.batch_size >= 1024 && (size_t)256 * (FB_D * FB_D + FB_D) <= m->part_count;
    }
#endif
    f.k = vs_knobs();
    return f;
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
        for (int32_t& v : m->nce_form) v = 0;   // (the instance launched below: sert_debug_nce_form, sert_hip_debug.h)
        if (de > 512) SERT_FAIL("entity_dim > 512 is not supported");
        // training with a side stream: the fork event of the backward pass is this kernel's own
        // completion signal (launch.h)
        CarriedEvent carry(TRAIN && m->plan.fork_at == SERT_VS_FORK_LOSS && m->plan.fork_carried ? m->ev_fork : nullptr);
        if (de % 4 == 0) {
            const int nch = cdiv(de / 4, 16);
            dim3 grid(cdiv(B, 16));
#define SERT_NCE_REGS(N, C)                                                                  \
    /* a training step at d_e == 64 N, every lane full: the instance without chunk masks */  \
    if (TRAIN && de == 64 * N)                                                               \
        launch((vs_nce_regs<N, TRAIN, C, TRAIN>), grid, block, 0, m->stream, m->T, m->re, y, \
               m->neg, w, m->DA, m->coef, m->cand, m->rowloss, B, c.num_negatives,           \
               de, inv_batch, TRAIN ? m->red_loss : (float*)nullptr);                        \
    else                                                                                     \
        launch((vs_nce_regs<N, TRAIN, C, false>), grid, block, 0, m->stream, m->T, m->re, y, \
               m->neg, w, m->DA, m->coef, m->cand, m->rowloss, B, c.num_negatives,           \
               de, inv_batch, TRAIN ? m->red_loss : (float*)nullptr);                        \
    m->nce_form[0] = SERT_NCE_FORM_REGS; m->nce_form[1] = N; m->nce_form[2] = C
            static const bool no_regs = variant_knob("SERT_NCE_PER_CANDIDATE") != nullptr;
            const int nc = c.num_negatives + 1;
            // (d_e = 300, five float4 per lane and candidate: 256 VGPRs + AGPR spills, one wave per SIMD --
            //  191 us against 169 us for the per-candidate kernel at C4: the limit stays at four)
            if (!no_regs && nch <= 4 && nc <= 12) {
                // every candidate row of a row in registers (kernels_vs.h: vs_nce_regs).  MAXC: 6 for z + 1 <= 6; 11 for
                // z + 1 == 11 exactly (z = 10, the reference's default: no twelfth row fetched for nothing, and d_e = 128 fits
                // four waves per SIMD); 12 for every other z + 1 <= 12
                const int key = nch * 3 + (nc <= 6 ? 0 : nc == 11 ? 1 : 2);
                switch (key) {
                    case 3: SERT_NCE_REGS(1, 6); break;
                    case 4: SERT_NCE_REGS(1, 11); break;
                    case 5: SERT_NCE_REGS(1, 12); break;
                    case 6: SERT_NCE_REGS(2, 6); break;
                    case 7: SERT_NCE_REGS(2, 11); break;
                    case 8: SERT_NCE_REGS(2, 12); break;
                    case 9: SERT_NCE_REGS(3, 6); break;
                    case 10: SERT_NCE_REGS(3, 11); break;
                    case 11: SERT_NCE_REGS(3, 12); break;
                    case 12: SERT_NCE_REGS(4, 6); break;
                    case 13: SERT_NCE_REGS(4, 11); break;
                    default: SERT_NCE_REGS(4, 12); break;
                }
            } else if (!dispatch_int<1, 8>(nch, [&](auto k) {
                           constexpr int K = decltype(k)::value;
                           launch((vs_nce<K, TRAIN>), grid, block, 0, m->stream, m->T, m->re, y, m->neg, w, m->DA, m->coef, m->cand,
                                  m->rowloss, B, c.num_negatives, de, inv_batch, TRAIN ? m->red_loss : (float*)nullptr);
                           m->nce_form[0] = SERT_NCE_FORM_PER_CANDIDATE; m->nce_form[1] = K;
                       }))
                SERT_FAIL("entity_dim > 512 is not supported");
#undef SERT_NCE_REGS
            // (training: the kernel left one loss partial per workgroup in red_loss)
            m->nce_loss_partials = TRAIN ? cdiv(B, 16) : 0;
            m->nce_form[4] = (int32_t)grid.x;
        } else {
            m->nce_loss_partials = 0;
            const int npl = cdiv(de, 64);
            dim3 grid(cdiv(B, 4));
            if (!dispatch_int<1, 8>(npl, [&](auto k) {
                    constexpr int K = decltype(k)::value;
                    launch((vs_nce_scalar<K, TRAIN>), grid, block, 0, m->stream, m->T, m->re, y, m->neg, w, m->DA, m->coef, m->cand,
                           m->rowloss, B, c.num_negatives, de, inv_batch);
                    m->nce_form[0] = SERT_NCE_FORM_SCALAR; m->nce_form[1] = K;
                }))
                SERT_FAIL("entity_dim > 512 is not supported");
            m->nce_form[4] = (int32_t)grid.x;
        }
        m->nce_form[3] = TRAIN ? 1 : 0;
        m->nce_form[5] = m->nce_loss_partials;
    }
    return 0;
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

// The pieces of the backward.  Each issues what the step's plan (step_plan.h) says, on the queue it says.
static hipStream_t vs_queue(const sert_model* m, int queue) {
    return queue == SERT_VS_QUEUE_SIDE ? m->stream2 : queue == SERT_VS_QUEUE_THIRD ? m->stream3 : m->stream;
}
static hipEvent_t vs_event(const sert_model* m, int event) {
    return event == SERT_VS_EVENT_FORK ? m->ev_fork : event == SERT_VS_EVENT_DENSE ? m->ev_dense : event == SERT_VS_EVENT_JOIN3 ? m->ev_join3
           : event == SERT_VS_EVENT_OPT_FORK ? m->ev_opt_fork : nullptr;
}
static int vs_bwd_fused_grid(int B) {
#ifdef SERT_VARIANTS
    return std::min(256, cdiv(B, FB_ROWS));   // one workgroup per CU, or per strip if there are fewer
#else
    (void)B;
    return 0;
#endif
}

// The partition of this step's (pair, entity) keys by entity range, from the labels and the negatives alone: on the side queue in
// front of its fork wait, beside gather / projection / loss (plan.bucket_early)
static int vs_early_bucket(sert_model* m, const DataSplit& ds, size_t row0) {
    const auto& c = m->cfg;
    ScopedTimer t(m, TG_SORT, m->stream2);
    launch(egrad_bucket, dim3(m->eg_num_sub), dim3(512), 0, m->stream2, (const int32_t*)nullptr, c.batch_size, c.num_negatives + 1,
           m->eg_sub_rows, m->eg_er_shift, m->eg_ranges, m->eg_entries, m->eg_offs,
           (const int32_t*)ds.y + row0, (const int32_t*)m->neg);
    return 0;
}
// ... and the stable counting sort of the (entity, pair) keys of the SORTED chain (plan.sort_early); behind the fork that chain is
// the chunked reduce + the fix-up.  (The first histogram pass also clears the per-entity run bounds: nothing of the previous step
// reads them any more -- its fix-up precedes this in the stream.)
static int vs_early_sort(sert_model* m, const DataSplit& ds, size_t row0) {
    const auto& c = m->cfg;
    const int total = c.batch_size * (c.num_negatives + 1);
    ScopedTimer t(m, TG_SORT, m->stream2);
    launch(vs_build_cand, dim3(grid_for(total)), dim3(256), 0, m->stream2, (const int32_t*)ds.y + row0, (const int32_t*)m->neg,
           c.batch_size, c.num_negatives, m->cand_early);
    const ChainSorted sorted = entity_key_sort(vs_entity_chain(m), m->cand_early, m->stream2);
    m->eg_plan[7] = sorted.bits; m->eg_plan[8] = sorted.passes;
    return 0;
}

// dR_e.  This chain only depends on the NCE kernel and is independent of the GEMMs / word-table reduction, so it runs on the
// side stream (timing mode measures every kernel alone: everything stays on the main stream)
static int vs_entity_grad(sert_model* m, const VsStepPlan& P) {
    const auto& c = m->cfg;
    const int B = c.batch_size, de = c.entity_dim;
    hipStream_t st = vs_queue(m, P.entity_queue);
    if (P.fork_recorded && !P.side_meets_fork) SERT_HIP(hipEventRecord(m->ev_fork, m->stream));
    if (P.entity_waits_fork) SERT_HIP(hipStreamWaitEvent(st, m->ev_fork, 0));
    const int total = B * (c.num_negatives + 1);
    const int V = c.num_entities;
    if (m->epart) {
        // small entity vocabulary: no global sort -- pairs bucketed by entity range per sub-group,
        // then row groups x entity ranges with the accumulators in LDS (kernels_egrad.h)
        const int de4 = de / 4, c1 = c.num_negatives + 1;
        const size_t lds = (size_t)4 * 16 * de * sizeof(float);
        const int grid = 8 * cdiv(m->eg_groups, 8) * m->eg_ranges;
        if (!P.bucket_early) {     // (else: the partition ran beside the forward, vs_early_bucket)
            ScopedTimer t(m, TG_SORT, st);
            launch(egrad_bucket, dim3(m->eg_num_sub), dim3(512), 0, st, m->cand, B, c1, m->eg_sub_rows,
                   m->eg_er_shift, m->eg_ranges, m->eg_entries, m->eg_offs, (const int32_t*)nullptr,
                   (const int32_t*)nullptr);
        }
        {
            ScopedTimer t(m, TG_EGRAD, st);
#define SERT_EL_ARGS m->eg_entries, m->eg_offs, m->coef, m->T, c1, de, V, m->eg_sub_rows, m->eg_num_sub, \
                 m->eg_subs_per_group, m->eg_groups, m->eg_ranges, m->epart
            launch((egrad_acc<2>), dim3(grid), dim3(256), lds, st, SERT_EL_ARGS);
            m->eg_plan[0] = SERT_EGRAD_PATH_BUCKET;
            m->eg_plan[1] = m->eg_sub_rows; m->eg_plan[2] = m->eg_num_sub; m->eg_plan[3] = m->eg_subs_per_group;
            m->eg_plan[4] = m->eg_groups; m->eg_plan[5] = m->eg_ranges;
#undef SERT_EL_ARGS
        }
        // Single GPU: the only reader of dR_e is the small-tensor optimiser, which adds the row
        // groups' tables itself (same order) -- no launch for the sum.  Data parallel: the
        // all-reduce needs the summed table.
        if (!P.re_in_parts) {
            ScopedTimer t(m, TG_EFIX, st);
            const size_t table4 = (size_t)V * de4;
            launch(egrad_group_sum, dim3(grid_for((int64_t)table4)), dim3(256), 0, st, m->epart, m->eg_groups,
                   table4, m->g_re);
            m->eg_plan[6] = 1;
        }
#ifdef SERT_VARIANTS
    } else if (egrad_ranges_ok(m, total)) {
        // few pairs over a mid-size table: one workgroup per range of 32 entities, no sort (variants/kernels_egrad_ranges.h)
        ScopedTimer t(m, TG_EGRAD, st);
        launch(egrad_ranges, dim3(cdiv(V, kERange)), dim3(256), 0, st, (const int32_t*)m->cand, (const float*)m->coef,
               (const float*)m->T, total, c.num_negatives + 1, de, V, m->g_re);
#endif
    } else {
    // dR_e: stable sort of the (entity, pair) keys, chunked reduce, carry fix-up (lazy_segsum.inc: EntityChain)
    const EntityChain chain = vs_entity_chain(m);
    m->eg_plan[0] = SERT_EGRAD_PATH_SORTED;
    if (!P.sort_early) {       // (else: the keys were sorted beside the forward, vs_early_sort)
        ScopedTimer t(m, TG_SORT, st);
        const ChainSorted sorted = entity_key_sort(chain, m->cand, st);
        m->eg_plan[7] = sorted.bits; m->eg_plan[8] = sorted.passes;
    }
    {
        ScopedTimer t(m, TG_EGRAD, st);
        const ChainReduced reduced = entity_chunk_reduce(chain, m->coef, m->T, m->g_re, st);
        m->eg_plan[9] = reduced.vec; m->eg_plan[10] = reduced.nch;
    }
    {
        ScopedTimer t(m, TG_EFIX, st);
        m->eg_plan[11] = entity_fixup(chain, m->g_re, st);
    }
    }   // sorted path
    return 0;
}

static int vs_dh_gemm(sert_model* m, const VsStepPlan& P) {
    const auto& c = m->cfg;
    const int B = c.batch_size, dw = c.word_dim, de = c.entity_dim;
    {
        // dh = da.W^T
        ScopedTimer t(m, TG_GEMM_DX);
        // (the event of its end: the completion signal of this GEMM, not a barrier packet behind it)
        CarriedEvent carry(P.dh_carried ? vs_event(m, P.dh_event) : nullptr);
#ifdef SERT_VARIANTS
        if (P.bwd_fused) {
            // dh, the per-workgroup partial slabs of dW and their column sums (db): one launch
            static const bool attr_set = hipFuncSetAttribute((const void*)vs_bwd_fused, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                             (int)vs_bwd_fused_lds_bytes()) == hipSuccess;
            if (!attr_set) SERT_FAIL("cannot reserve the LDS of vs_bwd_fused");
            BwdFusedArgs fa;
            fa.DA = m->DA; fa.H = m->H; fa.W = m->W; fa.DH = m->DH; fa.part = m->part; fa.B = B;
            fa.stride = (size_t)FB_D * FB_D + FB_D;
            launch(vs_bwd_fused, dim3(vs_bwd_fused_grid(B)), dim3(FB_THREADS), vs_bwd_fused_lds_bytes(), m->stream, fa);
        } else
        if (gemm_strip_ok(B, dw, de, de, de, true, m->DA, m->W))
            launch_gemm_strip<true, EPI_STORE>(m->stream, m->DA, m->W, m->DH, nullptr, B, dw, de, de, de, dw);
        else
#endif
            launch_gemm<false, true, EPI_STORE>(m->stream, m->DA, m->W, m->DH, nullptr, B, dw, de, de,
                                                de, dw);
    }
    // From here on the main stream has produced dW, db and the loss partials AND is done
    // READING W (the dh GEMM): the side stream may update the small tensors.
    if (P.dh_event != SERT_VS_EVENT_NONE && !P.dh_carried) SERT_HIP(hipEventRecord(vs_event(m, P.dh_event), m->stream));
    if (P.draw_next_neg) {
        // The NEXT step's negatives (Philox position = the step counter after this step's update) are drawn NOW,
        // while the side stream still idles in front of the fork -- beside this step's gather / projection / loss
        // kernels -- instead of at the end of the step between the entity chain and the R_e update, where the
        // 5 us launch stretched to 18 us beside the word table's Adam and sat on the path to the tail (round 4:
        // the side chain ended 2.5 us AFTER the main stream's Adam).  neg_alt is free: this step's own negatives
        // were swapped into `neg` at its start.  Ordered before the next step's loss kernel by this stream's
        // order and the end-of-step join (ev_small).
        const int64_t count = (int64_t)c.batch_size * c.num_negatives;
        launch(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0, m->stream2, m->neg_alt, count,
               (int64_t)m->rank * count, (uint32_t)c.num_entities, c.seed, (uint64_t)(m->step + 1) * 2, nullptr, 0, nullptr, 0);
        m->neg_alt_step = m->step + 1;
    }
    if (P.fork_at == SERT_VS_FORK_DH) SERT_HIP(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
    return 0;
}

static int vs_word_table_sum(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    {
        ScopedTimer t(m, TG_SCATTER);
        // dR_w[X[i,k],:] += dh[i,:] / n
        SERT_TRY(word_grad_segsum(m, ds, batch_index, m->DH, (float)m->cfg.window_size));
    }
    return allreduce_word_grad(m);
}

// dW = h^T.da (reduction over the batch: split-K, order-fixed combine);
// db = sum_i da_i rides along as the column sums of the da operand.
static int vs_dense_grad(sert_model* m, const VsStepPlan& P) {
    const auto& c = m->cfg;
    const int B = c.batch_size, dw = c.word_dim, de = c.entity_dim;
    hipStream_t sd = vs_queue(m, P.dense_queue);
    if (P.dense_queue == SERT_VS_QUEUE_THIRD) SERT_HIP(hipStreamWaitEvent(sd, m->ev_fork, 0));
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
    if (P.bwd_fused) {
        // (the partial slabs were written by vs_bwd_fused, behind which this runs)
        splits = vs_bwd_fused_grid(B);
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
        launch(gemm_strip_tn, dim3(splits), dim3(256), 0, sd, (const float*)m->H, (const float*)m->DA, B,
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
    m->dw_splits = splits;
    m->tail_stride = stride;
    if (!P.combine_in_tail) {
        ScopedTimer t(m, TG_SPLITK);
        launch_reduce_partials(sd, m->part,
                           splits, stride, stride, m->g_w, mn, m->g_b);
    }
    // the loss partials only depend on the NCE kernel too
    SERT_TRY(reduce_rowloss(m, sd));
    // (ev_dense: the tail waits for this, not for the chain behind it; ev_join3: the main stream, at the end of the backward)
    if (P.dense_event != SERT_VS_EVENT_NONE) SERT_HIP(hipEventRecord(vs_event(m, P.dense_event), sd));
    return 0;
}

static int vs_backward(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const VsStepPlan& P = m->plan;
    const size_t row0 = (size_t)batch_index * m->cfg.batch_size;
    for (int32_t& v : m->eg_plan) v = 0;
    if (P.bucket_early) SERT_TRY(vs_early_bucket(m, ds, row0));
    if (P.sort_early) SERT_TRY(vs_early_sort(m, ds, row0));
    if (P.side_meets_fork) {
        if (P.fork_recorded) SERT_HIP(hipEventRecord(m->ev_fork, m->stream));   // (else: the loss kernel's own completion signal)
        SERT_HIP(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
    }
    for (const int32_t piece : P.order) {
        if (piece == SERT_VS_PIECE_ENTITY) SERT_TRY(vs_entity_grad(m, P));
        else if (piece == SERT_VS_PIECE_DH) SERT_TRY(vs_dh_gemm(m, P));
        else if (piece == SERT_VS_PIECE_DENSE) SERT_TRY(vs_dense_grad(m, P));
        else SERT_TRY(vs_word_table_sum(m, ds, batch_index));
    }
    // join the entity-gradient chain (and the dense gradients of a third stream)
    if (P.end_join) {
        SERT_HIP(hipEventRecord(m->ev_join, m->stream2));
        SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_join, 0));
    }
    if (P.dense_event == SERT_VS_EVENT_JOIN3) SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_join3, 0));
    return 0;
}
