// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): the shared tail of a step: exchange, optimiser launches, loss; the step prologue; train_step_async.

// ---- shared tail: loss sum, exchange, optimiser, loss ---------------------------
// rowloss (B) -> per-block partials in red_loss; returns their count.  In a
// data-parallel step the partials are folded into the scalar slot of the flat
// gradient buffer so that the loss sum rides in the all-reduce.
static int reduce_rowloss(sert_model* m, hipStream_t st) {
    const int B = m->cfg.batch_size;
    int nb = std::min(kOptBlocks, cdiv(B, 256));
    m->loss_from_rows = false;
    if (is_vs(m) && !is_fs(m) && m->nce_loss_partials > 0) nb = m->nce_loss_partials;   // written by vs_nce
    else if (!is_dp(m) && B <= 8192) {
        // few rows: the finalisation sums them itself (fp64, fixed order) -- one 4 us launch less on a small step's chain
        m->loss_from_rows = true;
        nb = B;
    } else launch(sum_partial, dim3(nb), dim3(256), 0, st, m->rowloss, (size_t)B, m->red_loss);
    if (is_dp(m))
        launch(partials_to_scalar, dim3(1), dim3(256), 0, st, m->red_loss, nb, m->g_loss);
    m->n_loss_partials = nb;
    return 0;
}

// One streaming optimiser launch over `count` elements (kernels_opt.h).
static void launch_stream_opt(sert_model* m, hipStream_t st, float* p, float* g, float* s0, float* s1, size_t count,
                              int nb, const AdamArgs& aa, const AdadeltaArgs& da, float* sq,
                              const uint32_t* bits, unsigned row_len, float* sq_new = nullptr) {
    const bool keep = m->cfg.keep_grads != 0;
    const int rows_mode = kRowsAll;   // (kernels_opt.h keeps the rows_mode parameter of its kernels; the host always passes kRowsAll)
    if (is_vs(m)) {
        if (keep) launch((adam_l2<true>), dim3(nb), dim3(256), 0, st, p, g, s0, s1, count, aa, sq, bits, row_len, rows_mode, sq_new);
        else      launch((adam_l2<false>), dim3(nb), dim3(256), 0, st, p, g, s0, s1, count, aa, sq, bits, row_len, rows_mode, sq_new);
    } else {
        if (keep) launch((adadelta_l2<true>), dim3(nb), dim3(256), 0, st, p, g, s0, s1, count, da, sq, bits, row_len, rows_mode);
        else      launch((adadelta_l2<false>), dim3(nb), dim3(256), 0, st, p, g, s0, s1, count, da, sq, bits, row_len, rows_mode);
    }
}

// Optimiser hyper-parameters of optimiser step `t` (1-based; Adam's bias correction, models.py:922).
static void optimizer_args(const sert_model* m, int64_t t, AdamArgs* aa, AdadeltaArgs* da) {
    const auto& c = m->cfg;
    const float l2k = c.lambda_ > 0.f ? c.lambda_ / (float)c.global_batch_size : 0.f;
    *aa = AdamArgs{l2k, 0.f, c.beta1, c.beta2, c.eps};
    *da = AdadeltaArgs{l2k, c.lr, c.beta1, c.eps};
    if (is_vs(m)) {
        const float tf = (float)t;
        aa->a_t = c.lr * sqrtf(1.0f - powf(c.beta2, tf)) / (1.0f - powf(c.beta1, tf));
    }
}

// The LAZY forms of the word table's dense update (kernels_opt.h: dense_update_skip / dense_update_lazy) -- one launch on the main stream.
// t: the word table; tf: the rows this batch touches; next_bits: the rows the announced next batch touches (or null); nb: the dense launches'
// grid for a table of this size; sq: where the launch leaves its partial sums of squares.  Returns the number of partial slots it wrote.
static int launch_lazy_word_update(sert_model* m, const ParamTensor& t, const uint32_t* tf, const uint32_t* next_bits, const int nb,
                                   const AdamArgs& aa, const AdadeltaArgs& da, float* sq) {
    const auto& c = m->cfg;
    // the LAZY form of the dense update (kernels_opt.h): rows neither this batch nor the announced next one
    // touches are read (their share of sum(p^2)) but not written, except every kLazyK-th update
    LazyArgs lz = lazy_args(m, m->step - 1, /*update=*/1);
    int nb_skip = 0;    // (dense_update_skip's own grid, when it takes the launch)
    lz.next_bits = next_bits;
    lz.write_all = (next_bits == nullptr || m->step % kLazyK == 0) ? 1 : 0;
    const unsigned d4 = (unsigned)c.word_dim / 4;
    if (m->lazy_skip && m->rw_pred && d4 <= 256) {
        // rows nobody needs are not read either (kernels_opt.h: dense_update_skip): a full pass when there are no
        // valid predictions (first lazy step, behind a dense step or new parameters, no hint) and kLazyK updates
        // after the last one
        const int64_t u = m->step;                      // the update being applied
        const bool sparse = next_bits && m->rw_pred_ok && u < m->rw_pred_T;
        lz.write_all = sparse ? 0 : 1;
        if (!sparse) m->rw_pred_T = u + kLazyK;
        SkipArgs sk;
        sk.pred = m->rw_pred;
        sk.stride = m->rw_pred_stride;
        sk.npred = next_bits ? (int)(m->rw_pred_T - 1 - u) : 0;
        for (int j = 0; j < kLazyK; ++j) {
            AdamArgs a2; AdadeltaArgs d2;
            optimizer_args(m, u + 1 + j, &a2, &d2);
            sk.a_fut[j] = a2.a_t;
        }
        m->rw_pred_ok = next_bits != nullptr;
        const unsigned nrows = (unsigned)c.vocab_size;
        // (its own grid: a workgroup walks its rows one lane group per row, so shorter row ranges balance better --
        //  SERT_SKIP_BLOCKS in a variants build, tools/experiments/r05_skip_blocks.sh)
        static const int skip_blocks_knob = variant_knob("SERT_SKIP_BLOCKS") ? atoi(variant_knob("SERT_SKIP_BLOCKS")) : 0;
        const int nb_dense = nb;
        const int nb = std::max(1, std::min<int>(skip_blocks_knob > 0 ? std::min(skip_blocks_knob, 4 * kOptBlocks) : nb_dense,
                                                 (int)cdiv(nrows, 8u)));
        nb_skip = nb;
#define SERT_SKIP_LAUNCH(ADAM, LPR, CPL)                                                                                   \
    launch((dense_update_skip<ADAM, LPR, CPL>), dim3(nb), dim3(256), 0, m->stream, t.p, (const float*)t.g, t.s0,             \
           t.s1, nrows, aa, da, sq, tf, (unsigned)c.word_dim, lz, sk)
        // d_w = 300: 75 float4 per row are 3 x 32 lanes at 78 % or 2 x 64 at 59 % of the lanes, and eight rows per
        // workgroup instead of four.  Measured (tools/experiments/r05_skip_32x3.sh, three rounds, 64 x 2 -> 32 x 3):
        // product-search settings 0.1756 -> 0.1704 ms (the launch alone 68.5 us either way), W3C loglinear settings
        // 0.1922 -> 0.1894 (60.1 -> 57.5 us), C4's 150 M-element table 1.348 -> 1.344 (381 -> 387 us): taken below
        // 2^26 elements.  SERT_SKIP_32X3=0 / 1 (variants build) forces it off / on.
        static const int skip_32x3_knob = variant_knob("SERT_SKIP_32X3") ? atoi(variant_knob("SERT_SKIP_32X3")) : -1;
        const bool skip_32x3 = skip_32x3_knob >= 0 ? skip_32x3_knob != 0 : t.n < ((size_t)1 << 26);
#define SERT_SKIP_SHAPE(ADAM)                                                                   \
    do {                                                                                        \
        if (d4 <= 32) { SERT_SKIP_LAUNCH(ADAM, 32, 1); ++m->upd_counts[2]; }                    \
        else if (d4 <= 64) { SERT_SKIP_LAUNCH(ADAM, 64, 1); ++m->upd_counts[3]; }               \
        else if (d4 <= 96 && skip_32x3) { SERT_SKIP_LAUNCH(ADAM, 32, 3); ++m->upd_counts[4]; }  \
        else if (d4 <= 128) { SERT_SKIP_LAUNCH(ADAM, 64, 2); ++m->upd_counts[5]; }              \
        else if (d4 <= 192) { SERT_SKIP_LAUNCH(ADAM, 64, 3); ++m->upd_counts[6]; }              \
        else { SERT_SKIP_LAUNCH(ADAM, 64, 4); ++m->upd_counts[7]; }                             \
        ++m->upd_counts[sparse ? 9 : 8];                                                        \
    } while (0)
        if (is_vs(m)) SERT_SKIP_SHAPE(true);
        else SERT_SKIP_SHAPE(false);
#undef SERT_SKIP_SHAPE
#undef SERT_SKIP_LAUNCH
    } else {
    ++m->upd_counts[1];
    if (is_vs(m))
        launch((dense_update_lazy<true>), dim3(nb), dim3(256), 0, m->stream, t.p, (const float*)t.g, t.s0, t.s1, t.n,
               aa, da, sq, tf, (unsigned)c.word_dim, lz);
    else
        launch((dense_update_lazy<false>), dim3(nb), dim3(256), 0, m->stream, t.p, (const float*)t.g, t.s0, t.s1, t.n,
               aa, da, sq, tf, (unsigned)c.word_dim, lz);
    }
    m->rw_last_cur ^= 1;
    m->rw_stale = !lz.write_all;
    m->rw_ready_batch = lz.write_all ? -1 : m->lazy_next;
    return nb_skip > 0 ? nb_skip : nb;
}

// loss_dst: device [3], or the pinned host block (publish = true: its sequence number is
// stored after the values, for the host to spin on)
static int optimizer_and_loss(sert_model* m, float* loss_dst, bool publish = false,
                              const uint32_t* bits = nullptr, const uint32_t* next_bits = nullptr) {
    const int n_loss_partials = m->n_loss_partials;
    const auto& c = m->cfg;
    const float l2k = c.lambda_ > 0.f ? c.lambda_ / (float)c.global_batch_size : 0.f;
    m->step += 1;
    AdamArgs aa; AdadeltaArgs da;
    optimizer_args(m, m->step, &aa, &da);
    int n_sq = 0;
    const bool exchanged = m->comm && !m->timing.enabled;
    // single GPU: the small tensors are updated on the side stream WHILE the word table
    // streams on the main one (independent tensors; every gradient is complete here)
    // (loglinear whose dW stayed on the main stream -- small steps: the W, b update (6-8 us alone) stays there too; its fork
    //  and join cost the main queue 2 x 5.6 us for 25 us of side-stream work: round-5 timeline of the W3C settings)
    const VsStepPlan& P = m->plan;
    // (ll_dw_side: ll_backward sets it only on a single GPU, out of timing mode, with a side stream -- the conditions of
    //  plan.side_small; whoever relaxes them there has to repeat them here)
    const bool side_small = P.side_small || m->ll_dw_side;
    hipStream_t ss = side_small ? m->stream2 : m->stream;
    // what orders the side stream in front of them: nothing (late fork: everything the small tensors need was issued on the
    // side stream itself), the end of the dh GEMM, or a fork of its own here
    const int small_order = m->ll_dw_side ? SERT_VS_EVENT_OPT_FORK : P.small_order;
    if (small_order == SERT_VS_EVENT_OPT_FORK) SERT_HIP(hipEventRecord(m->ev_opt_fork, m->stream));
    if (small_order != SERT_VS_EVENT_NONE) SERT_HIP(hipStreamWaitEvent(ss, vs_event(m, small_order), 0));
    // ---- the big tensors, in the reference's parameter order (models.py:542-543, :1105; the
    // tensors are independent): one streaming launch each -- or, data parallel, one launch per
    // owned piece as soon as its gradient slab has been reduce-scattered, the all-gather of the
    // updated slab right behind it
    bool any_ag = false;
    // plan.defer_re -- side-heavy schedule: the entity table is updated BEHIND the join of the tail (see below)
    // plan.defer_small -- ... and so is a SMALL entity table (C2: 1000 x 128, one optimizer_small launch behind the entity chain on the side
    // stream).  Round 4, from the GPU timeline: that launch -- 4 us alone, 12-31 us beside the word table's Adam -- ended
    // when the Adam did, and the tail started 13 us later, behind the cross-queue join.  The tail needs nothing of it but
    // the sums of squares of R_e, which the PREVIOUS step's launch leaves (of the values it writes: same shares, same
    // order, the same bits -- sumsq_new_partial); the update itself only has to land before the next loss kernel
    // (settle_entity_update), so the main stream no longer joins the side stream at the end of a step.
    const int re_cur = (int)(m->step & 1), re_nxt = re_cur ^ 1;
    const size_t re_cap = (size_t)2 * kOptBlocks;
    bool small_needs_join = !P.defer_small;
    int re_sq_lo = 0, re_nb = 0;
    for (int i = 0; i < 4; ++i) {
        if (!m->pt_big[i]) continue;
        const ParamTensor t = param_tensor(m, i);
        if (t.n == 0) continue;
        const int tg = i == 0 ? TG_OPT_WORD : TG_OPTIMIZER;
        if (i == 1 && P.defer_re) {
            // (its slots in the partial array stay where they are: the tail reads them from re_sq)
            const int64_t max_nb = t.n >= ((size_t)1 << 24) ? 2 * kOptBlocks : kOptBlocks;
            re_nb = (int)std::min<int64_t>(max_nb, cdiv(cdiv(t.n, 4), 256));
            re_sq_lo = n_sq;
            n_sq += re_nb;
            continue;
        }
        if (!(is_dp(m) && m->pt_sharded[i])) {
            ScopedTimer tm(m, tg);
            // (tables of 2^24 elements and more -- C4: 150 M and 30 M -- stream faster over twice the
            //  workgroups: word table 708 -> 644 us, entity table 180 -> 167 us; no difference at
            //  C2's 12.8 M.  The count depends on the tensor size only: same tree in every run.)
            const int64_t max_nb = t.n >= ((size_t)1 << 24) ? 2 * kOptBlocks : kOptBlocks;
            const int nb = (int)std::min<int64_t>(max_nb, cdiv(cdiv(t.n, 4), 256));
            const uint32_t* tf = (i == 0 && m->use_touched) ? bits : nullptr;
            // Where it pays: the catch-up loop costs VALU time, the saving is the rows NOT written.  Measured (round 4,
            // tools/experiments/r04_lazy_sweep.sh; word-table update alone / step): C4, a batch touches 14 % of the rows:
            // 639 -> 530 us / 1.89 -> 1.77 ms; the reference's product-search settings (batch 4096, 12 %): 113 -> 85 us /
            // 231 -> 207 us; its W3C loglinear settings (batch 1024, 5 %): 141 -> 79 us / 331 -> 263 us; C2 dims at batch
            // 16384 (20 %): 58.5 -> 48 us; at C2's own batch (44 %, this or the next batch 69 %) a draw: 61.5 -> 57.5 us
            // alone, the step equal -- dense there.  Lazy up to a touched fraction of 0.35 (SERT_LAZY_MAX in a
            // variants build: 0 = never, 1 = always).
            // Round 5: dense_update_skip does not read the rows nobody needs, and then the lazy form wins at C2 too (a batch
            // touches 44 % of the rows, this or the next one 69 %: 61 -> 53 us per launch on average, 0.271 -> 0.261 ms per
            // step, tools/experiments/r05_skip_c2.sh).  With an announced next batch: lazy up to m->lazy_max (SERT_LAZY_MAX,
            // default 0.5 -- above that nearly every row is needed by this batch or the next and the passes that read
            // everything carry the predictions for nothing); without one every lazy step reads and writes every row, and
            // the dense launch takes over above 0.35 as before.
            const float lazy_max = (next_bits && m->lazy_skip) ? m->lazy_max : std::min(m->lazy_max, 0.35f);
            // (and for tables of 4 M elements and more: a small one lives in the caches, where the dense launch costs
            //  nothing to save -- the reference's C1, 640 k parameters: 91 us dense, 95 us lazy)
            static const bool lazy_small = variant_knob("SERT_LAZY_SMALL_TABLES") != nullptr;
            if (i == 0 && tf && m->rw_last[0] && !c.keep_grads && c.word_dim % 4 == 0 &&
                m->cur_touched_frac <= lazy_max && (t.n >= ((size_t)1 << 22) || lazy_small)) {
                n_sq += launch_lazy_word_update(m, t, tf, next_bits, nb, aa, da, m->red_sq + n_sq);
                continue;
            }
            if (i == 0) m->rw_pred_ok = false;   // (a dense launch moves every row off its predicted trajectory)
            if (i == 0) ++m->upd_counts[0];
            if (i == 0) SERT_TRY(ensure_rw_current(m, -1, m->step - 1));    // (a dense launch assumes every row is at the previous step; m->step is already this update's number)
            // (side_heavy: the entity table streams on the side stream, behind its gradient chain.  Loglinear with dW on the
            //  side stream: a W large enough to be a "big tensor" -- d x V_e >= 2^22, C4 -- is updated THERE, behind dW and
            //  its combine; on the main stream its update read dW's gradient while the side stream was still writing it:
            //  two runs of the C4 loglinear step differed by 0.5 % in W after two steps, tools/experiments/r04_ll_c4_rep.py)
            const bool on_side = (i == 1 && P.re_on_side) || (i >= 2 && m->ll_dw_side);
            launch_stream_opt(m, on_side ? ss : m->stream, t.p, t.g, t.s0, t.s1, t.n, nb, aa, da,
                              m->red_sq + n_sq, tf,
                              i == 0 ? (unsigned)c.word_dim : 1u);
            n_sq += nb;
            continue;
        }
        const size_t sc = m->pt_sc[i];
        const int nch = m->ar_chunks;
        // word table owned by rows: the gradient rows were returned to their owners (xr_return_grads);
        // rows of the owned range no rank touched take a zero gradient without reading it, and nothing
        // is gathered -- the next forward fetches the rows it needs (xr_fetch_params)
        const bool by_rows = (i == 0) && m->xr_on;
        {
            ScopedTimer tm(m, tg);
            for (int ch = 0; ch < nch; ++ch) {
                if (exchanged && m->rs_issued[i]) SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_rs_done[i][by_rows ? 0 : ch], 0));
                const size_t off = piece_off(m, i, ch);
                const int nb = (int)std::min<int64_t>(std::max(1, kOptBlocks / nch), cdiv(cdiv(sc, 4), 256));
                // (the padding behind the tensor's last element is zero with a zero gradient: it stays zero)
                const uint32_t* ub = by_rows ? m->xr_ubits + (size_t)m->xr_batch * (size_t)m->xr->owned_bit_words : nullptr;
                launch_stream_opt(m, m->stream, t.p + off, t.g + off, t.s0 + (size_t)ch * sc, t.s1 + (size_t)ch * sc, sc,
                                  nb, aa, da, m->sq_scratch, ub, by_rows ? (unsigned)c.word_dim : 1u);
                if (by_rows) {
                    // (recorded in every mode: a later step on the communication stream waits for it whatever
                    //  mode THIS step ran in)
                    if (m->ev_word_updated) SERT_HIP(hipEventRecord(m->ev_word_updated, m->stream));
                    m->rw_full = false;
                    m->xr_fetched_batch = -1;
                    continue;
                }
                m->comm_bytes_moved += 8.0 * (double)sc * (double)(m->world - 1);   // all-gather: (N-1) pieces out, (N-1) in
                if (exchanged) {
                    SERT_HIP(hipEventRecord(m->ev_opt_done[i][ch], m->stream));
                    SERT_HIP(hipStreamWaitEvent(m->comm_stream, m->ev_opt_done[i][ch], 0));
                    SERT_NCCL(g_rccl.AllGather(t.p + off, t.p + (size_t)ch * slab_elems(m, i), sc, /*ncclFloat32*/ 7,
                                               m->comm, m->comm_stream));
                    any_ag = true;
                }
            }
        }
        m->rs_issued[i] = false;
        if (by_rows) {
            // (nothing to gather)
        } else if (m->host_ar) {
            ScopedTimer tm(m, TG_ALLGATHER);
            for (int ch = 0; ch < nch; ++ch) SERT_TRY(host_allgather(m, t.p + (size_t)ch * slab_elems(m, i), sc, m->stream));
        } else if (m->comm && m->timing.enabled) {
            ScopedTimer tm(m, TG_ALLGATHER);
            for (int ch = 0; ch < nch; ++ch)
                SERT_NCCL(g_rccl.AllGather(t.p + piece_off(m, i, ch), t.p + (size_t)ch * slab_elems(m, i), sc, 7, m->comm,
                                           m->stream));
        }
    }
    if (exchanged) SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_ar_done, 0));
    if (side_small && egrad_writes_every_row(m) && c.kind == SERT_KIND_VECTORSPACE && !is_fs(m) && c.num_negatives > 0 && !c.keep_grads &&
        m->neg_alt_step != m->step) {
        // the next step's negatives (Philox position = the step counter after this update), drawn
        // here on the side stream unless the step's forward already drew them in front of its fork:
        // ev_small below orders them before anything of the next step
        const int64_t count = (int64_t)c.batch_size * c.num_negatives;
        launch(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0, ss, m->neg_alt, count,
               (int64_t)m->rank * count, (uint32_t)c.num_entities, c.seed, (uint64_t)m->step * 2, nullptr, 0, nullptr, 0);
        m->neg_alt_step = m->step;
    }
    auto small_tensors = [&](hipStream_t ss, unsigned mask) {
        // everything small goes into one launch (a kernel boundary costs more than updating it)
        ScopedTimer t(m, TG_OPTIMIZER);
        SmallTensors st;
        int k = 0, blocks = 0;
        for (int i = 1; i < 4; ++i) {
            const ParamTensor t2 = param_tensor(m, i);
            if (m->pt_big[i] || t2.n == 0 || !((mask >> i) & 1u)) continue;
            st.p[k] = t2.p; st.g[k] = t2.g; st.s0[k] = t2.s0; st.s1[k] = t2.s1; st.count[k] = t2.n;
            const bool parts = (i == 1) && P.re_in_parts;
            st.gparts[k] = parts ? m->epart : nullptr;
            st.ngroups[k] = parts ? m->eg_groups : 0;
            st.gstride[k] = parts ? (unsigned long long)m->n_re : 0ull;
            st.l2k[k] = t2.l2 ? l2k : 0.f;
            st.first_block[k] = blocks;
            blocks += (int)std::min<int64_t>(512, cdiv(t2.n, 256));
            ++k;
        }
        for (int i = k; i < 3; ++i) { st.p[i] = st.g[i] = st.s0[i] = st.s1[i] = nullptr; st.count[i] = 0; st.l2k[i] = 0.f; st.gparts[i] = nullptr; st.ngroups[i] = 0; st.gstride[i] = 0; }
        for (int i = k; i <= 3; ++i) st.first_block[i] = blocks;
        float* sq = m->red_sq + n_sq;
        float* sq_new = nullptr;
        if (P.defer_small && mask == 0x2u && blocks > 0) {
            // (R_e alone in this launch: its partial slots [n_sq, n_sq + blocks) are read from re_sq by the tail)
            re_sq_lo = n_sq;
            re_nb = blocks;
            sq_new = m->re_sq + re_nxt * re_cap;
            if (m->re_sq_for[re_cur] != m->step) {
                // no previous launch left this step's sums (first step, another schedule in between, the host replaced
                // the table): the same partials from a read-only pass IN FRONT of the update, and the tail joins once
                launch(sumsq_like_small, dim3(blocks), dim3(256), 0, ss, (const float*)m->re, m->n_re, l2k,
                       m->re_sq + re_cur * re_cap);
                m->re_sq_for[re_cur] = m->step;
                small_needs_join = true;
                ++m->state_counts[5];
            } else {
                ++m->state_counts[4];
            }
        }
        if (blocks > 0) {
            const bool keep = c.keep_grads != 0;
            if (is_vs(m) && sq_new) {
                launch((optimizer_small<true, false>), dim3(blocks), dim3(256), 0, ss, st, aa, da, sq, sq_new);
            } else if (is_vs(m)) {
                if (keep) launch((optimizer_small<true, true>), dim3(blocks), dim3(256), 0, ss, st, aa, da, sq, nullptr);
                else      launch((optimizer_small<true, false>), dim3(blocks), dim3(256), 0, ss, st, aa, da, sq, nullptr);
            } else {
                if (keep) launch((optimizer_small<false, true>), dim3(blocks), dim3(256), 0, ss, st, aa, da, sq, nullptr);
                else      launch((optimizer_small<false, false>), dim3(blocks), dim3(256), 0, ss, st, aa, da, sq, nullptr);
            }
        }
        n_sq += blocks;
    };
    if (P.combine_in_tail) {
        small_tensors(ss, 0x2u);          // R_e; W and b are updated by the tail launch below
    } else if (P.split_small) {
        // Late fork: dW / db were produced on the main stream, dR_e on the side
        // stream -- W and b are updated on the main stream, R_e on the side stream, no event between.
        small_tensors(m->stream, 0xCu);   // W, b
        small_tensors(ss, 0x2u);          // R_e
    } else {
        small_tensors(ss, 0xEu);
    }
    if (P.defer_re) ++m->state_counts[m->re_sq_for[re_cur] != m->step ? 6 : 4];
    if (P.defer_re && m->re_sq_for[re_cur] != m->step) {
        // no previous deferred launch left this step's sums (first step, another schedule in between, the
        // host replaced the table): the same partials from a read-only pass, in front of the join
        launch(sumsq_like_adam, dim3(re_nb), dim3(256), 0, ss, (const float*)m->re, m->n_re, m->re_sq + re_cur * re_cap);
        m->re_sq_for[re_cur] = m->step;
    }
    if (side_small && small_needs_join) {
        SERT_HIP(hipEventRecord(m->ev_small, ss));
        SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_small, 0));
    }
    if (P.defer_small && re_nb > 0) {
        // the update is in the side stream; the next reader of R_e (and, through this stream's order, of the negatives
        // drawn in front of this step's fork) waits for it in settle_entity_update
        m->re_sq_for[re_nxt] = m->step + 1;
        SERT_HIP(hipEventRecord(m->ev_re, ss));
        m->re_pending = true;
    }
    // The entity table's L2 + Adam, behind the join: the tail does not wait for it.  Nothing reads R_e, its state or dR_e before the next
    // loss kernel (settle_entity_update), so it streams its 0.96 GB beside the next step's gather and projection GEMM.  It also leaves
    // the sums of squares of the UPDATED table: the next step's regularisation term.
    if (P.defer_re) {
        const ParamTensor t = param_tensor(m, 1);
        launch_stream_opt(m, ss, t.p, t.g, t.s0, t.s1, t.n, re_nb, aa, da, m->red_sq + re_sq_lo, nullptr, 1u,
                          m->re_sq + re_nxt * re_cap);
        m->re_sq_for[re_nxt] = m->step + 1;
        SERT_HIP(hipEventRecord(m->ev_re, ss));
        m->re_pending = true;
    }
    {
        ScopedTimer t(m, TG_FINALIZE);
        const float inv_batch = 1.0f / (float)c.global_batch_size;
        const float reg_scale = c.lambda_ > 0.f ? c.lambda_ / (2.0f * (float)c.global_batch_size) : 0.f;
        // single GPU: the loss partials directly; data parallel: the all-reduced scalars (loss
        // sum; sum of squares of the sharded tensors -- the replicated ones come from red_sq)
        const float* lp = is_dp(m) ? m->g_loss : (m->loss_from_rows ? m->rowloss : m->red_loss);
        const int nl = is_dp(m) ? 1 : n_loss_partials;
        unsigned* flag = publish ? reinterpret_cast<unsigned*>(loss_dst + 4) : nullptr;
        if (P.combine_in_tail) {
            if (P.dense_event == SERT_VS_EVENT_DENSE) SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_dense, 0));   // (dW / db slabs: side stream)
            TailArgs ta;
            ta.part = m->part; ta.splits = m->dw_splits; ta.stride = m->tail_stride;
            ta.W = m->W; ta.b = m->b; ta.s0_w = m->s0_w; ta.s1_w = m->s1_w; ta.s0_b = m->s0_b; ta.s1_b = m->s1_b;
            ta.g_w = m->g_w; ta.g_b = m->g_b;
            ta.n_w = (unsigned)m->n_w; ta.n_b = (unsigned)m->n_b;
            ta.aa = aa;
            ta.loss_partials = lp; ta.n_loss = nl;
            ta.sq_partials = m->red_sq; ta.n_sq = n_sq;
            const bool alt = P.defer_re || (P.defer_small && re_nb > 0);
            ta.sq_alt = alt ? m->re_sq + re_cur * re_cap : nullptr;
            ta.sq_alt_lo = alt ? re_sq_lo : 0;
            ta.sq_alt_hi = alt ? re_sq_lo + re_nb : 0;
            ta.inv_batch = inv_batch; ta.reg_scale = reg_scale;
            ta.out = loss_dst; ta.host_flag = flag; ta.seq = publish ? ++m->loss_seq : 0u;
            ta.blk = m->tail_blk;
            if (++m->tail_launch_seq == 0) ++m->tail_launch_seq;   // (0 = "never written")
            ta.launch_seq = m->tail_launch_seq;
            const int nb = cdiv((int64_t)(m->n_w + m->n_b), 64);
            if (m->tail_defer && publish && !c.keep_grads) {
                // a hinted step: the gather launch of the run-ahead step carries these workgroups (vs_project); the wait
                // for ev_dense above stays where it is -- it also keeps that gather from overwriting H under dW
                m->tail_args = ta;
                m->tail_nb = nb;
                m->tail_pending = true;
            } else {
                ++m->tail_counts[0];
                if (c.keep_grads) launch((vs_tail<true>), dim3(nb), dim3(1024), 0, m->stream, ta);
                else              launch((vs_tail<false>), dim3(nb), dim3(1024), 0, m->stream, ta);
            }
        } else
        launch(finalize_loss, dim3(1), dim3(256), 0, m->stream, lp, nl, m->red_sq,
               n_sq, inv_batch, reg_scale, loss_dst, flag, publish ? ++m->loss_seq : 0u,
               is_dp(m) ? (const float*)m->g_sq : (const float*)nullptr);
    }
    if (any_ag) {
        // the loss leaves first; the next kernel that reads a parameter waits for the last slab
        SERT_HIP(hipEventRecord(m->ev_ag_done, m->comm_stream));
        SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_ag_done, 0));
    }
    return 0;
}

// First element of the gradient buffer the step's prologue has to zero when the word table needs no
// zeroing: behind g_rw -- and behind g_re too where the sorted entity-gradient chain runs, which writes
// EVERY row of dR_e (a run inside one chunk by the chunk, a longer one by the fix-up, an entity without a
// pair as zeros by the fix-up): 120 MB less to write per step at C4.
static size_t zero_from(const sert_model* m) {
    static const bool all = variant_knob("SERT_ZERO_GRE") != nullptr;   // cross-check knob
    if (!all && m->cfg.kind == SERT_KIND_VECTORSPACE && !m->epart && m->n_re > 0 && m->g_re == m->gflat + m->ar_split)
        return m->ar_split + round_up(m->pt_pad[1], 4);
    return m->ar_split;
}

// The entity-gradient chain writes EVERY row of dR_e (the sort-free path by construction, the sorted one through its fix-up):
// a step whose negatives were drawn ahead then needs no prologue launch at all.
static bool egrad_writes_every_row(const sert_model* m) { return m->epart != nullptr || zero_from(m) > m->ar_split; }

static bool fused_prologue_applies_with(const sert_model* m, bool touched) {
    return is_vs(m) && !is_fs(m) && !m->timing.enabled && m->nstreams >= 2 && touched &&
           m->cfg.num_negatives > 0 && (m->gflat_alloc - zero_from(m)) % 4 == 0;
}
static bool fused_prologue_applies(const sert_model* m) { return fused_prologue_applies_with(m, m->use_touched); }
// sampler of optimiser step m->step + zeroing of the small gradient buffers
static void launch_fused_prologue(sert_model* m) {
    const int64_t count = (int64_t)m->cfg.batch_size * m->cfg.num_negatives;
    launch(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0, m->stream, m->neg,
           count, (int64_t)m->rank * count, (uint32_t)m->cfg.num_entities, m->cfg.seed,
           (uint64_t)m->step * 2, reinterpret_cast<float4*>(m->gflat + zero_from(m)),
           (m->gflat_alloc - zero_from(m)) / 4, (uint4*)nullptr, (size_t)0);
}

static bool use_touched_now(const sert_model* m) {
    static const bool no_touched = knob("SERT_NO_TOUCHED") != nullptr;   // cross-check knob
    return !no_touched && !is_dp(m) && !m->cfg.keep_grads && m->cfg.word_dim % 4 == 0 &&
           m->n_rw < ((size_t)1 << 32) && m->split[SERT_SPLIT_TRAIN].idx_touched_bits != nullptr;
}

// Everything of a training step that does NOT change the model: forward, loss, backward into
// the gradient scratch (all of it a function of parameters, data and step counter only).
// `fused_pre_out`: whether the step took the fused main-stream prologue.
static int step_forward_backward(sert_model* m, const DataSplit& ds, int64_t batch_index,
                                 const int64_t* negatives, bool* fused_pre_out) {
    // Single GPU: the word-gradient table is not zeroed -- the segmented reduction flags
    // the rows it writes and the optimiser takes every other row's gradient as zero.
    // (Data parallel: the all-reduce needs the dense table; keep_grads: so does the caller.)
    m->use_touched = use_touched_now(m);
    SERT_TRY(ensure_rw_current(m, batch_index));   // (lazy word-table update: the rows this batch reads must be current)
    // Prologue (zeroing, negative sampling): nothing before the loss kernel needs it, so
    // for the vectorspace step it runs on the side stream beside gather + projection.
    m->ll_dw_side = false;
    const bool side_pre = is_vs(m) && !is_fs(m) && !m->timing.enabled && m->nstreams >= 2;
    // One fused prologue launch on the MAIN stream (sampler + zeroing of the small gradient
    // buffers and the row flags) when nothing big has to be zeroed and the device draws the
    // negatives: no side-stream prologue, no cross-queue wait in front of the loss kernel.
    // negatives drawn at the end of the previous step for exactly this step: nothing to do (the
    // sort-free entity-gradient path needs no zeroed buffer either: every row it owns is written)
    // (round 5: also behind the SORTED chain of a big entity table -- the product-search settings, C4 --, whose steps used to
    //  start with a sampler + zeroing launch on the main stream, 6 us + a queue bubble: nothing it zeroed is read there)
    const bool have_neg = negatives == nullptr && egrad_writes_every_row(m) && m->neg_alt_step == m->step && side_pre &&
                          fused_prologue_applies(m);
    if (have_neg) {
        std::swap(m->neg, m->neg_alt);
        m->neg_alt_step = -1;
    }
    // The step's schedule (step_plan.h), decided once.  (have_neg: this step's negatives are complete in the side stream's order)
    m->plan_facts = vs_step_facts(m, ds, have_neg);
    m->plan = vs_plan_step(m->plan_facts);
    const bool fused_pre = side_pre && negatives == nullptr && fused_prologue_applies(m);
    hipStream_t pre = (side_pre && !fused_pre) ? m->stream2 : m->stream;
    *fused_pre_out = (pre == m->stream);   // no side-stream prologue: no end-of-step event needed
    if (pre != m->stream && m->step_done_pending) {
        // a side-stream prologue must follow the previous step, which (fused prologue) did not
        // mark its end: nothing of this step is on the main stream yet, so mark it now
        SERT_HIP(hipEventRecord(m->ev_step_done, m->stream));
        m->step_done_pending = false;
    }
    // data parallel, word table owned by rows: the rows this batch touches arrive from their owners
    if (m->xr_on) {
        m->xr_batch = batch_index;
        SERT_TRY(xr_fetch_params(m, batch_index));
    }
    // the main stream's first kernels go out BEFORE the prologue's host calls: the GPU
    // starts on gather + projection while the host is still enqueueing
    if (is_vs(m) && !is_fs(m)) {
        if (m->projected_batch != batch_index) SERT_TRY(vs_project(m, ds, batch_index));
        m->projected_batch = -1;
    }
    SERT_TRY(settle_entity_update(m));   // (the prologue zeroes dR_e, the loss kernel reads R_e)
    if (have_neg) {
        // (no prologue launch at all)
    } else if (fused_pre) {
        launch_fused_prologue(m);
    } else {
        // (the previous step's optimiser and loss kernels read what the prologue overwrites)
        if (pre != m->stream) SERT_HIP(hipStreamWaitEvent(pre, m->ev_step_done, 0));
        if (m->use_touched && !is_vs(m) && !is_dp(m)) {
            // loglinear, single GPU: NOTHING to zero -- the word table's gradient is read through the touched-row bitmap, and
            // g_W / g_b are written in full by the split-K combine behind dW (ll_backward); the 5 us memset was a launch of
            // its own on the chain of an 18-kernel step (the reference's W3C settings: round-5 timeline)
        } else if (m->use_touched || m->xr_on) {
            // (by rows: dR_w is written where this rank's batch touches, read where the lists say, and
            //  the owned rows nobody touched are never read -- the table needs no zeroing)
            SERT_HIP(hipMemsetAsync(m->gflat + zero_from(m), 0, (m->gflat_alloc - zero_from(m)) * sizeof(float), pre));
        } else {
            SERT_HIP(hipMemsetAsync(m->gflat, 0, m->gflat_alloc * sizeof(float), pre));
        }
        // (vectorspace with a side-stream prologue: BEHIND the negatives and their event, see below)
        if (!(is_vs(m) && !is_fs(m) && pre != m->stream)) SERT_TRY(owned_sum_of_squares(m, pre));
    }
    if (is_fs(m)) {
        SERT_TRY(fs_forward<true>(m, ds, batch_index));
        SERT_TRY(fs_backward(m, ds, batch_index));
        SERT_TRY(reduce_rowloss(m, m->stream));
    } else if (is_vs(m)) {
        if (!fused_pre) SERT_TRY(vs_negatives(m, negatives, (uint64_t)m->step * 2, pre));
        if (pre != m->stream) {
            SERT_HIP(hipEventRecord(m->ev_neg, pre));
            SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_neg, 0));
            // Data parallel: the sums of squares of the owned pieces (the regularisation term's share of this rank: a pass
            // over the owned slice of every sharded tensor + one combine) only feed the all-reduce of the replicated rest,
            // which joins this stream much later -- they used to sit IN FRONT of the negatives, and the loss kernel waited
            // for all of it (round-5 timeline at C2, world of one: the loss kernel 25 us behind the projection).
            if (!have_neg && !fused_pre) SERT_TRY(owned_sum_of_squares(m, pre));
        }
        SERT_TRY(vs_loss<true>(m, ds, batch_index));
        SERT_TRY(vs_backward(m, ds, batch_index));   // (loss partials: beside dW)
    } else {
        SERT_TRY(ll_forward<true>(m, ds, batch_index));
        SERT_TRY(ll_backward(m, ds, batch_index));
        SERT_TRY(reduce_rowloss(m, m->stream));
    }
    return 0;
}

// May the forward + backward of a hinted next batch run ahead of the host (before the loss
// of the current step has been read)?  It touches nothing but activations and gradient scratch.
// Single GPU: product settings, device sampler.  Data parallel (round 6): as well -- the run-ahead then includes the
// collectives of the backward (the gradient rows' all-to-all / the reduce-scatter), which is safe because every rank
// sees the same sequence of hints and batches (the global batch order is rank-invariant, SURVEY 8-e) and therefore
// issues, keeps or discards the same run-ahead; the parameter fetch of the hinted batch was already issued this way.
// Without it the data-parallel step was HOST-bound: its ~45 runtime calls only started when the previous loss had
// arrived (world of one, 8192 rows: 0.174 ms against 0.096 on one GPU; profiles/r06_experiments.txt item 4).
// SERT_DP_RUN_AHEAD=0 (variants build) restores the round-5 behaviour.
static bool can_speculate_step(const sert_model* m) {
    if (m->timing.enabled || m->cfg.keep_grads) return false;
    if (is_dp(m)) {
        static const bool dp_off = variant_knob("SERT_DP_RUN_AHEAD") && atoi(variant_knob("SERT_DP_RUN_AHEAD")) == 0;
        return !dp_off && is_vs(m) && !is_fs(m);
    }
    if (is_vs(m) && !is_fs(m)) return use_touched_now(m) && fused_prologue_applies_with(m, true);
    return true;   // loglinear / full-softmax: the whole step lives on the main stream
}

// Will sert_train_batch send the whole forward + backward of the announced batch `hint` out behind the step it is issuing?
// ONE predicate for the two places that must agree: prefetch_next, which does it, and the deferral of the step's tail
// launch into that run-ahead's gather launch.
static bool will_run_ahead(const sert_model* m, int64_t hint) {
    return hint >= 0 && (hint + 1) * (int64_t)m->cfg.batch_size <= m->split[SERT_SPLIT_TRAIN].N && can_speculate_step(m);
}

static int train_step_async(sert_model* m, int64_t batch_index, const int64_t* negatives,
                            float* loss_dst, bool publish = false) {
    const DataSplit& ds = m->split[SERT_SPLIT_TRAIN];
    const int B = m->cfg.batch_size;
    if (m->cfg.inference_only) SERT_FAIL("model was created inference_only");
    if (m->comm_dead) SERT_FAIL("the communicator of this data-parallel model was destroyed");
    if (ds.N == 0) SERT_FAIL("no training data uploaded");
    if (batch_index < 0 || (batch_index + 1) * (int64_t)B > ds.N) SERT_FAIL("batch_index out of range");
    if (m->instep.on) ++m->instep.steps;
    // what the previous call already ran ahead for this step (sert_hint_next_batch)
    const bool have_fb = negatives == nullptr && m->spec_fb_batch == batch_index && m->spec_fb_step == m->step &&
                         can_speculate_step(m);
    bool fused_pre = true;   // (a speculated step always ran its prologue on the main stream)
    if (have_fb) { m->spec_fb_batch = -1; ++m->state_counts[1]; }   // consumed
    else discard_run_ahead(m);              // a run-ahead for something else: discard it cleanly
    const uint32_t* bits = ds.idx_touched_bits ? ds.idx_touched_bits + (size_t)batch_index * ds.bit_words : nullptr;
    if (!have_fb) SERT_TRY(step_forward_backward(m, ds, batch_index, negatives, &fused_pre));
    SERT_TRY(allreduce_rest(m));
    m->cur_touched_frac = (size_t)batch_index < ds.idx_batches.size()
                              ? (float)ds.idx_batches[(size_t)batch_index].num_distinct / (float)m->cfg.vocab_size : 1.f;
    // the rows the ANNOUNCED next batch touches: the lazy word-table update keeps them current (sert_hint_next_batch)
    const uint32_t* next_bits = nullptr;
    if (ds.idx_touched_bits && m->lazy_next >= 0 && (m->lazy_next + 1) * (int64_t)B <= ds.N)
        next_bits = ds.idx_touched_bits + (size_t)m->lazy_next * ds.bit_words;
    SERT_TRY(optimizer_and_loss(m, loss_dst, publish, bits, next_bits));
    if (is_dp(m)) m->comm_steps += 1;
    SERT_HIP(hipGetLastError());   // a rejected launch (bad configuration) surfaces here, not as a hang
    // (an event record stalls its queue for ~6 us: steps with the fused prologue skip it)
    if (fused_pre) m->step_done_pending = true;
    else { SERT_HIP(hipEventRecord(m->ev_step_done, m->stream)); m->step_done_pending = false; }
    return 0;
}
