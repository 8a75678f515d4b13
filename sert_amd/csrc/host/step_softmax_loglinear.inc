// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): the additive full-softmax variant and the loglinear step.

// ---- the full-softmax vectorspace variant (additive) ----------------------------
template <bool TRAIN>
static int fs_forward(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, dw = c.word_dim, de = c.entity_dim, V = c.num_entities;
    const size_t row0 = (size_t)batch_index * B;
    {
        ScopedTimer t(m, TG_GATHER);
        SERT_ID_DISPATCH(c.id_bytes, {
            const IdT* X = (const IdT*)ds.x + row0 * n;
            gather_mean(m->stream, X, m->rw, m->H, B, n, dw);
        });
    }
    {
        ScopedTimer t(m, TG_GEMM_FWD);
        launch_gemm<false, false, EPI_BIAS_TANH>(m->stream, m->H, m->W, m->T, m->b, B, de, dw, dw, de, de);
        // p = clip(t) ; logits = p.R_e^T   (B, V)
        launch(vs_clip, dim3(grid_for((int64_t)B * de)), dim3(256), 0, m->stream, m->T, m->DH2,
               (size_t)B * de);
    }
    const float inv_batch = 1.0f / (float)c.global_batch_size;
    const int tile = m->fs_tile > 0 ? m->fs_tile : B;
    for (int r0 = 0; r0 < B; r0 += tile) {
        const int rows = std::min(tile, B - r0);
        {
            ScopedTimer t(m, TG_GEMM_FWD);
            launch_gemm<false, true, EPI_STORE>(m->stream, m->DH2 + (size_t)r0 * de, m->re, m->Z, nullptr, rows, V, de, de, de, V);
        }
        {
            ScopedTimer t(m, TG_LOSS);
            // rows up to 2048 entities stay in registers (one read, one write)
#define SERT_FS_CE(EPL)                                                                                   \
    launch((fs_softmax_ce<TRAIN, EPL>), dim3(cdiv(rows, 4)), dim3(256), 0, m->stream, m->Z,             \
           ds.y + row0 + r0, TRAIN ? ds.w + row0 + r0 : nullptr, m->rowloss + r0, rows, V, inv_batch)
            if (V <= 64 * 16)      SERT_FS_CE(16);
            else if (V <= 64 * 32) SERT_FS_CE(32);
            else                   SERT_FS_CE(0);
#undef SERT_FS_CE
        }
        if (TRAIN && tile < B) {
            // row tiles: this tile's share of the backward that needs its dZ, before the next tile's
            // logits overwrite it -- dR_e += dZ_t^T.p_t (the first tile stores), dp_t = dZ_t.R_e
            {
                ScopedTimer t(m, TG_EGRAD);
                if (r0 == 0)
                    launch_gemm<true, false, EPI_STORE>(m->stream, m->Z, m->DH2, m->g_re, nullptr, V, de, rows, V, de, de);
                else
                    launch_gemm<true, false, EPI_ACCUM>(m->stream, m->Z, m->DH2 + (size_t)r0 * de, m->g_re, nullptr, V, de, rows, V, de, de);
            }
            {
                ScopedTimer t(m, TG_GEMM_DX);
                SERT_TRY((gemm_long_k<false, false>(m->skbuf, m->stream, m->Z, m->re, m->DA + (size_t)r0 * de, rows, de, V, V, de)));
            }
        }
    }
    return 0;
}

static int fs_backward(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, dw = c.word_dim, de = c.entity_dim, V = c.num_entities;
    const bool tiled = m->fs_tile > 0 && m->fs_tile < B;   // (fs_forward already consumed every tile's dZ)
    if (!tiled) {
        // dR_e (V, d_e) = dZ^T.p : reduction over the batch, split-K, order-fixed combine
        ScopedTimer t(m, TG_EGRAD);
        const int tiles = cdiv(de, GN) * cdiv(V, GM);
        int splits = std::max(1, std::min(cdiv(B, GK), cdiv(1024, tiles)));
        int kper = (int)round_up(cdiv(B, splits), GK);
        splits = cdiv(B, kper);
        const size_t mn = (size_t)V * de;
        launch_gemm<true, false, EPI_STORE>(m->stream, m->Z, m->DH2, m->part, nullptr, V, de, B, V, de, de,
                                            splits, kper, mn);
        launch_reduce_partials(m->stream, m->part, splits, mn,
                           mn, m->g_re, mn, m->g_re);
    }
    {
        // dp = dZ.R_e (B, d_e) ; da = dp * clip'(t) * tanh'(a)
        ScopedTimer t(m, TG_GEMM_DX);
        if (!tiled) SERT_TRY((gemm_long_k<false, false>(m->skbuf, m->stream, m->Z, m->re, m->DA, B, de, V, V, de)));
        launch(vs_tanh_backward, dim3(grid_for((int64_t)B * de)), dim3(256), 0, m->stream, m->DA,
               m->T, (size_t)B * de);
    }
    {
        static const int want_splits = [] { const char* e = variant_knob("SERT_DW_SPLITS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 1024; }();
        int splits = std::min(want_splits, cdiv(B, GK));
        int kper = (int)round_up(cdiv(B, splits), GK);
        splits = cdiv(B, kper);
        const size_t mn = (size_t)dw * de;
        const size_t stride = mn + de;
        {
            ScopedTimer t(m, TG_GEMM_DW);
            launch_gemm<true, false, EPI_STORE, true>(m->stream, m->H, m->DA, m->part, nullptr, dw, de, B, dw, de,
                                                      de, splits, kper, stride);
        }
        {
            ScopedTimer t(m, TG_SPLITK);
            launch_reduce_partials(m->stream, m->part, splits,
                               stride, stride, m->g_w, mn, m->g_b);
        }
        launch_gemm<false, true, EPI_STORE>(m->stream, m->DA, m->W, m->DH, nullptr, B, dw, de, de, de, dw);
    }
    {
        ScopedTimer t(m, TG_SCATTER);
        SERT_TRY(word_grad_segsum(m, ds, batch_index, m->DH, (float)n));
    }
    SERT_TRY(allreduce_word_grad(m));
    return 0;
}

// ---- the loglinear step -------------------------------------------------------
// Streaming loss for entity vocabularies beyond the LDS-resident slab (kernels_ll.h).
template <bool TRAIN, bool V4>
static int ll_stream_loss(sert_model* m, const DataSplit& ds, size_t row0, const int32_t* y,
                          const int64_t* indptr, const float* w, float inv_batch, const int32_t* slot) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, V = c.num_entities;
    const int64_t rows = (int64_t)B * n;
    const int nseg = cdiv(V, kLlSeg);
    hipStream_t s = m->stream;
    if (TRAIN && !ds.labfix) SERT_FAIL("training split has no label scratch");
    float* labfix = TRAIN ? ds.labfix + (y ? row0 : 0) : nullptr;
    // slot: the logits live in the distinct-word table Zu (U rows); the per-token log-sum-exp
    // is then a per-WORD quantity, and dL/dZ of every token goes to Z
    const float* logits = slot ? m->Zu : m->Z;
    const int64_t lrows = slot ? m->ll_U : rows;
    launch((ll_s_tokstat<V4>), dim3((unsigned)(lrows * nseg)), dim3(256), 0, s, logits, V, nseg, m->ll_tokstat);
    launch(ll_s_lse, dim3(cdiv(lrows, 4)), dim3(256), 0, s, m->ll_tokstat, lrows, nseg, m->ll_lse);
    launch((ll_s_window<V4>), dim3((unsigned)((int64_t)B * nseg)), dim3(256), 0, s, logits, m->ll_lse, n, V,
           nseg, m->J, m->ll_jstat, slot);
    launch((ll_s_rowloss<TRAIN>), dim3(B), dim3(256), 0, s, m->J, m->ll_jstat, y, indptr,
           ds.csr_indices, ds.csr_data, w, m->rowloss, m->ll_rowinfo, labfix, V, nseg, inv_batch);
    if (!TRAIN) return 0;
    launch((ll_s_dj<V4>), dim3((unsigned)((int64_t)B * nseg)), dim3(256), 0, s, m->J, m->ll_rowinfo, V, nseg);
    launch(ll_s_labfix, dim3(B), dim3(256), 0, s, m->J, y, indptr, ds.csr_indices, labfix, V);
    launch((ll_s_tokr<V4>), dim3((unsigned)(rows * nseg)), dim3(256), 0, s, logits, m->ll_lse, m->J, n, V,
           nseg, m->ll_rpart, slot);
    launch(ll_s_rsum, dim3(cdiv(rows, 4)), dim3(256), 0, s, m->ll_rpart, rows, nseg, m->ll_r);
    if (slot) {
        // distinct-word mode: stop here -- dJ (in J) and r_ik are all the per-word backward
        // needs (dzu_from_dj); the per-token dL/dZ pass and its 2 x B*n*V_e floats are skipped.
        // The word rows must hold LOG-probabilities for the finishing transform:
        launch(ll_s_logp_rows, dim3((unsigned)(lrows * nseg)), dim3(256), 0, s, m->Zu, m->ll_lse, V, nseg);
        return 0;
    }
    launch((ll_s_dz<V4>), dim3((unsigned)(rows * nseg)), dim3(256), 0, s, m->Z, m->ll_lse, m->J, m->ll_r, n,
           V, nseg);
    return 0;
}

template <bool TRAIN>
static int ll_forward(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, d = c.word_dim, V = c.num_entities;
    const size_t row0 = (size_t)batch_index * B;
    const int64_t rows = (int64_t)B * n;
    const size_t fused_lds = ((size_t)n * V + V) * sizeof(float);
    // (the label bound is the capacity of the fused kernels' per-thread fix-up lists, whichever NT is launched below:
    //  kernels_ll.h, kLlFusedLabels / LlLabelFix)
    const bool fused = fused_lds <= 150 * 1024 && ds.max_labels_per_row <= kLlFusedLabels;
    m->ll_form[0] = SERT_LL_FORM_NONE; m->ll_form[1] = 0; m->ll_form[2] = TRAIN ? 1 : 0;
    // Duplicate tokens share their logit row (Z[r,:] = R_w[X[r],:].W + b depends on the word
    // only): in a training step the gather and all three GEMMs run on the batch's DISTINCT
    // words (Zipfian batches: a third of the tokens), the loss kernel reads the table through
    // the per-token slot, and dL/dZ is summed per word before the backward GEMMs.
    static const bool no_dedup = knob("SERT_LL_NODEDUP") != nullptr;   // cross-check knob
    static const bool rowwise = variant_knob("SERT_LL_ROWWISE") != nullptr;
    // (evaluation passes over the TRAINING split -- train_error() -- have the index too)
    static const bool eval_dedup = variant_knob("SERT_LL_NO_EVAL_DEDUP") == nullptr;
    m->ll_dedup = (TRAIN || eval_dedup) && (fused || !rowwise) && !no_dedup && ds.idx_slots != nullptr &&
                  (size_t)batch_index < ds.idx_batches.size();
    const BatchIndex* bx = m->ll_dedup ? &ds.idx_batches[(size_t)batch_index] : nullptr;
    m->ll_U = bx ? bx->num_distinct : 0;
    const int64_t grows = m->ll_dedup ? m->ll_U : rows;          // rows of the gathered operand
    {
        ScopedTimer t(m, TG_GATHER);
        if (m->ll_dedup) {
            const uint32_t* U = reinterpret_cast<const uint32_t*>(ds.idx_uwords + bx->uw_off);
            gather_rows(m->stream, U, m->rw, m->G, grows, d);
        } else {
            SERT_ID_DISPATCH(c.id_bytes, {
                const IdT* X = (const IdT*)ds.x + row0 * n;
                gather_rows(m->stream, X, m->rw, m->G, rows, d);
            });
        }
    }
    {
        ScopedTimer t(m, TG_GEMM_FWD);
        launch_gemm<false, false, EPI_BIAS>(m->stream, m->G, m->W, m->ll_dedup ? m->Zu : m->Z, m->b, (int)grows,
                                            V, d, d, V, V);
    }
    const float inv_batch = 1.0f / (float)c.global_batch_size;
    const int32_t* y = ds.y ? ds.y + row0 : nullptr;
    const int64_t* indptr = ds.csr_indptr ? ds.csr_indptr + row0 : nullptr;
    const float* w = TRAIN ? ds.w + row0 : nullptr;
    const int32_t* slot = m->ll_dedup ? ds.idx_slots + (size_t)batch_index * rows : nullptr;
    m->ll_form[3] = slot ? 1 : 0;
    m->ll_form[4] = fused ? 0 : cdiv(V, kLlSeg);
    // fused path: the row's (n, V) slab lives in LDS; a split with a CSR row of > kLlFusedLabels labels falls back
    if (fused) {
        ScopedTimer t(m, TG_LOSS);
        if (m->ll_dedup) logsoftmax_rows(m->stream, m->Zu, grows, V);   // the per-token log-softmax, once per distinct word
        // 512 threads per row: 302 us at 256 (too few waves to hide the slab load), 228 at
        // 512, 320 at 640 (one wave per token, but only two workgroups fit a CU)
        // (distinct-word mode: the kernel writes dJ_i into J and r_ik into ll_r instead of dL/dZ)
        static const bool slab = variant_knob("SERT_LL_SLAB") != nullptr;   // cross-check knob
        if (TRAIN && m->ll_dedup && n <= kLlTableWindow && !slab) {
            // distinct-word mode: no LDS slab, the n table rows are read once, coalesced along e
            const size_t lds = ((size_t)V + n) * sizeof(float);
            // a row is latency-bound (a handful of barriers), not work-bound: 128-thread workgroups
            // put four times as many rows on a CU -- loss kernel 307 -> 111 us at batch 65536, V_e = 100;
            // 86 -> 75 us at V_e = 1000, 139 -> 134 us at 2000 (batch 8192)
            static const int nt128_below = variant_knob("SERT_LL_NT128_BELOW") ? atoi(variant_knob("SERT_LL_NT128_BELOW")) : 2048;   // tuning knob
            // up to 2048 entities (V_e % 4 == 0): one WAVE per row, the row in registers, no LDS and no barrier
            static const bool no_wave = variant_knob("SERT_LL_NO_ROW_WAVE") != nullptr;   // cross-check knob
#define SERT_LL_WAVE(E)                                                                                        \
    m->ll_form[0] = SERT_LL_FORM_WAVE; m->ll_form[1] = E;                                                       \
    launch((ll_row_wave<E>), dim3(cdiv(B, 4)), dim3(256), 0, m->stream, (const float*)m->Zu, slot, y,             \
           indptr, ds.csr_indices, ds.csr_data, w, m->rowloss, B, n, V, inv_batch, m->J, m->ll_r)
            // (its row fetches are buffer loads off one descriptor of the table: 32-bit byte offsets)
            if (!no_wave && V % 4 == 0 && V <= 2048 && (size_t)m->ll_U * V * sizeof(float) < ((size_t)1 << 32)) {
                const int e4 = cdiv(V / 4, 64);
                if (e4 <= 1) { SERT_LL_WAVE(1); }
                else if (e4 <= 2) { SERT_LL_WAVE(2); }
                else if (e4 <= 4) { SERT_LL_WAVE(4); }
                else { SERT_LL_WAVE(8); }
            } else
#undef SERT_LL_WAVE
            if (V <= nt128_below) {
                m->ll_form[0] = SERT_LL_FORM_TABLE; m->ll_form[1] = 128;
                launch((ll_row_from_table<128>), dim3(B), dim3(128), lds, m->stream, (const float*)m->Zu,
                       slot, y, indptr, ds.csr_indices, ds.csr_data, w, m->rowloss, n, V, inv_batch,
                       m->J, m->ll_r);
            } else {
                m->ll_form[0] = SERT_LL_FORM_TABLE; m->ll_form[1] = 512;
                launch((ll_row_from_table<512>), dim3(B), dim3(512), lds, m->stream, (const float*)m->Zu,
                       slot, y, indptr, ds.csr_indices, ds.csr_data, w, m->rowloss, n, V, inv_batch,
                       m->J, m->ll_r);
            }
        } else {
            m->ll_form[0] = SERT_LL_FORM_FUSED_ROW; m->ll_form[1] = 512;
            launch((ll_fused_row<TRAIN, 512>), dim3(B), dim3(512), fused_lds, m->stream,
                   m->ll_dedup ? m->J : m->Z, (const float*)m->Zu, slot, y, indptr, ds.csr_indices,
                   ds.csr_data, w, m->rowloss, n, V, inv_batch, m->ll_r);
        }
    } else if (rowwise) {
        // the plain row-per-workgroup kernels (kept as a cross-check of the streaming path)
        ScopedTimer t(m, TG_LOSS);
        m->ll_form[0] = SERT_LL_FORM_ROWWISE;
        launch(ll_softmax_rows, dim3(cdiv(rows, 4)), dim3(256), 0, m->stream, m->Z, rows,
               V);
        launch((ll_window<TRAIN>), dim3(B), dim3(256), 0, m->stream, m->Z, m->J, y,
               indptr, ds.csr_indices, ds.csr_data, w, m->rowloss, n, V, inv_batch);
    } else {
        ScopedTimer t(m, TG_LOSS);
        m->ll_form[0] = SERT_LL_FORM_STREAM; m->ll_form[1] = V % 4 == 0 ? 1 : 0;
        if (V % 4 == 0) SERT_TRY((ll_stream_loss<TRAIN, true>(m, ds, row0, y, indptr, w, inv_batch, slot)));
        else            SERT_TRY((ll_stream_loss<TRAIN, false>(m, ds, row0, y, indptr, w, inv_batch, slot)));
    }
    return 0;
}

static int ll_backward(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const auto& c = m->cfg;
    const int B = c.batch_size, n = c.window_size, d = c.word_dim, V = c.num_entities;
    const size_t row0 = (size_t)batch_index * B;
    int64_t rows = (int64_t)B * n;          // rows of the dZ operand of the two GEMMs
    const float* dZ = m->Z;
    bool dg_mapped = false;                 // dG went straight to the word-table gradient rows
    if (m->ll_dedup) {
        // per-word sums of dL/dZ (the backward of "duplicate tokens share a logit row")
        ScopedTimer t(m, TG_EGRAD);
        SERT_TRY(dzu_from_dj(m, ds, batch_index));   // (every distinct-word step emits dJ_i + r_ik)
        dZ = m->dZu;
        rows = m->ll_U;
    }
    {
        // dW (d, V) = G^T.dZ, reduction over the tokens (distinct words); db = column sums of dZ
        const int tiles = cdiv(V, GN) * cdiv(d, GM);
        static const int want_items = variant_knob("SERT_LL_DW_ITEMS") ? std::max(1, atoi(variant_knob("SERT_LL_DW_ITEMS"))) : 1024;   // tuning knob
        int splits = std::max(1, std::min(cdiv(rows, GK), cdiv(want_items, tiles)));
        int kper = (int)round_up(cdiv(rows, splits), GK);
        splits = cdiv(rows, kper);
        const size_t mn = (size_t)d * V;
        const size_t stride = mn + V;
        // Single GPU, a GEMM worth forking for: dW, its combine and (optimizer_and_loss) the W, b update only
        // feed the loss finalisation -- they run on the side stream beside dG -> row scatter -> word-table
        // update instead of in front of them.  SERT_LL_DW_SIDE=0 keeps the whole step on one stream.
        static const bool dw_side_off = knob("SERT_LL_DW_SIDE") && atoi(knob("SERT_LL_DW_SIDE")) == 0;
        const bool dw_side = !dw_side_off && !is_dp(m) && !m->timing.enabled && m->nstreams >= 2 && ext_events() &&
                             2.0 * (double)rows * d * V >= 2e9;
        hipStream_t sd = dw_side ? m->stream2 : m->stream;
        m->ll_dw_side = dw_side;   // (optimizer_and_loss: W and b are updated on that stream too, whatever their size)
        if (dw_side) {
            SERT_HIP(hipEventRecord(m->ev_fork, m->stream));
            SERT_HIP(hipStreamWaitEvent(sd, m->ev_fork, 0));
        }
        {
            ScopedTimer t(m, TG_GEMM_DW);
            launch_gemm<true, false, EPI_STORE, true>(sd, m->G, dZ, m->part, nullptr, d, V,
                                                      (int)rows, d, V, V, splits, kper, stride);
        }
        {
            ScopedTimer t(m, TG_SPLITK);
            launch_reduce_partials(sd, m->part,
                               splits, stride, stride, m->g_w, mn, m->g_b);
        }
        {
            // dG (rows, d) = dZ.W^T -- in distinct-word mode row u IS the gradient of word uwords[u]: where the
            // 64x64-tile kernel takes the launch its epilogue stores the rows straight into dR_w (14.8 us of
            // scatter pass less on the step's chain at C2 dims); keep_grads keeps dG readable
            ScopedTimer t(m, TG_GEMM_DX);
            static const bool no_map = variant_knob("SERT_LL_NO_ROWMAP") != nullptr;   // cross-check knob
            const int32_t* rowmap = (m->ll_dedup && !c.keep_grads && !no_map)
                                        ? ds.idx_uwords + ds.idx_batches[(size_t)batch_index].uw_off : nullptr;
            SERT_TRY((gemm_long_k<false, true>(m->skbuf, m->stream, dZ, m->W, m->DG, (int)rows, d, V, V, V, rowmap, m->g_rw, &dg_mapped)));
        }
    }
    if (!dg_mapped) {
        ScopedTimer t(m, TG_SCATTER);
        if (m->ll_dedup) {
            // dG already holds one row per distinct word: dR_w[word_u, :] = dG[u, :]
            const BatchIndex& bx = ds.idx_batches[(size_t)batch_index];
            launch(ll_scatter_rows, dim3(grid_for(rows * d)), dim3(256), 0, m->stream, m->DG,
                   ds.idx_uwords + bx.uw_off, rows, d, m->g_rw,
                   (unsigned char*)nullptr);
        } else {
            // dR_w[X[r],:] += dG[r,:]
            SERT_TRY(word_grad_segsum(m, ds, batch_index, m->DG, 1.0f));
        }
    }
    SERT_TRY(allreduce_word_grad(m));
    (void)row0;
    return 0;
}
