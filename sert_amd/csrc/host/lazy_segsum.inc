// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): the lazy word-table update's host state, the tensor table, the word-gradient tree, the loglinear per-word sums, the sorted entity-gradient chain, the gather and log-softmax launchers, long-K GEMMs.

// ---- lazy dense update of the word table (kernels_opt.h: dense_update_lazy) ----------------------------------------
static void optimizer_args(const sert_model* m, int64_t t, AdamArgs* aa, AdadeltaArgs* da);
static LazyArgs lazy_args(sert_model* m, int64_t t_prev, int update) {
    LazyArgs lz;
    lz.last_in = m->rw_stale ? m->rw_last[m->rw_last_cur] : nullptr;
    lz.last_out = m->rw_last[m->rw_last_cur ^ 1];
    lz.next_bits = nullptr;
    lz.t_prev = (int)t_prev;
    lz.write_all = 1;
    lz.update = update;
    for (int k = 0; k <= kLazyK; ++k) {
        AdamArgs aa; AdadeltaArgs da;
        optimizer_args(m, std::max<int64_t>(1, t_prev + 1 - k), &aa, &da);
        lz.a_of[k] = aa.a_t;
    }
    return lz;
}
// Bring every row of R_w (and of its optimiser state) to the model's step -- unless `batch` is the training batch
// whose rows the last update made current (the announced one: its forward may read them as they are).  Main stream.
// t_applied = number of updates a CURRENT row has seen (default: m->step).  Inside optimizer_and_loss the step counter is
// already the number of the update being applied, so the dense fallback there passes m->step - 1: flushing against the
// incremented counter gave every row one zero-gradient update too many before the dense launch applied the same update
// number again (round-4 advisor finding; tests/test_gpu_lazy_dense.py alternates lazy and dense steps).
static int ensure_rw_current(sert_model* m, int64_t batch, int64_t t_applied) {
    if (!m->rw_stale) return 0;
    if (batch >= 0 && batch == m->rw_ready_batch) return 0;
    if (t_applied < 0) t_applied = m->step;
    ++m->state_counts[2];
    AdamArgs aa; AdadeltaArgs da;
    optimizer_args(m, std::max<int64_t>(1, t_applied), &aa, &da);
    const LazyArgs lz = lazy_args(m, t_applied, /*update=*/0);
    const int64_t max_nb = m->n_rw >= ((size_t)1 << 24) ? 2 * kOptBlocks : kOptBlocks;
    const int nb = (int)std::min<int64_t>(max_nb, cdiv(cdiv(m->n_rw, 4), 256));
    if (is_vs(m))
        launch((dense_update_lazy<true>), dim3(nb), dim3(256), 0, m->stream, m->rw, (const float*)m->g_rw, m->s0_rw, m->s1_rw,
               m->n_rw, aa, da, m->sq_scratch, (const uint32_t*)nullptr, (unsigned)m->cfg.word_dim, lz);
    else
        launch((dense_update_lazy<false>), dim3(nb), dim3(256), 0, m->stream, m->rw, (const float*)m->g_rw, m->s0_rw, m->s1_rw,
               m->n_rw, aa, da, m->sq_scratch, (const uint32_t*)nullptr, (unsigned)m->cfg.word_dim, lz);
    m->rw_last_cur ^= 1;
    m->rw_stale = false;
    m->rw_ready_batch = -1;
    return 0;
}

// A deferred entity-table update (side-heavy schedule) must have landed before the main stream reads R_e,
// its optimiser state or dR_e again.
static int settle_entity_update(sert_model* m) {
    if (m->re_pending) {
        SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_re, 0));
        m->re_pending = false;
        ++m->state_counts[3];
    }
    return 0;
}

struct TensorRef {
    float* ptr;
    size_t count;
};
static TensorRef tensor_ref(sert_model* m, int which) {
    const size_t B = m->cfg.batch_size;
    switch (which) {
        case SERT_T_RW: return {m->rw, m->n_rw};
        case SERT_T_RE: return {m->re, m->n_re};
        case SERT_T_W: return {m->W, m->n_w};
        case SERT_T_B: return {m->b, m->n_b};
        case SERT_T_STATE0_RW: return {m->s0_rw, m->n_rw};
        case SERT_T_STATE0_RE: return {m->s0_re, m->n_re};
        case SERT_T_STATE0_W: return {m->s0_w, m->n_w};
        case SERT_T_STATE0_B: return {m->s0_b, m->n_b};
        case SERT_T_STATE1_RW: return {m->s1_rw, m->n_rw};
        case SERT_T_STATE1_RE: return {m->s1_re, m->n_re};
        case SERT_T_STATE1_W: return {m->s1_w, m->n_w};
        case SERT_T_STATE1_B: return {m->s1_b, m->n_b};
        case SERT_T_GRAD_RW: return {m->g_rw, m->n_rw};
        case SERT_T_GRAD_RE: return {m->g_re, m->n_re};
        case SERT_T_GRAD_W: return {m->g_w, m->n_w};
        case SERT_T_GRAD_B: return {m->g_b, m->n_b};
        case SERT_T_ACT_H: return {m->H, m->H ? B * m->cfg.word_dim : 0};
        case SERT_T_ACT_T: return {m->T, m->T ? B * m->cfg.entity_dim : 0};
        case SERT_T_ACT_DA: return {m->DA, m->DA ? B * m->cfg.entity_dim : 0};
        case SERT_T_ACT_DH: return {m->DH, m->DH ? B * m->cfg.word_dim : 0};
        case SERT_T_ACT_ROWLOSS: return {m->rowloss, B};
        default: return {nullptr, 0};
    }
}

// Dispatch on the token-id width (np.min_scalar_type, bin/prepare.py:380).
#define SERT_ID_DISPATCH(id_bytes, ...)                                  \
    do {                                                                 \
        if ((id_bytes) == 1) { typedef uint8_t IdT; __VA_ARGS__; }       \
        else if ((id_bytes) == 2) { typedef uint16_t IdT; __VA_ARGS__; } \
        else { typedef uint32_t IdT; __VA_ARGS__; }                      \
    } while (0)


// dR_w = scatter-add of `src` rows into the word table, as an order-fixed
// segmented reduction over the batch's prebuilt inverted index (word_index.h).
static int word_grad_segsum(sert_model* m, const DataSplit& ds, int64_t batch_index,
                            const float* src, float divisor) {
    const int d = m->cfg.word_dim;
    if ((size_t)batch_index >= ds.idx_batches.size()) SERT_FAIL("batch has no word index");
    const BatchIndex& bx = ds.idx_batches[(size_t)batch_index];
    // (sert_debug_wgrad_plan: what is launched below, recorded beside every launch)
    int32_t* wp = m->wg_plan;
    for (int i = 0; i < 24; ++i) wp[i] = 0;
    wp[0] = SERT_WGRAD_PATH_WORD_GRAD; wp[1] = bx.nlevels; wp[3] = bx.dense_cnt; wp[8] = bx.slot_is_row ? 1 : 0;
    auto wp_launch = [&](int form, int grid_y) { if (wp[2] < 6) { wp[10 + 2 * wp[2]] = form; wp[11 + 2 * wp[2]] = grid_y; } ++wp[2]; };
    unsigned char* touched = nullptr;   // (row flags are static per batch: DataSplit::idx_touched_bits)
    static const bool no_fused_upper = variant_knob("SERT_SEG_NO_FUSED_UPPER") != nullptr;   // cross-check knob
    const bool fused_upper = !no_fused_upper && bx.fused_upper_ok && ds.idx_heavy && d % 4 == 0 &&
                             bx.nlevels == 3 && bx.item_cnt[1] > 0;
    // the batch's heavy words: one streaming pass over src for all of them (kernels_seg.h: segsum_heavy)
    // (vectorspace only: a loglinear index marks dense words for the V_e-wide per-word sums of dzu_from_dj; its
    // word gradient -- when it comes through here at all: SERT_LL_NODEDUP / the row-wise loss path -- has one source
    // row per TOKEN, not per batch row, and hpart is sized for V_e columns, not d_w)
    // Round 5: INSIDE the tree's launches where those are the 32-lane forms (kernels_seg.h: segsum_rows_plus) -- the streaming
    // pass beside level 0, its combine beside level 1; SERT_HEAVY_NO_FUSE (variants build) keeps the two launches in front.
    bool heavy_fused = false, heavy_combined = false;
    PlusJob hjob = PlusJob();
    if (bx.dense_cnt > 0 && is_vs(m) && d % 4 == 0) {
        const int B = m->cfg.batch_size, d4 = d / 4;
        static const bool no_fuse = variant_knob("SERT_HEAVY_NO_FUSE") != nullptr;
        const bool lpi32 = d4 <= 32 || (d4 > 64 && 64 * cdiv(d4, 64) > 32 * cdiv(d4, 32));
        const bool bundled = bx.bundle_cnt > 0 && ds.idx_bundles;
        heavy_fused = !no_fuse && lpi32 && bx.nlevels >= 1 && bx.item_cnt[0] > 0 && bx.row_groups == 1 && !bundled;
        const uint4* cnt = ds.idx_dense_counts + (size_t)batch_index * B;
        if (heavy_fused) {
            hjob.kind = 1; hjob.rpb = heavy_rows_fused(B); hjob.extra = cdiv(B, hjob.rpb); hjob.src = src; hjob.cnt16 = cnt; hjob.part = m->hpart;
            hjob.words = (const int32_t*)ds.idx_dense_words + (size_t)batch_index * kHeavyMax;
            hjob.nheavy = bx.dense_cnt; hjob.nblocks = hjob.extra; hjob.B = B;
            wp[4] = SERT_WGRAD_HEAVY_FUSED; wp[5] = hjob.rpb; wp[6] = hjob.extra;
        } else {
        const int nblk = cdiv(B, kHeavyRowsPerBlock);
        wp[4] = SERT_WGRAD_HEAVY_TWO_LAUNCHES; wp[5] = kHeavyRowsPerBlock; wp[6] = nblk;
        const size_t lds = (size_t)4 * kHeavyMax * 32 * sizeof(float4);   // 32 KB
        launch(segsum_heavy, dim3(nblk * cdiv(d4, 32)), dim3(1024), lds, m->stream, src, cnt, B, d, m->hpart);
        launch(segsum_heavy_combine, dim3(bx.dense_cnt, cdiv(d4, 32)), dim3(256), 0, m->stream,
               (const float*)m->hpart, nblk, d, (const int32_t*)ds.idx_dense_words + (size_t)batch_index * kHeavyMax,
               bx.dense_cnt, m->g_rw, divisor);
        }
    }
    auto heavy_combine_job = [&]() { PlusJob j = hjob; j.kind = 2; j.extra = bx.dense_cnt; j.src = m->hpart; return j; };
    for (int l = 0; l < bx.nlevels; ++l) {
        const int nitems = bx.item_cnt[l];
        if (nitems == 0) continue;
        if (fused_upper && l == 1) {
            // levels 1 and 2 in one launch (kernels_seg.h: segsum_upper_fused)
            const int nb_normal = cdiv(nitems, 32);
            launch(segsum_upper_fused, dim3(nb_normal + bx.heavy_cnt, cdiv(d / 4, 32)), dim3(1024), 0, m->stream,
                   m->wpart + (size_t)bx.part_off[0] * d, ds.idx_items + bx.item_off[1], nitems, nb_normal,
                   ds.idx_heavy + bx.heavy_off, m->g_rw, d, divisor);
            wp_launch(SERT_WGRAD_FORM_UPPER_FUSED, cdiv(d / 4, 32));
            break;
        }
        const float* in = (l == 0) ? src : m->wpart + (size_t)bx.part_off[l - 1] * d;
        const int32_t* rows = (l == 0) ? ds.idx_rows + bx.rows_off : nullptr;
        const int4* items = ds.idx_items + bx.item_off[l];
        float* pout = m->wpart + (size_t)bx.part_off[l] * d;
        if (heavy_fused && l <= 1) {
            // level 0 + the heavy words' partial sums / level 1 + their combine: one launch each
            PlusJob j = l == 0 ? hjob : heavy_combine_job();
            j.slot_is_row = (l == 0 && bx.slot_is_row) ? 1 : 0;
            launch(segsum_rows_plus, dim3(j.extra + cdiv(nitems, 8), cdiv(d / 4, 32)), dim3(256), 0, m->stream, in, rows, items,
                   nitems, m->g_rw, pout, d, divisor, j);
            wp_launch(SERT_WGRAD_FORM_ROWS_PLUS, cdiv(d / 4, 32));
            if (l == 1) heavy_combined = true;
            continue;
        }
        // level 0 in bundles of short items (kernels_seg.h: segsum_rows_bundled; opt-in, SERT_SEG_BUNDLE=1 at upload -- the
        // same sums bit for bit as one item per lane group, tests/test_gpu_parity.py::test_word_gradient_bundled_level0)
#ifdef SERT_VARIANTS
        if (l == 0 && d % 4 == 0 && bx.bundle_cnt > 0 && ds.idx_bundles && bx.row_groups == 1) {
            launch(segsum_rows_bundled, dim3(cdiv(bx.bundle_cnt, 8), cdiv(d / 4, 32)), dim3(256), 0, m->stream, in, rows,
                   items, (const int32_t*)ds.idx_bundles + bx.bundle_off, (int)bx.bundle_cnt, m->g_rw, pout, d, divisor);
            wp_launch(SERT_WGRAD_FORM_BUNDLED, cdiv(d / 4, 32));
            continue;
        }
#endif
        if (d % 4 == 0) {
            // lane groups of 32 or 64 float4 columns, whichever wastes fewer lanes (d = 300: 75 chunks are
            // 3 x 32 at 78 % instead of 2 x 64 at 59 %: 147 -> 143 us at C4; the sums do not depend on it)
            const int ch = d / 4;
            const bool seg32y = ch > 64 && ch * (64 * cdiv(ch, 64)) > ch * (32 * cdiv(ch, 32));
            // row-grouped level 0: eight item lists, one per XCD (kernels_seg.h: XcdLists)
            XcdLists xl = XcdLists();
            xl.slot_is_row = (l == 0 && bx.slot_is_row) ? 1 : 0;
            int longest = 0;
            if (l == 0 && bx.row_groups > 1) {
                xl.on = 1;
                for (int x = 0; x < 8; ++x) { xl.off[x] = bx.xcd_off[x]; xl.cnt[x] = bx.xcd_cnt[x]; longest = std::max(longest, bx.xcd_cnt[x]); }
            }
            const int ipb = (d / 4 <= 32 || seg32y) ? 8 : 4;
            const int gx = xl.on ? 8 * cdiv(longest, ipb) : cdiv(nitems, ipb);
            if (d / 4 <= 32) {
                launch((segsum_rows<32>), dim3(gx), dim3(256), 0, m->stream,
                       in, rows, items, nitems, m->g_rw, pout, d, divisor, touched, 1, nullptr, nullptr, DenseSlots(), xl);
                wp_launch(SERT_WGRAD_FORM_ROWS32, 1);
            } else if (seg32y) {
                launch((segsum_rows<32>), dim3(gx, cdiv(d / 4, 32)), dim3(256), 0, m->stream,
                       in, rows, items, nitems, m->g_rw, pout, d, divisor, touched, 1, nullptr, nullptr, DenseSlots(), xl);
                wp_launch(SERT_WGRAD_FORM_ROWS32, cdiv(d / 4, 32));
            } else {   // rows wider than 64 float4 chunks (d = 300: 75): the rest goes to further column groups
                launch((segsum_rows<64>), dim3(gx, cdiv(d / 4, 64)), dim3(256), 0, m->stream,
                       in, rows, items, nitems, m->g_rw, pout, d, divisor, touched, 1, nullptr, nullptr, DenseSlots(), xl);
                wp_launch(SERT_WGRAD_FORM_ROWS64, cdiv(d / 4, 64));
            }
        } else {
            launch((segsum_rows_scalar<false>), dim3(cdiv(nitems, 4), cdiv(d, 64)), dim3(256), 0, m->stream, in,
                   rows, items, nitems, m->g_rw, pout, d, divisor, touched, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
            wp_launch(SERT_WGRAD_FORM_SCALAR, cdiv(d, 64));
        }
    }
    if (heavy_fused && !heavy_combined) {   // (no level 1, or the fused upper levels took it: the combine alone)
        const PlusJob j = heavy_combine_job();
        launch(segsum_rows_plus, dim3(j.extra, cdiv(d / 4, 32)), dim3(256), 0, m->stream, (const float*)nullptr,
               (const int32_t*)nullptr, (const int4*)nullptr, 0, m->g_rw, (float*)nullptr, d, divisor, j);
        wp[7] = 1;
    }
    return 0;
}

// Loglinear on the distinct-word tables (kernels_ll.h): per word, the sum of the dJ rows of the
// batch rows it occurs in and the sum of its r_ik, then dZu = mask dJsum - P rsum.  Both sums
// ride the word's occurrence tree -- the same order-fixed tree as the word gradient, over
// V_e-wide rows (source row = batch row of the occurrence), destination = the word's rank
// among the batch's distinct words.
static int dzu_from_dj(sert_model* m, const DataSplit& ds, int64_t batch_index) {
    const int V = m->cfg.num_entities;
    const BatchIndex& bx = ds.idx_batches[(size_t)batch_index];
    // (sert_debug_wgrad_plan: what is launched below for the V_e-wide sums, recorded beside every launch)
    int32_t* wp = m->wg_plan;
    for (int i = 0; i < 24; ++i) wp[i] = 0;
    wp[0] = SERT_WGRAD_PATH_DZU; wp[1] = bx.nlevels; wp[3] = bx.dense_cnt; wp[8] = bx.slot_is_row ? 1 : 0;
    auto wp_launch = [&](int form, int grid_y) { if (wp[2] < 6) { wp[10 + 2 * wp[2]] = form; wp[11 + 2 * wp[2]] = grid_y; } ++wp[2]; };
    // odd V_e: the scalar sums and the finishing expression ride the V_e-wide launches (kernels_seg.h: segsum_rows_scalar<true, true>)
    static const bool split_odd = variant_knob("SERT_LL_DZU_SPLIT") != nullptr;   // the three extra launches, for A/B
    const bool fused_odd = V % 4 != 0 && !split_odd;
    // the scalars first: the V_e-wide pass applies them when it stores a word's final row
    for (int l = 0; l < bx.nlevels && !fused_odd; ++l) {
        const int nitems = bx.item_cnt[l];
        if (nitems == 0) continue;
        const int32_t* rows = (l == 0) ? ds.idx_rows + bx.rows_off : nullptr;
        const int4* items = ds.idx_items + bx.item_off[l];
        const float* in = (l == 0) ? m->ll_r : m->ll_rpart + (size_t)bx.part_off[l - 1];
        float* pout = m->ll_rpart + (size_t)bx.part_off[l];
        launch(segsum_scalar_wave, dim3(cdiv(nitems, 4)), dim3(256), 0, m->stream, in, rows, items, nitems,
               m->ll_rsum, pout);
    }
    // the dense heavy words inside the tree's launches (round 5; SERT_HEAVY_NO_FUSE in a variants build: the two launches behind the tree)
    static const bool ll_no_fuse = variant_knob("SERT_HEAVY_NO_FUSE") != nullptr;
    const bool ll_heavy_fused = !ll_no_fuse && V % 4 == 0 && bx.dense_cnt > 0 && bx.nlevels >= 1 && bx.item_cnt[0] > 0;
    bool ll_heavy_combined = false;
    PlusJobLL ll_job = PlusJobLL();
    if (ll_heavy_fused) {
        const int B = m->cfg.batch_size;
        ll_job.j.kind = 1; ll_job.j.rpb = heavy_rows_fused(B); ll_job.j.extra = cdiv(B, ll_job.j.rpb); ll_job.j.src = m->J;
        ll_job.j.cnt16 = ds.idx_dense_counts + (size_t)batch_index * B; ll_job.j.part = m->hpart;
        ll_job.j.nheavy = bx.dense_cnt; ll_job.j.nblocks = ll_job.j.extra; ll_job.j.B = B;
        ll_job.logp = m->Zu; ll_job.rsum = m->ll_rsum;
        wp[4] = SERT_WGRAD_HEAVY_FUSED; wp[5] = ll_job.j.rpb; wp[6] = ll_job.j.extra;
    }
    for (int l = 0; l < bx.nlevels; ++l) {
        const int nitems = bx.item_cnt[l];
        if (nitems == 0) continue;
        const int32_t* rows = (l == 0) ? ds.idx_rows_div + bx.rows_off : nullptr;   // batch row of the entry
        const int4* items = ds.idx_items + bx.item_off[l];
        const float* in = (l == 0) ? m->J : m->zpart + (size_t)bx.part_off[l - 1] * V;
        float* pout = m->zpart + (size_t)bx.part_off[l] * V;
        if (V % 4 == 0 && bx.dense_cnt > 0) {
            // (the batch's heavy words are summed densely: their items are skipped)
            DenseSlots dsl;
            dsl.n = bx.dense_cnt;
            for (int h = 0; h < kHeavyMax; ++h) dsl.slot[h] = h < bx.dense_cnt ? bx.dense_slot[h] : -2;
            if (ll_heavy_fused && l <= 1) {
                // ... by extra workgroups of this very launch (kernels_seg.h: segsum_rows_plus_ll): the stream over dJ beside
                // level 0, its combine and finishing expression beside level 1
                PlusJobLL j = ll_job;
                j.dense = dsl;
                if (l == 1) { j.j.kind = 2; j.j.extra = bx.dense_cnt; j.j.src = m->hpart; ll_heavy_combined = true; }
                launch(segsum_rows_plus_ll, dim3(j.j.extra + cdiv(nitems, 4), cdiv(V / 4, 64)), dim3(256), 0, m->stream, in,
                       rows, items, nitems, m->dZu, pout, V, dsl, j);
                wp_launch(SERT_WGRAD_FORM_ROWS_PLUS_LL, cdiv(V / 4, 64));
                continue;
            }
            launch((segsum_rows<64, true, true, true>), dim3(cdiv(nitems, 4), cdiv(V / 4, 64)), dim3(256), 0,
                   m->stream, in, rows, items, nitems, m->dZu, pout, V, 1.0f,
                   (unsigned char*)nullptr, 1, (const float*)m->Zu,
                   (const float*)m->ll_rsum, dsl, XcdLists());
            wp_launch(SERT_WGRAD_FORM_ROWS64, cdiv(V / 4, 64));
        } else if (V % 4 == 0) {
            launch((segsum_rows<64, true, true>), dim3(cdiv(nitems, 4), cdiv(V / 4, 64)), dim3(256), 0,
                   m->stream, in, rows, items, nitems, m->dZu, pout, V, 1.0f,
                   (unsigned char*)nullptr, 1, (const float*)m->Zu,
                   (const float*)m->ll_rsum, DenseSlots(), XcdLists());
            wp_launch(SERT_WGRAD_FORM_ROWS64, cdiv(V / 4, 64));
        } else if (fused_odd) {
            launch((segsum_rows_scalar<true, true>), dim3(cdiv(nitems, 4), cdiv(V, 64)), dim3(256), 0, m->stream, in,
                   rows, items, nitems, m->dZu, pout, V, 1.0f, (unsigned char*)nullptr, 1, (const float*)m->Zu,
                   (const float*)((l == 0) ? m->ll_r : m->ll_rpart + (size_t)bx.part_off[l - 1]),
                   (l == 0) ? (const int32_t*)(ds.idx_rows + bx.rows_off) : (const int32_t*)nullptr,
                   m->ll_rsum, m->ll_rpart + (size_t)bx.part_off[l]);
            wp_launch(SERT_WGRAD_FORM_SCALAR_LL, cdiv(V, 64));
        } else {
            launch((segsum_rows_scalar<true>), dim3(cdiv(nitems, 4), cdiv(V, 64)), dim3(256), 0, m->stream, in,
                   rows, items, nitems, m->dZu, pout, V, 1.0f, (unsigned char*)nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
            wp_launch(SERT_WGRAD_FORM_SCALAR, cdiv(V, 64));
        }
    }
    if (ll_heavy_fused && !ll_heavy_combined) {   // (no level 1: the combine alone)
        PlusJobLL j = ll_job;
        j.dense.n = bx.dense_cnt;
        for (int h = 0; h < kHeavyMax; ++h) j.dense.slot[h] = h < bx.dense_cnt ? bx.dense_slot[h] : -2;
        j.j.kind = 2; j.j.extra = bx.dense_cnt; j.j.src = m->hpart;
        launch(segsum_rows_plus_ll, dim3(j.j.extra, cdiv(V / 4, 64)), dim3(256), 0, m->stream, (const float*)nullptr,
               (const int32_t*)nullptr, (const int4*)nullptr, 0, m->dZu, (float*)nullptr, V, j.dense, j);
        wp[7] = 1;
    }
    if (V % 4 == 0 && bx.dense_cnt > 0 && !ll_heavy_fused) {
        // Heavy words: sum_i cnt[i][h] dJ[i, :] by ONE pass over dJ (262 MB at C2 dims) instead of one 4 kB
        // row fetch per occurrence -- a dozen words hold over half of a Zipfian batch's tokens
        const int B = m->cfg.batch_size, d4 = V / 4;
        const int nblk = cdiv(B, kHeavyRowsPerBlock);
        wp[4] = SERT_WGRAD_HEAVY_WIDE; wp[5] = kHeavyRowsPerBlock; wp[6] = nblk;
        const uint4* cnt = ds.idx_dense_counts + (size_t)batch_index * B;
        static const bool attr_set = hipFuncSetAttribute((const void*)segsum_heavy_wide, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         2 * kHeavyMax * 128 * (int)sizeof(float4)) == hipSuccess;
        if (!attr_set) SERT_FAIL("cannot reserve the LDS of segsum_heavy_wide");
        launch(segsum_heavy_wide, dim3(nblk * cdiv(d4, 128)), dim3(512), (size_t)2 * kHeavyMax * 128 * sizeof(float4), m->stream,
               (const float*)m->J, cnt, B, V, m->hpart);
        DenseSlots dsl;
        dsl.n = bx.dense_cnt;
        for (int h = 0; h < kHeavyMax; ++h) dsl.slot[h] = h < bx.dense_cnt ? bx.dense_slot[h] : -2;
        launch(segsum_heavy_combine_ll, dim3(bx.dense_cnt, cdiv(d4, 32)), dim3(256), 0, m->stream,
               (const float*)m->hpart, nblk, V, dsl, m->dZu, (const float*)m->Zu, (const float*)m->ll_rsum);
    }
    if (V % 4 != 0 && !fused_odd)   // (odd V_e, split form: separate finishing pass)
        launch(ll_dzu_combine, dim3(grid_for((int64_t)m->ll_U * V)), dim3(256), 0, m->stream, m->dZu,
               (const float*)m->Zu, (const float*)m->ll_rsum, (int64_t)m->ll_U, V);
    return 0;
}

// ---- the sorted entity-gradient chain: stable key sort -> chunked reduce -> carry fix-up (kernels_sort.h, kernels_egrad.h) ----
// One chain for the vectorspace step (vs_entity_grad, vs_early_sort: V_e rows) and the fold-in step (foldin_grad,
// api_foldin.inc: N trainable rows behind a sentinel run).  EntityChain is a VIEW of the owner's buffers: pointers and sizes,
// nothing is allocated or freed through it.  Each function returns what it launched; the owner records that in its own plan.
struct EntityChain {
    int32_t *keys_sorted, *pairs_sorted;      // (total) the sort's output: keys, and the pair index of each
    int32_t *k_tmp, *v_tmp;                   // (total) ping-pong, only if sort_bits > kSortMaxBits
    int32_t *sort_hist, *sort_bin_total;      // counting-sort scratch
    int32_t *run_start, *run_end;             // per-row bounds of the sorted runs; run_end follows run_start in one array ...
    int nbounds;                              // ... of nbounds ints, cleared by the sort's first pass
    float *ehead, *etail;                     // (chunks, d_e) carries
    int sort_bits, rows, de, zp1, total;      // rows of the gradient table (V_e / N); zp1 = z + 1; total = B (z + 1) keys
};
struct ChainSorted { int bits, passes; };
struct ChainReduced { int vec, nch; };

// Stable sort of the (key, pair index) entries: keys -> keys_sorted, iota -> pairs_sorted, LSD over ceil(bits/11) digits.
static ChainSorted entity_key_sort(const EntityChain& c, const int32_t* keys, hipStream_t st) {
    const int bits = c.sort_bits;
    const int passes = cdiv(bits, kSortMaxBits);
    const int width = cdiv(bits, passes);
    const int32_t* kin = keys;
    const int32_t* vin = nullptr;  // value of element i is i
    for (int p = 0; p < passes; ++p) {
        const int shift = p * width;
        const int nb = std::min(width, bits - shift);
        const bool to_final = ((passes - 1 - p) % 2) == 0;
        int32_t* kout = to_final ? c.keys_sorted : c.k_tmp;
        int32_t* vout = to_final ? c.pairs_sorted : c.v_tmp;
        // (first digit: also clears run_start / run_end, which the chunked reduce only writes for the rows it meets --
        //  a step whose negatives were drawn ahead has no prologue launch to clear them)
        csort_pass(st, kin, vin, kout, vout, c.total, shift, nb, c.sort_hist, c.sort_bin_total,
                   p == 0 ? c.run_start : (int32_t*)nullptr, p == 0 ? c.nbounds : 0);
        kin = kout;
        vin = vout;
    }
    return {bits, passes};
}

// The chunked reduce of the sorted pairs into G (rows, d_e) and the carries.  sentinel >= 0: the last run of the order, keys
// == sentinel, is pairs that are not reduced (foldin_chunk_reduce); the model has none.
static ChainReduced entity_chunk_reduce(const EntityChain& c, const float* coef, const float* T, float* G, hipStream_t st,
                                        int sentinel = -1) {
    const dim3 grid(cdiv(cdiv(c.total, kEChunk), 16)), blk(256);
    auto go = [&](auto vec, auto nch) {
        constexpr int VEC = decltype(vec)::value, NCH = decltype(nch)::value;
        if (sentinel < 0)
            launch((egrad_chunk_reduce<VEC, NCH>), grid, blk, 0, st, c.keys_sorted, c.pairs_sorted, coef, T, c.total, c.zp1, c.de,
                   G, c.ehead, c.etail, c.run_start, c.run_end);
        else
            launch((foldin_chunk_reduce<VEC, NCH>), grid, blk, 0, st, c.keys_sorted, c.pairs_sorted, coef, T, c.total, c.zp1, c.de,
                   sentinel, G, c.ehead, c.etail, c.run_start, c.run_end);
        return ChainReduced{VEC, NCH};
    };
    using std::integral_constant;
    if (c.de % 4 != 0) return go(integral_constant<int, 1>(), integral_constant<int, 4>());
    const int nch = cdiv(c.de / 4, 16);
    const integral_constant<int, 4> v4;
    return nch <= 1 ? go(v4, integral_constant<int, 1>()) : nch <= 2 ? go(v4, integral_constant<int, 2>())
         : nch <= 5 ? go(v4, integral_constant<int, 5>()) : go(v4, integral_constant<int, 8>());
}

// The fix-up over the table's rows: rows no pair hit get a zero gradient row, runs that cross chunks their carries in chunk
// order.  Few rows: one workgroup per row (long runs).  -> SERT_EGRAD_FIXUP_WORKGROUP / SERT_EGRAD_FIXUP_WAVE
static int entity_fixup(const EntityChain& c, float* G, hipStream_t st) {
    const bool few = c.rows < 256 && c.de <= 512;
    auto go = [&](auto vec) {
        constexpr int VEC = decltype(vec)::value;
        if (few)
            launch((egrad_fixup_wg<VEC>), dim3(c.rows), dim3(256), 0, st, c.run_start, c.run_end, c.rows, c.de, c.ehead, c.etail, G);
        else
            launch((egrad_fixup<VEC>), dim3(cdiv(c.rows, 4)), dim3(256), 0, st, c.run_start, c.run_end, c.rows, c.de, c.ehead,
                   c.etail, G);
    };
    if (c.de % 4 == 0) go(std::integral_constant<int, 4>());
    else go(std::integral_constant<int, 1>());
    return few ? SERT_EGRAD_FIXUP_WORKGROUP : SERT_EGRAD_FIXUP_WAVE;
}

// the model's chain (api_model.inc owns the buffers)
static EntityChain vs_entity_chain(const sert_model* m) {
    const auto& c = m->cfg;
    return {m->cand_sorted, m->pair_sorted, m->sort_k_tmp, m->sort_v_tmp, m->sort_hist, m->sort_bin_total, m->run_start, m->run_end,
            (int)(2 * round_up(c.num_entities, 4)), m->ehead, m->etail, m->sort_bits, c.num_entities, c.entity_dim,
            c.num_negatives + 1, c.batch_size * (c.num_negatives + 1)};
}

// ---- launchers that the training steps, the rankers and the fold-ins share ----------------------------------------------
// out (rows, d) = table[ids]: 16-byte pieces when d allows them
template <typename IdT>
static void gather_rows(hipStream_t s, const IdT* ids, const float* table, float* out, int64_t rows, int d) {
    if (d % 4 == 0) launch((ll_gather_rows<IdT, 4>), dim3(grid_for(rows * d / 4, 256, 1 << 20)), dim3(256), 0, s, ids, table, out, rows, d);
    else            launch((ll_gather_rows<IdT, 1>), dim3(grid_for(rows * d, 256, 1 << 20)), dim3(256), 0, s, ids, table, out, rows, d);
}
// out (rows, d) = the mean of the n rows table[ids[r, :]]
template <typename IdT>
static void gather_mean(hipStream_t s, const IdT* ids, const float* table, float* out, int rows, int n, int d) {
    if (d % 4 == 0)
        launch((vs_gather_mean<IdT, 4>), dim3(grid_for((int64_t)rows * d / 4, 256, 1 << 20)), dim3(256), 0, s, ids, table, out, rows, n, d);
    else
        launch((vs_gather_mean<IdT, 1>), dim3(grid_for((int64_t)rows * d, 256, 1 << 20)), dim3(256), 0, s, ids, table, out, rows, n, d);
}
// rows of Z (rows, V) -> log softmax, in place; a wave per row, the row in registers up to V = 2048
static void logsoftmax_rows(hipStream_t s, float* Z, int64_t rows, int V) {
    if (V <= 64 * 16)      launch((ll_logsoftmax_rows<16>), dim3(cdiv(rows, 4)), dim3(256), 0, s, Z, rows, V);
    else if (V <= 64 * 32) launch((ll_logsoftmax_rows<32>), dim3(cdiv(rows, 4)), dim3(256), 0, s, Z, rows, V);
    else                   launch((ll_logsoftmax_rows<0>), dim3(cdiv(rows, 4)), dim3(256), 0, s, Z, rows, V);
}

// the kernel a launch_gemm call goes to (gemm.h: GemmRoute), asked of the launcher's own predicates; splits, kper as launch_gemm
// normalises them: one k range = (1, K)
static int gemm_route(bool ta, bool tb, int epi, bool csb, bool rowmap, const float* A, const float* Bm, int M, int N, int K,
                      int lda, int ldb, int splits, int kper) {
    if (gemm_takes_x3(ta, tb, epi, csb, rowmap, A, Bm, M, N, K, lda, ldb, splits, kper))
        return ta ? x3_ta_route(M, N) : x3_route(tb, A, Bm, M, N, K, lda, ldb, splits);
    return gemm_f32_route(ta, tb, epi, csb, A, Bm, M, N, K, lda, ldb, splits, kper);
}

// C (M,N, contiguous) = op(A).op(B) for a contraction over a LONG K (the entity
// vocabulary in the dX GEMMs of the full-softmax models) whose output has too few
// 128x128 tiles to fill 256 CUs: split K so that ~1024 workgroup items exist, then an
// order-fixed combine (deterministic).  skbuf: the caller's buffer for the k ranges, grown here; route, k_ranges
// (optional): the GemmRoute of the GEMM launch and the number of k ranges it was cut into.
template <bool TA, bool TB>
static int gemm_long_k(DevBuf<float>& skbuf, hipStream_t s, const float* A, const float* Bm, float* C, int M,
                       int N, int K, int lda, int ldb, const int32_t* rowmap = nullptr, float* mapped_C = nullptr,
                       bool* mapped = nullptr, int* route = nullptr, int* k_ranges = nullptr) {
    if (mapped) *mapped = false;
    const int tiles = cdiv(M, GM) * cdiv(N, GN);
    int splits = 1;
    if (tiles < 512 && K >= 4096) splits = std::min(cdiv(1024, tiles), K / 1024);
    else if (tiles < 256 && K >= 512) splits = std::min(cdiv(1024, tiles), K / 128);   // few tiles, medium K
    if (!TA && K >= 4096 && gemm_x3_enabled()) {
        // the bf16-pipe kernel (gemm_x3.h) has larger tiles -- 256 rows, up to 320 columns --: enough k ranges for two
        // workgroups per CU (the loglinear dG over 100 000 entities: 9 tiles x 57 ranges; 1.83 -> 1.1 ms)
        const int t3 = cdiv(M, N <= 128 ? 128 : 256) * cdiv(N, N <= 128 ? 128 : 320);
        const int s3 = std::max(1, std::min(cdiv(512, t3), K / 1024));
        if (s3 > 1 && x3_shape_ok(false, TB, A, Bm, M, N, K, lda, ldb, s3)) splits = s3;
    }
    // (between one and two tiles per CU -- the loglinear dG at C2 dims, 347 tiles -- a three-way split was
    //  tried: 162 -> 175 us with its combine; co-resident workgroups share the matrix pipe without loss)
    if (splits <= 1) {
        if (route) *route = gemm_route(TA, TB, EPI_STORE, false, rowmap != nullptr, A, Bm, M, N, K, lda, ldb, 1, K);
        if (k_ranges) *k_ranges = 1;
        launch_gemm<TA, TB, EPI_STORE>(s, A, Bm, C, nullptr, M, N, K, lda, ldb, N, 1, 0, 0, nullptr, nullptr, 0, rowmap, mapped_C,
                                       mapped);
        return 0;
    }
    const int kper = (int)round_up(cdiv(K, splits), GK);
    splits = cdiv(K, kper);
    const size_t mn = (size_t)M * N;
    if ((int64_t)(mn * splits) > skbuf.cap) {
        SERT_HIP(hipStreamSynchronize(s));      // (DevBuf::reserve frees the old buffer without synchronising)
        SERT_TRY(skbuf.reserve((int64_t)(mn * splits)));
    }
    if (route) *route = gemm_route(TA, TB, EPI_STORE, false, false, A, Bm, M, N, K, lda, ldb, splits, kper);
    if (k_ranges) *k_ranges = splits;
    launch_gemm<TA, TB, EPI_STORE>(s, A, Bm, skbuf.p, nullptr, M, N, K, lda, ldb, N, splits, kper, mn);
    if (rowmap && mapped_C) {
        // (the combine stores row r as row rowmap[r] of mapped_C: no copy kernel behind it)
        launch_reduce_partials(s, skbuf.p, splits, mn, mn, mapped_C, mn, mapped_C, rowmap, N);
        if (mapped) *mapped = true;
    } else launch_reduce_partials(s, skbuf.p, splits, mn, mn, C, mn, C);
    return 0;
}
