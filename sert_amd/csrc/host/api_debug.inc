// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): C ABI: test hooks, roctx ranges, synchronise, timing, micro-benchmarks (include/sert_hip_debug.h).

int sert_debug_poison_scratch(sert_model* m) {
    if (!m) SERT_FAIL("null argument");
    if (m->spec_fb_batch >= 0) SERT_FAIL("a run-ahead step is in flight (sert_hint_next_batch): its gradients live in the scratch");
    SERT_HIP(hipSetDevice(m->cfg.device));
    SERT_HIP(hipDeviceSynchronize());
    if (!m->gflat) return 0;
    // gradients, loss / sum-of-squares slots: quiet NaNs; the per-entity sorted-run bounds behind them: the in-range but wrong
    // run [0, 1) (a fix-up that trusted a stale bound would add chunk 0's carry to an entity the reduce never met)
    std::vector<uint32_t> h(m->gflat_alloc, 0x7fc00000u);
    if (m->run_start) {
        const size_t V4 = round_up((size_t)m->cfg.num_entities, 4);
        for (size_t i = 0; i < V4; ++i) { h[m->gflat_count + i] = 0u; h[m->gflat_count + V4 + i] = 1u; }
    }
    SERT_HIP(hipMemcpy(m->gflat, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
}

int sert_debug_update_counts(sert_model* m, int64_t* out, int n) {
    if (!m || !out || n < 1 || n > 10) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = m->upd_counts[i];
    return 0;
}

int sert_debug_tail_counts(sert_model* m, int64_t* out, int n) {
    if (!m || !out || n < 1 || n > 2) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = m->tail_counts[i];
    return 0;
}

int sert_debug_state_counts(sert_model* m, int64_t* out, int n) {
    if (!m || !out || n < 1 || n > 7) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = m->state_counts[i];
    return 0;
}

int sert_debug_ll_loss_form(sert_model* m, int32_t* out, int n) {
    if (!m || !out || n < 1 || n > 5) SERT_FAIL("bad argument");
    if (is_vs(m)) SERT_FAIL("not a loglinear model");
    for (int i = 0; i < n; ++i) out[i] = m->ll_form[i];
    return 0;
}

int sert_debug_egrad_plan(sert_model* m, int32_t* out, int n) {
    if (!m || !out || n < 1 || n > 12) SERT_FAIL("bad argument");
    if (!is_vs(m)) SERT_FAIL("not a vectorspace model");
    for (int i = 0; i < n; ++i) out[i] = m->eg_plan[i];
    return 0;
}

int sert_debug_nce_form(sert_model* m, int32_t* out, int n) {
    if (!m || !out || n < 1 || n > 6) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = m->nce_form[i];
    return 0;
}

int sert_debug_wgrad_plan(sert_model* m, int32_t* out, int n) {
    if (!m || !out || n < 1 || n > 24) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = m->wg_plan[i];
    return 0;
}

int sert_debug_vs_plan(sert_model* m, int32_t* out, int n) {
    if (!m || !out || n < 1 || n > SERT_VS_PLAN_COUNT) SERT_FAIL("bad argument");
    memcpy(out, &m->plan, (size_t)n * sizeof(int32_t));
    return 0;
}

int sert_debug_vs_facts(sert_model* m, int32_t* out, int n) {
    if (!m || !out || n < 1 || n > SERT_VS_FACT_COUNT) SERT_FAIL("bad argument");
    memcpy(out, &m->plan_facts, (size_t)n * sizeof(int32_t));
    return 0;
}

int sert_debug_vs_plan_for(const int32_t* facts, int nfacts, int32_t* out, int n) {
    if (!facts || !out || nfacts < 1 || nfacts > SERT_VS_FACT_COUNT || n < 1 || n > SERT_VS_PLAN_COUNT) SERT_FAIL("bad argument");
    VsStepFacts f;
    memcpy(&f, facts, (size_t)nfacts * sizeof(int32_t));
    const VsStepPlan p = vs_plan_step(f);
    memcpy(out, &p, (size_t)n * sizeof(int32_t));
    return 0;
}

int sert_debug_scorer_counts(sert_scorer* sc, int64_t* out, int n) {
    if (!sc || !out || n < 1 || n > 6) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = i < 5 ? sc->path_counts[i] : (sc->bf16_demoted ? 1 : 0);
    return 0;
}

int sert_debug_scorer_select(int device, int mode, const float* S, int64_t Q, int32_t V, int32_t k, float thr,
                             int32_t* idx_out, float* score_out) {
    if (!S || !idx_out || !score_out || Q <= 0 || V <= 0 || k <= 0 || k > V || k > kTopKMax || mode < 0 || mode > 1)
        SERT_FAIL("bad argument");
    SERT_HIP(hipSetDevice(device));
    const int ngroups = (int)cdiv(V, 64), gcap = 16, ccap = 1024;
    float* dS = nullptr; float* dval = nullptr; int32_t* didx = nullptr;
    unsigned long long* dcand = nullptr; unsigned char* dcnt = nullptr; int* dflag = nullptr;
    auto body = [&]() -> int {
        SERT_TRY(dmalloc(&dval, (size_t)Q * k));
        SERT_TRY(dmalloc(&didx, (size_t)Q * k));
        SERT_HIP(hipMemset(didx, 0xff, (size_t)Q * k * sizeof(int32_t)));       // a flagged row stays -1
        SERT_HIP(hipMemset(dval, 0, (size_t)Q * k * sizeof(float)));
        if (mode == 0) {
            SERT_TRY(dmalloc(&dS, (size_t)Q * V));
            SERT_HIP(hipMemcpy(dS, S, (size_t)Q * V * sizeof(float), hipMemcpyHostToDevice));
            launch(topk_rows<false>, dim3((unsigned)Q), dim3(256), 0, 0, dS, (int)V, (int)k, didx, dval, (float*)nullptr);
        } else {
            // the lists as the fp32 filter epilogue leaves them: per (row, 64-entity group) the elements with S >= thr in
            // ascending entity order, keyed by plain desc_key (a NaN fails the compare there as here)
            std::vector<unsigned long long> cand((size_t)Q * ngroups * gcap, 0ull);
            std::vector<unsigned char> cnt((size_t)Q * ngroups, 0);
            for (int64_t q = 0; q < Q; ++q)
                for (int32_t e = 0; e < V; ++e) {
                    const float v = S[q * V + e];
                    if (!(v >= thr)) continue;
                    uint32_t u; memcpy(&u, &v, 4);
                    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                    const size_t g = (size_t)q * ngroups + e / 64;
                    if (cnt[g] < gcap) cand[g * gcap + cnt[g]] = ((unsigned long long)(~u) << 32) | (uint32_t)e;
                    if (cnt[g] < 255) ++cnt[g];
                }
            SERT_TRY(dmalloc(&dcand, cand.size()));
            SERT_TRY(dmalloc(&dcnt, cnt.size()));
            SERT_TRY(dmalloc(&dflag, (size_t)Q + 1));
            SERT_HIP(hipMemcpy(dcand, cand.data(), cand.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
            SERT_HIP(hipMemcpy(dcnt, cnt.data(), cnt.size(), hipMemcpyHostToDevice));
            SERT_HIP(hipMemset(dflag, 0, ((size_t)Q + 1) * sizeof(int)));
            launch(topk_from_groups, dim3((unsigned)Q), dim3(256), (size_t)ccap * sizeof(unsigned long long), 0,
                   dcand, dcnt, ngroups, gcap, (int)k, didx, dval, 0, dflag, dflag + 1, ccap, (int*)nullptr);
        }
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipDeviceSynchronize());
        SERT_HIP(hipMemcpy(idx_out, didx, (size_t)Q * k * sizeof(int32_t), hipMemcpyDeviceToHost));
        SERT_HIP(hipMemcpy(score_out, dval, (size_t)Q * k * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = body();
    (void)hipFree(dS); (void)hipFree(dval); (void)hipFree(didx); (void)hipFree(dcand); (void)hipFree(dcnt); (void)hipFree(dflag);
    return rc;
}

int sert_debug_scorer_rank_counts(sert_scorer* sc, int64_t* out, int n) {
    if (!sc || !out || n < 1 || n > 6) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = sc->rank_counts[i];
    return 0;
}

int sert_debug_scorer_rerank_counts(sert_scorer* sc, int64_t out[6]) {
    if (!sc || !out) SERT_FAIL("bad argument");
    for (int i = 0; i < 6; ++i) out[i] = sc->rerank_counts[i];
    return 0;
}

int sert_debug_scorer_rank_select(int device, const float* S, int64_t Q, int32_t V, int32_t k, int32_t* idx_out, float* score_out) {
    if (!S || !idx_out || !score_out || Q <= 0 || V <= 0 || k == 0 || k < -1) SERT_FAIL("bad argument");
    const int kk = (k < 0 || k >= V) ? V : k;
    const int mode = V <= kRankLdsMax ? RANK_LDS : RANK_CSORT;
    const int64_t n = Q * (int64_t)V;
    if (mode == RANK_CSORT && !rank_chunk_fits(Q, V)) SERT_FAIL("too many queries x entities for one sorted chunk");
    SERT_HIP(hipSetDevice(device));
    float* dS = nullptr; float* dval = nullptr; int32_t* didx = nullptr;
    RankSortScratch r;
    auto body = [&]() -> int {
        SERT_TRY(dmalloc(&dS, (size_t)n));
        SERT_TRY(dmalloc(&dval, (size_t)Q * kk));
        SERT_TRY(dmalloc(&didx, (size_t)Q * kk));
        if (mode == RANK_CSORT) SERT_TRY(rank_scratch_reserve(r, n));
        SERT_HIP(hipMemcpy(dS, S, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        SERT_TRY(rank_rows_full(0, mode, /*raw=*/false, dS, (int)Q, (int)V, kk, r, didx, dval));
        SERT_HIP(hipDeviceSynchronize());
        SERT_HIP(hipMemcpy(idx_out, didx, (size_t)Q * kk * sizeof(int32_t), hipMemcpyDeviceToHost));
        SERT_HIP(hipMemcpy(score_out, dval, (size_t)Q * kk * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = body();
    (void)hipFree(dS); (void)hipFree(dval); (void)hipFree(didx); rank_scratch_free(r);
    return rc;
}

int sert_debug_row_lists(const uint32_t* allbits, int world, int rank, int64_t num_batches, int64_t bit_words,
                         int64_t rows_per_rank, int64_t vocab, int64_t batch, int32_t* serve_cnt, int32_t* fetch_cnt,
                         int32_t* serve_rows, int32_t* fetch_rows, int32_t* union_rows, int32_t* ptr, int32_t* ent,
                         int64_t capacity, int64_t* sizes) {
    if (!allbits || world < 1 || rank < 0 || rank >= world || batch < 0 || batch >= num_batches || !sizes)
        SERT_FAIL("bad argument");
    RowExchangeLists L;
    build_row_exchange(allbits, world, rank, num_batches, bit_words, rows_per_rank, vocab, L);
    const RowExchangeBatch& xb = L.batches[(size_t)batch];
    sizes[0] = xb.serve_total; sizes[1] = xb.fetch_total; sizes[2] = xb.nunion; sizes[3] = xb.nent; sizes[4] = L.max_xfer_rows;
    if (std::max<int64_t>(std::max(xb.serve_total, xb.fetch_total), std::max(xb.nunion + 1, xb.nent)) > capacity)
        SERT_FAIL("capacity too small");
    for (int q = 0; q < world; ++q) { serve_cnt[q] = xb.serve_cnt[(size_t)q]; fetch_cnt[q] = xb.fetch_cnt[(size_t)q]; }
    std::copy_n(L.serve_rows.begin() + xb.serve_off, xb.serve_total, serve_rows);
    std::copy_n(L.fetch_rows.begin() + xb.fetch_off, xb.fetch_total, fetch_rows);
    std::copy_n(L.union_rows.begin() + xb.union_off, xb.nunion, union_rows);
    std::copy_n(L.ptr.begin() + xb.ptr_off, xb.nunion + 1, ptr);
    std::copy_n(L.ent.begin() + xb.ent_off, xb.nent, ent);
    return 0;
}

// Host only (no GPU): the per-batch inverted index of sert_upload_dataset (word_index.h) built for `ids` and EVALUATED
// on the host exactly as the kernels of kernels_seg.h walk it -- every item sums its entries left to right, final items
// store acc / divisor into the gradient table, chunk items into their partial row, the upper levels read the partial
// rows of the level below -- so the structure (levels, chunk bounds, partial-row numbering, the row-grouped level 0 with
// its eight XCD lists, the dense heavy words left out of the tree) is checked by the CPU suite.
int sert_debug_word_index_sum(const void* ids, int id_bytes, int64_t num_batches, int B, int n, int vocab, int row_groups,
                              int dense_heavy, int64_t batch, const float* src, int d, float divisor, float* grad_out,
                              int64_t* stats) {
    if (!ids || !src || !grad_out || !stats || num_batches <= 0 || B <= 0 || n <= 0 || vocab <= 0 || d <= 0 || batch < 0 ||
        batch >= num_batches || (id_bytes != 1 && id_bytes != 2 && id_bytes != 4))
        SERT_FAIL("bad argument");
    WordIndex wi;
    bool ok = true;
    SERT_ID_DISPATCH(id_bytes, ok = build_word_index<IdT>((const IdT*)ids, num_batches, B, n, vocab, /*row_is_pos=*/false, wi,
                                                          /*want_slots=*/false, (dense_heavy & 1) != 0, row_groups,
                                                          /*sort_level0=*/(dense_heavy & 2) != 0));
    if (!ok) SERT_FAIL("token id >= vocab");
    const BatchIndex& bx = wi.batches[(size_t)batch];
    // (dense_heavy & 2: level 0 sorted by item length, first row number in the descriptor -- what sert_upload_dataset builds
    //  for the vectorspace models; a row-grouped index is never sorted)
    if (((dense_heavy & 2) != 0 && row_groups <= 1 && bx.nlevels >= 1 && bx.item_cnt[0] > 0) != bx.slot_is_row) SERT_FAIL("slot_is_row not as asked");
    if (bx.slot_is_row) {
        const SegItem* l0 = wi.items.data() + bx.item_off[0];
        const int32_t* r0 = wi.rows.data() + bx.rows_off;
        for (int32_t k = 0; k < bx.item_cnt[0]; ++k) {
            if (l0[k].slot != r0[l0[k].begin]) SERT_FAIL("a level-0 item's slot is not its first row");
            if (k > 0 && l0[k].end - l0[k].begin > l0[k - 1].end - l0[k - 1].begin) SERT_FAIL("level 0 is not sorted by length");
        }
    }
    std::fill(grad_out, grad_out + (size_t)vocab * d, 0.f);
    std::vector<float> part((size_t)std::max<int64_t>(1, bx.part_rows) * d, 0.f);
    int64_t items_total = 0, finals = 0;
    for (int l = 0; l < bx.nlevels; ++l) {
        const SegItem* items = wi.items.data() + bx.item_off[l];
        const float* in = l == 0 ? src : part.data() + (size_t)bx.part_off[l - 1] * d;
        const int32_t* rows = l == 0 ? wi.rows.data() + bx.rows_off : nullptr;
        float* pout = part.data() + (size_t)bx.part_off[l] * d;
        // level 0 of a row-grouped index is addressed through its XCD lists, as the kernel does
        std::vector<int32_t> order;
        if (l == 0 && bx.row_groups > 1) {
            for (int x = 0; x < 8; ++x)
                for (int k = 0; k < bx.xcd_cnt[x]; ++k) order.push_back(bx.xcd_off[x] + k);
            if ((int32_t)order.size() != bx.item_cnt[0]) SERT_FAIL("XCD lists do not cover level 0");
        } else {
            for (int32_t k = 0; k < bx.item_cnt[l]; ++k) order.push_back(k);
        }
        for (int32_t k : order) {
            const SegItem& it = items[k];
            if (it.end - it.begin > kSegChunk && l < kSegMaxLevels - 1) SERT_FAIL("an item longer than a chunk");
            ++items_total;
            float* dst = it.dst >= 0 ? grad_out + (size_t)it.dst * d : pout + (size_t)(-(it.dst + 1)) * d;
            if (it.dst >= 0) ++finals;
            for (int c = 0; c < d; ++c) {
                float a = 0.f;
                if (l == 0 && bx.slot_is_row && it.end - it.begin == 1) a += in[(size_t)it.slot * d + c];   // (as segsum_rows does)
                else
                for (int32_t e = it.begin; e < it.end; ++e) a += in[(size_t)(rows ? rows[e] : e) * d + c];
                dst[c] = it.dst >= 0 ? a / divisor : a;
            }
        }
    }
    // the dense heavy words: count-weighted sums over all batch rows (segsum_heavy + combine; the block structure of the
    // device reduction is not restated here -- integer-valued test data makes every association exact)
    for (int h = 0; h < bx.dense_cnt; ++h) {
        const uint8_t* dc = wi.dense_counts.data() + (size_t)(batch * B) * kHeavyMax;
        for (int c = 0; c < d; ++c) {
            float a = 0.f;
            for (int i = 0; i < B; ++i) a += (float)dc[(size_t)i * kHeavyMax + h] * src[(size_t)i * d + c];
            grad_out[(size_t)bx.dense_word[h] * d + c] = a / divisor;
        }
    }
    stats[0] = bx.nlevels; stats[1] = items_total; stats[2] = bx.part_rows; stats[3] = finals; stats[4] = bx.dense_cnt;
    stats[5] = bx.row_groups; stats[6] = bx.item_cnt[0]; stats[7] = bx.num_distinct;
    stats[8] = bx.fused_upper_ok ? 1 : 0; stats[9] = bx.heavy_cnt; stats[10] = bx.nlevels > 1 ? bx.item_cnt[1] : 0;
    return 0;
}

int sert_profile_range_push(const char* name) {
    roctx_load();
    if (!name) SERT_FAIL("null range name");
    return g_roctx.push ? (g_roctx.push(name) < 0 ? 1 : 0) : 0;
}
int sert_profile_range_pop(void) {
    roctx_load();
    return g_roctx.pop ? (g_roctx.pop() < 0 ? 1 : 0) : 0;
}

int sert_synchronize(sert_model* m) {
    if (!m) SERT_FAIL("null model");
    SERT_HIP(hipSetDevice(m->cfg.device));
    SERT_HIP(hipStreamSynchronize(m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream2));
    if (m->stream3) SERT_HIP(hipStreamSynchronize(m->stream3));
    if (m->comm_stream) SERT_HIP(hipStreamSynchronize(m->comm_stream));
    return 0;
}

int sert_timing_enable(sert_model* m, int on) {
    if (!m) SERT_FAIL("null model");
    if (on < 0 || on > 2) SERT_FAIL("timing mode: 0 = off, 1 = every group alone on one queue, 2 = in the step");
    SERT_HIP(hipSetDevice(m->cfg.device));
    if (m->instep.on && on != 2) {        // leaving the in-step mode: everything in flight is measured first
        SERT_HIP(hipDeviceSynchronize());
        instep_harvest(m, true);
    }
    if (on == 2 && !m->instep.created) {
        for (int i = 0; i < InStep::kRing; ++i)
            for (int k = 0; k < 2; ++k) SERT_HIP(hipEventCreate(&m->instep.ev[i][k]));
        m->instep.created = true;
    }
    m->timing.enabled = on == 1;
    m->instep.on = on == 2;
    m->instep.cur_group = -1;
    return 0;
}
int sert_timing_reset(sert_model* m) {
    if (!m) SERT_FAIL("null model");
    for (int g = 0; g < TG_COUNT; ++g) { m->timing.total_us[g] = 0; m->timing.samples[g] = 0; m->timing.used[g] = false; }
    if (m->instep.created) {
        SERT_HIP(hipSetDevice(m->cfg.device));
        SERT_HIP(hipDeviceSynchronize());
        instep_harvest(m, true);
        for (int g = 0; g < TG_COUNT; ++g) { m->instep.total_us[g] = 0; m->instep.launches[g] = 0; }
        m->instep.steps = 0;
    }
    return 0;
}
int sert_timing_count(sert_model*) { return TG_COUNT; }
const char* sert_timing_name(sert_model*, int i) { return (i >= 0 && i < TG_COUNT) ? kTimingNames[i] : ""; }
double sert_timing_avg_us(sert_model* m, int i) {
    if (!m || i < 0 || i >= TG_COUNT) return 0.0;
    if (m->instep.steps > 0) {
        // in-step mode: the group's kernel time per training step (sum of its timed launches' own durations)
        if (m->instep.head < m->instep.tail) {
            (void)hipSetDevice(m->cfg.device);
            (void)hipDeviceSynchronize();
            instep_harvest(m, true);
        }
        return m->instep.total_us[i] / (double)m->instep.steps;
    }
    if (m->timing.samples[i] == 0) return 0.0;
    return m->timing.total_us[i] / (double)m->timing.samples[i];
}
double sert_timing_launches(sert_model* m, int i) {
    if (!m || i < 0 || i >= TG_COUNT || m->instep.steps == 0) return 0.0;
    return (double)m->instep.launches[i] / (double)m->instep.steps;
}

int sert_bench_gemm(int device, int ta, int tb, int epi, int M, int N, int K, int splits, int iters,
                    double* avg_us) {
    refresh_gemm_choice();
    if (!avg_us || M <= 0 || N <= 0 || K <= 0 || iters <= 0) SERT_FAIL("bad argument");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (splits < 1) splits = 1;
    int kper = (int)round_up(cdiv(K, splits), GK);
    splits = cdiv(K, kper);
    // SERT_BENCH_GEMM_CSB=1 (A^T.B only): with the column sums of B riding along, as dW + db run in the step
    const bool csb = ta && !tb && variant_knob("SERT_BENCH_GEMM_CSB") != nullptr;
    const size_t na = (size_t)M * K, nb = (size_t)K * N, nc = ((size_t)M * N + (csb ? N : 0)) * splits;
    float *A = nullptr, *B = nullptr, *C = nullptr, *bias = nullptr;
    SERT_TRY(dmalloc(&A, na)); SERT_TRY(dmalloc(&B, nb)); SERT_TRY(dmalloc(&C, nc)); SERT_TRY(dmalloc(&bias, (size_t)N));
    std::vector<float> h(std::max(std::max(na, nb), (size_t)N));
    uint32_t x = 12345u;
    auto fill = [&](float* d, size_t n) {
        for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; h[i] = ((x >> 8) * (1.0f / 8388608.0f)) - 1.0f; }
        return hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice);
    };
    SERT_HIP(fill(A, na)); SERT_HIP(fill(B, nb)); SERT_HIP(fill(bias, (size_t)N));
    const int lda = ta ? M : K, ldb = tb ? K : N;
#ifdef SERT_VARIANTS
    const int big = (variant_knob("SERT_GEMM_BIG") && !ta && tb && gemm_big_ok(K, lda, ldb) && splits == 1) ? atoi(variant_knob("SERT_GEMM_BIG")) : 0;
#endif
    auto run = [&]() {
#ifdef SERT_VARIANTS
        if (big) { launch_gemm_big_nt(s, A, B, C, M, N, K, lda, ldb, N, big == 2); return; }
#endif
#define SERT_BG(TA, TB, E) launch_gemm<TA, TB, E>(s, A, B, C, bias, M, N, K, lda, ldb, N, splits, kper, (size_t)M * N)
        if (!ta && !tb) { if (epi == 2) SERT_BG(false, false, EPI_BIAS_TANH); else if (epi == 1) SERT_BG(false, false, EPI_BIAS); else SERT_BG(false, false, EPI_STORE); }
        else if (csb) launch_gemm<true, false, EPI_STORE, true>(s, A, B, C, bias, M, N, K, lda, ldb, N, splits, kper, (size_t)M * N + N);
        else if (ta && !tb) SERT_BG(true, false, EPI_STORE);
        else if (!ta && tb) SERT_BG(false, true, EPI_STORE);
        else SERT_BG(true, true, EPI_STORE);
#undef SERT_BG
    };
    hipEvent_t e0, e1;
    SERT_HIP(hipEventCreate(&e0)); SERT_HIP(hipEventCreate(&e1));
    run(); run();
    SERT_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) run();
    SERT_HIP(hipEventRecord(e1, s));
    SERT_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    SERT_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = 1000.0 * ms / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(A); (void)hipFree(B); (void)hipFree(C); (void)hipFree(bias);
    (void)hipStreamDestroy(s);
    return 0;
}

// the k ranges of the two split forms below: whole GK steps per range, no empty range at the end
static inline int debug_k_ranges(int K, int splits, int* kper) {
    *kper = (int)round_up(cdiv(K, splits), GK);
    return cdiv(K, *kper);
}

// Host only: the GemmRoute (gemm.h) the three hooks below end in for a shape -- the predicates launch_gemm, launch_gemm_x3 and
// launch_gemm_x3_ta ask, on operands of which only the alignment exists.  < 0: bad argument.
static_assert(ROUTE_F32_SMALL == SERT_GEMM_ROUTE_F32_TILE64 && ROUTE_F32_TILE128 == SERT_GEMM_ROUTE_F32_TILE128 &&
              ROUTE_F32_N160 == SERT_GEMM_ROUTE_F32_TILE128X160 && ROUTE_X3_128_VEC == SERT_GEMM_ROUTE_X3_128_VEC &&
              ROUTE_X3_128_SCALAR == SERT_GEMM_ROUTE_X3_128_SCALAR && ROUTE_X3_256 == SERT_GEMM_ROUTE_X3_256 &&
              ROUTE_X3_320 == SERT_GEMM_ROUTE_X3_320 && ROUTE_X3_TA_SINGLE == SERT_GEMM_ROUTE_X3_TA_SINGLE &&
              ROUTE_X3_TA_320X160 == SERT_GEMM_ROUTE_X3_TA_320X160 && ROUTE_X3_TA_TILES == SERT_GEMM_ROUTE_X3_TA_TILES,
              "GemmRoute (gemm.h) is the header's SERT_GEMM_ROUTE_*");
int sert_debug_gemm_route(int form, int ta, int tb, int M, int N, int K, int splits, int align) {
    refresh_gemm_choice();
    if (form < 0 || form > 2 || M <= 0 || N <= 0 || K <= 0 || splits <= 0 || align <= 0) {
        (void)::sert::fail(__FILE__, __LINE__, "bad argument");
        return -1;
    }
    const float* A = reinterpret_cast<const float*>((uintptr_t)align);   // (never dereferenced)
    const float* B = A;
    int kper = K;
    bool csb = false;
    if (form == SERT_GEMM_FORM_PLAIN) splits = 1;
    else {
        if (form == SERT_GEMM_FORM_SPLITK) { ta = 1; tb = 0; csb = true; } else ta = 0;
        splits = debug_k_ranges(K, splits, &kper);
        if (splits <= 1) { splits = 1; kper = K; }      // (launch_gemm: one k range is no split)
    }
    const int lda = ta ? M : K, ldb = tb ? K : N;
    return gemm_route(ta != 0, tb != 0, EPI_STORE, csb, false, A, B, M, N, K, lda, ldb, splits, kper);
}

// C = epi(op(A).op(B)) for host arrays, through launch_gemm -- i.e. through whichever kernel a shape is routed to in a
// training step (tests/test_gpu_gemm.py pins every kernel of gemm.h / gemm_stream.h against float64 this way).
int sert_debug_gemm(int device, int ta, int tb, int epi, int M, int N, int K, const float* A, const float* B,
                    const float* bias, float* C) {
    refresh_gemm_choice();
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || epi < 0 || epi > 2 || (epi && !bias)) SERT_FAIL("bad argument");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const size_t na = (size_t)M * K, nb = (size_t)K * N, nc = (size_t)M * N;
    float *dA = nullptr, *dB = nullptr, *dC = nullptr, *dbias = nullptr;
    int rc = 0;
    auto body = [&]() -> int {
        SERT_TRY(dmalloc(&dA, na)); SERT_TRY(dmalloc(&dB, nb)); SERT_TRY(dmalloc(&dC, nc)); SERT_TRY(dmalloc(&dbias, (size_t)N));
        SERT_HIP(hipMemcpyAsync(dA, A, na * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemcpyAsync(dB, B, nb * sizeof(float), hipMemcpyHostToDevice, s));
        if (bias) SERT_HIP(hipMemcpyAsync(dbias, bias, (size_t)N * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemsetAsync(dC, 0xff, nc * sizeof(float), s));      // (NaNs wherever the kernel does not write)
        const int lda = ta ? M : K, ldb = tb ? K : N;
#define SERT_DG(TA, TB, E) launch_gemm<TA, TB, E>(s, dA, dB, dC, dbias, M, N, K, lda, ldb, N)
        if (!ta && !tb) { if (epi == 2) SERT_DG(false, false, EPI_BIAS_TANH); else if (epi == 1) SERT_DG(false, false, EPI_BIAS); else SERT_DG(false, false, EPI_STORE); }
        else if (!ta && tb) { if (epi == 2) SERT_DG(false, true, EPI_BIAS_TANH); else if (epi == 1) SERT_DG(false, true, EPI_BIAS); else SERT_DG(false, true, EPI_STORE); }
        else if (ta && !tb) SERT_DG(true, false, EPI_STORE);
        else SERT_DG(true, true, EPI_STORE);
#undef SERT_DG
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipMemcpyAsync(C, dC, nc * sizeof(float), hipMemcpyDeviceToHost, s));
        SERT_HIP(hipStreamSynchronize(s));
        return 0;
    };
    rc = body();
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC); (void)hipFree(dbias);
    (void)hipStreamDestroy(s);
    return rc;
}

// out (M * N + N) = A^T.B (A (K, M), B (K, N) host arrays) followed by the column sums of B, through the split-K launch
// + order-fixed combine the projection's dW / db take in a training step (tests/test_gpu_gemm.py)
int sert_debug_gemm_splitk(int device, int M, int N, int K, int splits, const float* A, const float* B, float* out) {
    refresh_gemm_choice();
    if (!A || !B || !out || M <= 0 || N <= 0 || K <= 0 || splits <= 0) SERT_FAIL("bad argument");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int kper = 0;
    splits = debug_k_ranges(K, splits, &kper);
    const size_t na = (size_t)K * M, nb = (size_t)K * N, stride = (size_t)M * N + N;
    float *dA = nullptr, *dB = nullptr, *dP = nullptr, *dO = nullptr;
    auto body = [&]() -> int {
        SERT_TRY(dmalloc(&dA, na)); SERT_TRY(dmalloc(&dB, nb)); SERT_TRY(dmalloc(&dP, stride * splits)); SERT_TRY(dmalloc(&dO, stride));
        SERT_HIP(hipMemcpyAsync(dA, A, na * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemcpyAsync(dB, B, nb * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemsetAsync(dP, 0xff, stride * splits * sizeof(float), s));
        launch_gemm<true, false, EPI_STORE, true>(s, dA, dB, dP, nullptr, M, N, K, M, N, N, splits, kper, stride);
        launch_reduce_partials(s, dP, splits, stride, stride, dO, stride, dO);
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipMemcpyAsync(out, dO, stride * sizeof(float), hipMemcpyDeviceToHost, s));
        SERT_HIP(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dP); (void)hipFree(dO);
    (void)hipStreamDestroy(s);
    return rc;
}

// C (M, N) = A . op(B) over a LONG K cut into `splits` k ranges (partial slabs + order-fixed combine): the form the loglinear
// dG = dZ.W^T takes over 100 000 entities (gemm_long_k).  A (M, K), B (K, N) or (N, K) if tb: host arrays.
int sert_debug_gemm_longk(int device, int tb, int M, int N, int K, int splits, const float* A, const float* B, float* C) {
    refresh_gemm_choice();
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || splits <= 0) SERT_FAIL("bad argument");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int kper = 0;
    splits = debug_k_ranges(K, splits, &kper);
    const size_t na = (size_t)M * K, nb = (size_t)K * N, mn = (size_t)M * N;
    float *dA = nullptr, *dB = nullptr, *dP = nullptr, *dO = nullptr;
    auto body = [&]() -> int {
        SERT_TRY(dmalloc(&dA, na)); SERT_TRY(dmalloc(&dB, nb)); SERT_TRY(dmalloc(&dP, mn * splits)); SERT_TRY(dmalloc(&dO, mn));
        SERT_HIP(hipMemcpyAsync(dA, A, na * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemcpyAsync(dB, B, nb * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemsetAsync(dP, 0xff, mn * splits * sizeof(float), s));
        if (tb) launch_gemm<false, true, EPI_STORE>(s, dA, dB, dP, nullptr, M, N, K, K, K, N, splits, kper, mn);
        else    launch_gemm<false, false, EPI_STORE>(s, dA, dB, dP, nullptr, M, N, K, K, N, N, splits, kper, mn);
        launch_reduce_partials(s, dP, splits, mn, mn, dO, mn, dO);
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipMemcpyAsync(C, dO, mn * sizeof(float), hipMemcpyDeviceToHost, s));
        SERT_HIP(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dP); (void)hipFree(dO);
    (void)hipStreamDestroy(s);
    return rc;
}

int sert_bench_memory(int device, int kind, size_t bytes, size_t table_bytes, int row_bytes, int window,
                      size_t gap_bytes, int blocks, int iters, double* avg_us) {
    if (!avg_us || iters <= 0 || bytes < 4096) SERT_FAIL("bad argument");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::vector<void*> owned;
    auto alloc = [&](size_t b, void** out) -> int {
        SERT_HIP(hipMalloc(out, b));
        owned.push_back(*out);
        return 0;
    };
    auto cleanup = [&]() {
        for (void* p : owned) (void)hipFree(p);
        (void)hipStreamDestroy(s);
    };
    const size_t n = (bytes / 16) * 4;   // floats per array (multiple of 4)
    std::function<void()> run;
    int rc = 0;
    if (kind == SERT_MEMBENCH_COPY || kind == SERT_MEMBENCH_READ) {
        float *a = nullptr, *b = nullptr;
        if ((rc = alloc(n * 4, (void**)&a)) || (rc = alloc(kind == SERT_MEMBENCH_COPY ? n * 4 : 65536 * 4, (void**)&b))) { cleanup(); return rc; }
        launch(mb_fill_f32, dim3(2048), dim3(256), 0, s, a, n, 1.0f);
        const int nb = blocks > 0 ? blocks : 4096;
        if (kind == SERT_MEMBENCH_COPY)
            run = [=]() { launch(mb_stream_copy, dim3(nb), dim3(256), 0, s, (const float4*)a, (float4*)b, n / 4); };
        else
            run = [=]() { launch(mb_stream_read, dim3(nb), dim3(256), 0, s, (const float4*)a, n / 4, b); };
    } else if (kind == SERT_MEMBENCH_GATHER) {
        if (row_bytes < 16 || row_bytes % 16 || window < 1 || table_bytes < (size_t)row_bytes) { cleanup(); SERT_FAIL("bad gather shape"); }
        const int d = row_bytes / 4;
        const size_t rows = table_bytes / (size_t)row_bytes;
        const size_t B = std::max<size_t>(1, n / d);
        if (rows >= ((size_t)1 << 32) || B >= ((size_t)1 << 31)) { cleanup(); SERT_FAIL("gather shape too large"); }
        float *tab = nullptr, *out = nullptr; uint32_t* ids = nullptr;
        if ((rc = alloc(rows * row_bytes, (void**)&tab)) || (rc = alloc(B * row_bytes, (void**)&out)) ||
            (rc = alloc(B * window * 4, (void**)&ids))) { cleanup(); return rc; }
        launch(mb_fill_f32, dim3(2048), dim3(256), 0, s, tab, rows * d, 1.0f);
        launch(mb_fill_ids, dim3(2048), dim3(256), 0, s, ids, B * window, (uint32_t)rows, 17u);
        const int grid = grid_for((int64_t)B * d / 4, 256, 1 << 20);
        run = [=]() { launch((vs_gather_mean<uint32_t, 4>), dim3(grid), dim3(256), 0, s, (const uint32_t*)ids, (const float*)tab, out, (int)B, window, d); };
    } else if (kind == SERT_MEMBENCH_OPTIMIZER) {
        float* arr[4] = {nullptr, nullptr, nullptr, nullptr};
        if (gap_bytes == (size_t)-1) {   // four allocations of their own, as the model holds them
            for (int k = 0; k < 4; ++k) if ((rc = alloc(n * 4, (void**)&arr[k]))) { cleanup(); return rc; }
        } else {
            if (gap_bytes % 16) { cleanup(); SERT_FAIL("gap must be a multiple of 16 bytes"); }
            char* base = nullptr;
            if ((rc = alloc(4 * (n * 4 + gap_bytes), (void**)&base))) { cleanup(); return rc; }
            for (int k = 0; k < 4; ++k) arr[k] = (float*)(base + (size_t)k * (n * 4 + gap_bytes));
        }
        float* sq = nullptr;
        if ((rc = alloc((size_t)8 * kOptBlocks * 4, (void**)&sq))) { cleanup(); return rc; }
        launch(mb_fill_f32, dim3(2048), dim3(256), 0, s, arr[0], n, 0.01f);
        launch(mb_fill_f32, dim3(2048), dim3(256), 0, s, arr[1], n, 1e-4f);
        SERT_HIP(hipMemsetAsync(arr[2], 0, n * 4, s));
        SERT_HIP(hipMemsetAsync(arr[3], 0, n * 4, s));
        const int nb = blocks > 0 ? std::min(blocks, 8 * kOptBlocks) : 2 * kOptBlocks;
        const AdamArgs aa{1e-7f, 1e-3f, 0.9f, 0.999f, 1e-8f};
        float *p = arr[0], *g = arr[1], *m1 = arr[2], *v1 = arr[3];
        run = [=]() { launch((adam_l2<false>), dim3(nb), dim3(256), 0, s, p, g, m1, v1, n, aa, sq, (const uint32_t*)nullptr, 1u, (int)kRowsAll, nullptr); };
    } else {
        cleanup();
        SERT_FAIL("unknown membench kind");
    }
    hipEvent_t e0, e1;
    SERT_HIP(hipEventCreate(&e0)); SERT_HIP(hipEventCreate(&e1));
    run(); run();
    SERT_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) run();
    SERT_HIP(hipEventRecord(e1, s));
    const hipError_t se = hipStreamSynchronize(s);
    float ms = 0.f;
    if (se == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
    *avg_us = 1000.0 * ms / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    cleanup();
    SERT_HIP(se);
    SERT_HIP(hipGetLastError());
    return 0;
}
