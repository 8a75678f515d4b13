// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): C ABI: sert_upload_dataset, training, evaluation, prediction.

// Label rows as a CSR matrix (rows, cols), validated on the host before any kernel indexes with them: indptr starts at 0 and
// never decreases, at most max_nnz entries, every column in [0, cols) (col_error: the caller's wording of that range) and
// strictly increasing within a row -- the loss kernels add a row's label entries from different threads without atomics, two
// entries of one column would race, and the fold-in's row kernel finds a column by bisection.  The one statement behind
// sert_upload_dataset, sert_ll_foldin_upload_csr and sert_ll_wfold_upload_csr.
static int check_csr_rows(const int64_t* indptr, const int32_t* indices, const float* data, int64_t rows, int64_t cols,
                          const char* col_error, int64_t max_nnz) {
    if (indptr[0] != 0) SERT_FAIL("csr_indptr[0] != 0");
    for (int64_t r = 0; r < rows; ++r)
        if (indptr[r + 1] < indptr[r]) SERT_FAIL("csr_indptr is not non-decreasing");
    const int64_t nnz = indptr[rows];
    if (nnz > max_nnz) SERT_FAIL("more than 2^31 - 1 label entries");
    if (nnz > 0 && (!indices || !data)) SERT_FAIL("bad argument");
    for (int64_t i = 0; i < nnz; ++i)
        if (indices[i] < 0 || indices[i] >= cols) SERT_FAIL(col_error);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t i = indptr[r] + 1; i < indptr[r + 1]; ++i)
            if (indices[i] <= indices[i - 1]) {
                char msg[160];
                snprintf(msg, sizeof msg, "csr_indices of row %lld are not strictly increasing (duplicate or unsorted label column %d)",
                         (long long)r, (int)indices[i]);
                SERT_FAIL(msg);
            }
    return 0;
}

int sert_upload_dataset(sert_model* m, int split, const void* x, const int32_t* y_int,
                        const int64_t* csr_indptr, const int32_t* csr_indices,
                        const float* csr_data, const float* w, int64_t N) {
    if (!m) SERT_FAIL("null model");
    invalidate_speculation(m);
    m->hint_next = -1;
    if (split != SERT_SPLIT_TRAIN && split != SERT_SPLIT_VALIDATE) SERT_FAIL("bad split");
    if (N < 0) SERT_FAIL("negative instance count");
    if (N > 0 && !x) SERT_FAIL("x is null");
    if (N > 0 && !y_int && !(csr_indptr && csr_indices && csr_data)) SERT_FAIL("no labels given");
    if (is_vs(m) && N > 0 && !y_int) SERT_FAIL("vectorspace requires int labels (models.py:933-934)");
    SERT_HIP(hipSetDevice(m->cfg.device));
    // Every id the kernels will index with is checked here, once, on the host: the reference
    // raises IndexError for an out-of-range token or label (numpy / Theano advanced indexing);
    // on the device it would be an out-of-bounds read, and in the backward a write.
    if (N > 0) {
        const size_t toks = (size_t)N * m->cfg.window_size;
        const uint32_t Vw = (uint32_t)m->cfg.vocab_size;
        bool ok = true;
        SERT_ID_DISPATCH(m->cfg.id_bytes, {
            const IdT* xi = (const IdT*)x;
            uint32_t mx = 0;
            for (size_t i = 0; i < toks; ++i) mx = std::max<uint32_t>(mx, (uint32_t)xi[i]);
            ok = mx < Vw;
        });
        if (!ok) SERT_FAIL("token id >= vocab_size in x");
        const int32_t Ve = m->cfg.num_entities;
        if (y_int) {
            for (int64_t i = 0; i < N; ++i)
                if (y_int[i] < 0 || y_int[i] >= Ve) SERT_FAIL("label out of range [0, num_entities) in y");
        } else {
            // (the model's split states no limit on its label entries: none is checked here, as before)
            SERT_TRY(check_csr_rows(csr_indptr, csr_indices, csr_data, N, Ve, "label column out of range [0, num_entities) in csr_indices",
                                    INT64_MAX));
        }
    }
    DataSplit& d = m->split[split];
    free_split(d);
    d.N = N;
    if (N == 0) return 0;
    hipStream_t s = m->stream;
    const size_t xbytes = (size_t)N * m->cfg.window_size * m->cfg.id_bytes;
    SERT_HIP(hipMalloc(&d.x, xbytes));
    SERT_HIP(hipMemcpyAsync(d.x, x, xbytes, hipMemcpyHostToDevice, s));
    if (y_int) {
        d.max_labels_per_row = 1;
        SERT_TRY(dmalloc(&d.y, (size_t)N));
        SERT_HIP(hipMemcpyAsync(d.y, y_int, N * sizeof(int32_t), hipMemcpyHostToDevice, s));
    } else {
        d.nnz = csr_indptr[N];
        for (int64_t r = 0; r < N; ++r)
            d.max_labels_per_row = std::max<int64_t>(d.max_labels_per_row, csr_indptr[r + 1] - csr_indptr[r]);
        SERT_TRY(dmalloc(&d.csr_indptr, (size_t)N + 1));
        SERT_TRY(dmalloc(&d.csr_indices, (size_t)std::max<int64_t>(1, d.nnz)));
        SERT_TRY(dmalloc(&d.csr_data, (size_t)std::max<int64_t>(1, d.nnz)));
        SERT_HIP(hipMemcpyAsync(d.csr_indptr, csr_indptr, (N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (d.nnz) {
            SERT_HIP(hipMemcpyAsync(d.csr_indices, csr_indices, d.nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(d.csr_data, csr_data, d.nnz * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    if (split == SERT_SPLIT_TRAIN) {
        SERT_TRY(dmalloc(&d.w, (size_t)N));
        if (w) {
            SERT_HIP(hipMemcpyAsync(d.w, w, N * sizeof(float), hipMemcpyHostToDevice, s));
        } else {
            std::vector<float> ones((size_t)N, 1.0f);
            SERT_HIP(hipMemcpyAsync(d.w, ones.data(), N * sizeof(float), hipMemcpyHostToDevice, s));
            SERT_HIP(hipStreamSynchronize(s));
        }
    }
    if (split == SERT_SPLIT_TRAIN && !m->cfg.inference_only && !is_vs(m))
        SERT_TRY(dmalloc(&d.labfix, (size_t)std::max<int64_t>(1, y_int ? N : d.nnz)));
    if (split == SERT_SPLIT_TRAIN && !m->cfg.inference_only) {
        const int B = m->cfg.batch_size, n = m->cfg.window_size;
        const int64_t nb = N / B;
        WordIndex wi;
        const bool row_is_pos = !is_vs(m);
        // vectorspace models: the heavy words of a batch are summed by one dense pass (word_index.h);
        // SERT_NO_DENSE_HEAVY=1 keeps them in the tree (cross-check knob)
        // (loglinear: the V_e-wide per-word sums are bandwidth-bound; on by default where V_e % 4 == 0.  vectorspace: as two
        //  launches in FRONT of the tree the pass cost what the heavy words' entries saved -- round 3: 56.4 against 55.6 us at C2,
        //  opt-in then.  Round 5: inside the tree's own launches (kernels_seg.h: segsum_rows_plus -- the stream beside the
        //  latency-bound level 0, the combine beside level 1) the C2 tree takes 42.6 us instead of 55.8 and the step 0.2481 ->
        //  0.2374 ms, C4 1.386 -> 1.361, C2 dims at 8192 rows 0.0988 -> 0.0964, product-search settings 0.1762 -> 0.1750
        //  (tools/experiments/r05_heavy_fused.sh; the two launches in front: 0.257, 1.440, 0.114, 0.181).  ON by default where
        //  the tree runs its 32-lane forms (d_w / 4 <= 32, or rows that three 32-lane column groups cover better than two
        //  64-lane ones); SERT_DENSE_HEAVY=0 / 1 forces it off / on.)
        bool vs_heavy = false;
        if (is_vs(m) && m->cfg.word_dim % 4 == 0 && m->cfg.word_dim <= 512) {
            const int d4 = m->cfg.word_dim / 4;
            const bool lpi32 = d4 <= 32 || (d4 > 64 && 64 * cdiv(d4, 64) > 32 * cdiv(d4, 32));
            const bool bundle_on = variant_knob("SERT_SEG_BUNDLE") && atoi(variant_knob("SERT_SEG_BUNDLE")) != 0;
            vs_heavy = knob("SERT_DENSE_HEAVY") ? atoi(knob("SERT_DENSE_HEAVY")) != 0 : (lpi32 && !bundle_on);
        }
        const bool dense_heavy = !variant_knob("SERT_NO_DENSE_HEAVY") && (is_vs(m) ? vs_heavy : (m->cfg.num_entities % 4 == 0));
        // Row-grouped level 0 of the vectorspace word-gradient tree (word_index.h: row_groups; kernels_seg.h: XcdLists):
        // MEASURED AND NOT USED (round 4, profiles/r04_experiments.txt).  At C2 it does what it was built for -- the
        // fabric traffic of the tree falls from 264 MB to 149 MB per step (level 0: 237 -> 98 MB) -- and level 0 takes
        // the same 41.5 us while the upper level grows from 8 to 14 us (100 k items and 75 k partial rows instead of
        // 52 k and 10 k): the step 0.2945 -> 0.3114 ms with 8 row ranges, 0.318 with 16, 0.325 with 32.
        // SERT_SEG_GROUPS=k builds it (tests/test_gpu_parity.py::test_word_gradient_row_grouped_tree keeps it exact).
        int row_groups = 1;
        if (is_vs(m) && m->cfg.word_dim % 4 == 0)
            if (const char* e = variant_knob("SERT_SEG_GROUPS")) row_groups = std::min(std::max(1, atoi(e)), std::max(1, B / 64));
        // vectorspace: level 0 sorted by item length with the first row number in the descriptor (word_index.h: slot_is_row);
        // not with bundles (they need the items in entry order); SERT_SEG_NO_SORT (variants build) for the A/B
        const bool sort_level0 = is_vs(m) && row_groups == 1 && !(variant_knob("SERT_SEG_BUNDLE") && atoi(variant_knob("SERT_SEG_BUNDLE")) != 0) &&
                                 !variant_knob("SERT_SEG_NO_SORT");
        bool ids_ok = true;
        SERT_ID_DISPATCH(m->cfg.id_bytes,
                         ids_ok = build_word_index<IdT>((const IdT*)x, nb, B, n, m->cfg.vocab_size, row_is_pos, wi,
                                                        /*want_slots=*/!is_vs(m), /*dense_heavy=*/dense_heavy, row_groups, sort_level0));
        if (!ids_ok) SERT_FAIL("token id >= vocab_size in x");
        if (!is_vs(m) && !wi.slots.empty()) {
            const size_t V = (size_t)m->cfg.num_entities;
            SERT_TRY(dmalloc(&d.idx_uwords, std::max<size_t>(1, wi.uwords.size())));
            SERT_TRY(dmalloc(&d.idx_slots, wi.slots.size()));
            SERT_HIP(hipMemcpyAsync(d.idx_uwords, wi.uwords.data(), wi.uwords.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(d.idx_slots, wi.slots.data(), wi.slots.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_TRY(dmalloc(&d.idx_rows_div, wi.rows_div.size()));
            SERT_HIP(hipMemcpyAsync(d.idx_rows_div, wi.rows_div.data(), wi.rows_div.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipStreamSynchronize(s));
            if ((size_t)wi.max_distinct > m->zu_rows) {
                (void)hipFree(m->Zu); (void)hipFree(m->dZu);
                m->Zu = nullptr; m->dZu = nullptr;
                m->zu_rows = (size_t)wi.max_distinct;
                SERT_TRY(dmalloc(&m->Zu, m->zu_rows * V));
                SERT_TRY(dmalloc(&m->dZu, m->zu_rows * V));
            }
            if ((size_t)wi.max_part_rows + 1 > m->zpart_rows) {
                (void)hipFree(m->zpart);
                m->zpart = nullptr;
                m->zpart_rows = (size_t)wi.max_part_rows + 1;
                SERT_TRY(dmalloc(&m->zpart, m->zpart_rows * V));
            }
        }
        if (!wi.rows.empty()) {
            SERT_TRY(dmalloc(&d.idx_rows, wi.rows.size()));
            SERT_HIP(hipMemcpyAsync(d.idx_rows, wi.rows.data(), wi.rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMalloc((void**)&d.idx_items, std::max<size_t>(1, wi.items.size()) * sizeof(SegItem)));
            SERT_HIP(hipMemcpyAsync(d.idx_items, wi.items.data(), wi.items.size() * sizeof(SegItem), hipMemcpyHostToDevice, s));
            if (!wi.heavy.empty()) {
                SERT_HIP(hipMalloc((void**)&d.idx_heavy, wi.heavy.size() * sizeof(int32_t)));
                SERT_HIP(hipMemcpyAsync(d.idx_heavy, wi.heavy.data(), wi.heavy.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            }
            // OPT-IN (SERT_SEG_BUNDLE=1, read at upload: two models of one process can run either way).  Measured SLOWER
            // (round 5, profiles/r05_experiments.txt: C2 word-gradient group 59.5 us against 56.7, C4 150.9 against 145.0): the
            // short items are not what level 0 waits for -- with their lane groups leaving right after the descriptor load
            // (a knock-out) the group loses 7 of 57 us.
            const bool bundle = variant_knob("SERT_SEG_BUNDLE") && atoi(variant_knob("SERT_SEG_BUNDLE")) != 0;
            if (!wi.bundles.empty() && bundle && is_vs(m)) {
                SERT_TRY(dmalloc(&d.idx_bundles, wi.bundles.size()));
                SERT_HIP(hipMemcpyAsync(d.idx_bundles, wi.bundles.data(), wi.bundles.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            }
            SERT_HIP(hipStreamSynchronize(s));
        }
        if (!wi.touched_bits.empty()) {
            SERT_TRY(dmalloc(&d.idx_touched_bits, wi.touched_bits.size()));
            SERT_HIP(hipMemcpyAsync(d.idx_touched_bits, wi.touched_bits.data(), wi.touched_bits.size() * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, s));
            SERT_HIP(hipStreamSynchronize(s));
            d.bit_words = wi.bit_words;
        }
        // data parallel, word table owned by rows: the per-batch exchange lists (collective)
        if (is_dp(m)) SERT_TRY(xr_build_lists(m, wi.touched_bits, nb, wi.bit_words));
        if (wi.any_dense) {
            SERT_HIP(hipMalloc((void**)&d.idx_dense_counts, wi.dense_counts.size()));
            SERT_HIP(hipMemcpyAsync(d.idx_dense_counts, wi.dense_counts.data(), wi.dense_counts.size(), hipMemcpyHostToDevice, s));
            std::vector<int32_t> hw((size_t)nb * kHeavyMax, 0);
            for (int64_t b = 0; b < nb; ++b)
                for (int h = 0; h < wi.batches[(size_t)b].dense_cnt; ++h) hw[(size_t)b * kHeavyMax + h] = wi.batches[(size_t)b].dense_word[h];
            // (only where the opt-in gather that reads it is switched on: a byte per token of the data set)
            if (!wi.dense_tok_slot.empty() && variant_knob("SERT_GATHER_HOT") && atoi(variant_knob("SERT_GATHER_HOT")) != 0) {
                SERT_HIP(hipMalloc((void**)&d.idx_tok_slot, wi.dense_tok_slot.size()));
                SERT_HIP(hipMemcpyAsync(d.idx_tok_slot, wi.dense_tok_slot.data(), wi.dense_tok_slot.size(), hipMemcpyHostToDevice, s));
                d.dense_cnt_of.resize((size_t)nb);
                for (int64_t b = 0; b < nb; ++b) d.dense_cnt_of[(size_t)b] = wi.batches[(size_t)b].dense_cnt;
            }
            SERT_TRY(dmalloc(&d.idx_dense_words, hw.size()));
            SERT_HIP(hipMemcpyAsync(d.idx_dense_words, hw.data(), hw.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipStreamSynchronize(s));
            if (!m->hpart)
                // (row blocks of the form that runs: the fused stream's heavy_rows_fused(B) rows or the two launches'
                //  kHeavyRowsPerBlock -- sized for the smallest block, 64 rows, a loglinear model at batch 65536 and 100 k
                //  entities asked for 6.5 GB where 1.6 GB is used)
                SERT_TRY(dmalloc(&m->hpart, (size_t)std::max(cdiv(B, heavy_rows_fused(B)), cdiv(B, kHeavyRowsPerBlock)) * kHeavyMax *
                                               (size_t)(is_vs(m) ? m->cfg.word_dim : m->cfg.num_entities)));
        } else {
            for (auto& bxx : wi.batches) bxx.dense_cnt = 0;
        }
        d.idx_batches = wi.batches;
        if ((size_t)wi.max_part_rows + 1 > m->wpart_rows) {
            (void)hipFree(m->wpart);
            m->wpart_rows = (size_t)wi.max_part_rows + 1;
            SERT_TRY(dmalloc(&m->wpart, m->wpart_rows * m->cfg.word_dim));
        }
    }
    SERT_HIP(hipStreamSynchronize(s));
    return 0;
}

int sert_train_batch(sert_model* m, int64_t batch_index, const int64_t* negatives, float* loss_out) {
    refresh_gemm_choice();
    if (!m) SERT_FAIL("null model");
    SERT_HIP(hipSetDevice(m->cfg.device));
    static const bool no_spin = variant_knob("SERT_NO_SPIN") != nullptr;   // cross-check knob
    // sert_hint_next_batch: the next batch's parameter-only forward part goes out behind
    // this step, before the host starts waiting for this step's loss
    const int64_t hint = m->hint_next;
    m->hint_next = -1;
    m->lazy_next = hint;
    auto prefetch_next = [&]() -> int {
        const DataSplit& ds = m->split[SERT_SPLIT_TRAIN];
        if (will_run_ahead(m, hint)) {
            // the whole forward + backward of the announced batch runs ahead: it depends on the
            // parameters (final: this step's update is already in the stream), the data and the
            // step counter only, and writes activations / gradient scratch only.  The UPDATE of
            // that step is not issued before the host has seen this step's loss.
            bool fused = false;
            SERT_TRY(step_forward_backward(m, ds, hint, nullptr, &fused));
            m->spec_fb_batch = hint;
            m->spec_fb_step = m->step;
            return 0;
        }
        // (keep_grads: the caller may read this batch's activations after the call)
        if (hint < 0 || m->timing.enabled || m->cfg.keep_grads) return 0;
        if ((hint + 1) * (int64_t)m->cfg.batch_size > ds.N) return 0;
        if (is_vs(m) && !is_fs(m)) {
            // data parallel: the parameter-only part (by rows: behind the fetch of the rows it reads)
            if (m->xr_on) SERT_TRY(xr_fetch_params(m, hint));
            SERT_TRY(vs_project(m, ds, hint));
            m->projected_batch = hint;
        } else if (m->xr_on) {
            SERT_TRY(xr_fetch_params(m, hint));
        }
        return 0;
    };
    if (m->timing.enabled || no_spin) {
        SERT_TRY(train_step_async(m, batch_index, negatives, m->d_loss));
        SERT_HIP(hipMemcpyAsync(m->h_loss, m->d_loss, 3 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        SERT_HIP(hipEventRecord(m->ev_loss, m->stream));
        SERT_TRY(prefetch_next());
        SERT_HIP(hipEventSynchronize(m->ev_loss));   // (not the stream: the next batch may be running ahead)
        timing_collect(m);
        if (loss_out) *loss_out = m->h_loss[0];
        return 0;
    }
    // The step's last kernel writes the loss straight into pinned host memory followed by
    // a sequence number; the host spins on that word -- no copy kernel and no stream
    // synchronisation on the per-step read-back the reference's epoch loop performs
    // (sert/models.py:369-379): 0.412 -> 0.396 ms/step at C2.  Everything the step did is
    // stream-ordered before that kernel, so the parameters are final when the number appears.
    // A step whose announced next batch will run ahead right behind it leaves its tail launch (vs_tail: dW / db combine, the
    // W, b update, the loss) to that batch's gather launch (kernels_vs.h: vs_gather_mean_tail; vs_project).  Whatever
    // prefetch_next does -- nothing, an error -- a tail no gather carried is launched on its own before the host waits:
    // a step is never left without its publisher.  (SERT_TAIL_IN_GATHER=0, variants build: every tail alone.)
    static const bool no_fold = variant_knob("SERT_TAIL_IN_GATHER") && atoi(variant_knob("SERT_TAIL_IN_GATHER")) == 0;
    // (single-GPU vectorspace: will_run_ahead then implies keep_grads off and word_dim % 4 == 0 -- the VEC == 4 gather --
    //  through use_touched_now; a gather launch of another form flushes the tail in front of itself, vs_project)
    m->tail_defer = !no_fold && !is_dp(m) && is_vs(m) && !is_fs(m) && will_run_ahead(m, hint);
    int rc = train_step_async(m, batch_index, negatives, m->h_loss_dev, true);
    m->tail_defer = false;
    if (rc == 0) rc = prefetch_next();
    flush_pending_tail(m);
    if (rc != 0) return rc;
    const unsigned want = m->loss_seq;
    volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(m->h_loss + 4);
    // A faulted step never publishes: ask the stream -- but RARELY.  hipStreamQuery on a stream whose last command carries no
    // completion signal makes the runtime enqueue a marker (a barrier packet) to get one; asked every 16 k spins (~5 us, the
    // flag is a cached read) the first marker landed right behind the run-ahead backward of the NEXT batch, and the next call's
    // word-table update started 6-7 us late behind it at every batch size (round 5: HIP API trace, tools/experiments/
    // r05_hip_trace.sh; sert_train_batches, which never asks, has no such gap).  Now: the clock every 4 k spins, the stream
    // only after 50 ms without a loss and every 50 ms from then on.
    {
        const auto t_spin0 = std::chrono::steady_clock::now();
        double next_query_ms = 50.0;
        for (unsigned spins = 1; *flag != want; ++spins) {
            if ((spins & 0xfff) != 0) continue;
            const double waited_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_spin0).count();
            if (waited_ms < next_query_ms) continue;
            next_query_ms = waited_ms + 50.0;
            const hipError_t q = hipStreamQuery(m->stream);   // (the stream the publishing kernel is on)
            if (q == hipSuccess) {
                if (*flag == want) break;
                SERT_FAIL("training step completed without publishing its loss");
            }
            if (q != hipErrorNotReady) SERT_HIP(q);
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (loss_out) *loss_out = m->h_loss[0];
    return 0;
}

int sert_hint_next_batch(sert_model* m, int64_t next_batch_index) {
    if (!m) SERT_FAIL("null model");
    m->hint_next = next_batch_index;
    return 0;
}

int sert_train_batches(sert_model* m, const int64_t* batch_indices, int64_t count, float* losses_out) {
    refresh_gemm_choice();
    if (!m || !batch_indices || count < 0) SERT_FAIL("bad argument");
    m->hint_next = -1;
    SERT_HIP(hipSetDevice(m->cfg.device));
    if (count == 0) return 0;
    if (m->d_losses_cap < count) {
        (void)hipFree(m->d_losses);
        SERT_TRY(dmalloc(&m->d_losses, (size_t)count * 3));
        m->d_losses_cap = count;
    }
    static const bool report_host = variant_knob("SERT_DEBUG_HOST") != nullptr;
    const auto t_host0 = std::chrono::steady_clock::now();
    for (int64_t i = 0; i < count; ++i) {
        m->lazy_next = i + 1 < count ? batch_indices[i + 1] : -1;
        SERT_TRY(train_step_async(m, batch_indices[i], nullptr, m->d_losses + 3 * i));
        if (m->timing.enabled) {  // events are single-slot: drain per step when timing
            SERT_HIP(hipStreamSynchronize(m->stream));
            timing_collect(m);
        }
    }
    if (report_host) {
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_host0).count();
        fprintf(stderr, "[sert] host enqueue: %.1f us/step over %lld steps\n", us / (double)count, (long long)count);
    }
    std::vector<float> tmp((size_t)count * 3);
    SERT_HIP(hipMemcpyAsync(tmp.data(), m->d_losses, count * 3 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    if (losses_out)
        for (int64_t i = 0; i < count; ++i) losses_out[i] = tmp[3 * i];
    return 0;
}

// One evaluation pass over a batch, enqueued on the main stream: forward + loss kernel, then the
// unweighted, unregularised batch mean (models.py:751-752) into dst[0] (device).
static int eval_step_async(sert_model* m, const DataSplit& ds, int64_t batch_index, const int64_t* negatives,
                           float* dst) {
    const int B = m->cfg.batch_size;
    SERT_TRY(settle_entity_update(m));
    SERT_TRY(ensure_rw_current(m, -1));
    if (is_fs(m)) {
        SERT_TRY(fs_forward<false>(m, ds, batch_index));
    } else if (is_vs(m)) {
        SERT_TRY(vs_negatives(m, negatives, (uint64_t)(m->eval_draws++) * 2 + 1, m->stream));
        SERT_TRY(vs_project(m, ds, batch_index));
        SERT_TRY(vs_loss<false>(m, ds, batch_index));
    } else {
        SERT_TRY(ll_forward<false>(m, ds, batch_index));
    }
    const int nb = std::min(kOptBlocks, cdiv(B, 256));
    launch(sum_partial, dim3(nb), dim3(256), 0, m->stream, m->rowloss, (size_t)B, m->red_loss);
    launch(finalize_loss, dim3(1), dim3(256), 0, m->stream, m->red_loss, nb, m->red_loss, 0,
           1.0f / (float)B, 0.0f, dst, nullptr, 0u, nullptr);
    return 0;
}

static int eval_check_args(sert_model* m, int split) {
    if (!m) SERT_FAIL("null model");
    if (split != SERT_SPLIT_TRAIN && split != SERT_SPLIT_VALIDATE) SERT_FAIL("bad split");
    if (m->cfg.inference_only) SERT_FAIL("model was created inference_only");
    return 0;
}

int sert_eval_batch(sert_model* m, int split, int64_t batch_index, const int64_t* negatives, float* loss_out) {
    refresh_gemm_choice();
    SERT_TRY(eval_check_args(m, split));
    invalidate_speculation(m);   // evaluation reuses the activation buffers and the negatives
    SERT_HIP(hipSetDevice(m->cfg.device));
    SERT_TRY(ensure_full_rw(m));
    const DataSplit& ds = m->split[split];
    const int B = m->cfg.batch_size;
    if (batch_index < 0 || (batch_index + 1) * (int64_t)B > ds.N) SERT_FAIL("batch_index out of range");
    SERT_TRY(eval_step_async(m, ds, batch_index, negatives, m->d_loss));
    SERT_HIP(hipMemcpyAsync(m->h_loss, m->d_loss, 3 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    float v = m->h_loss[0];
    if (is_dp(m)) {
        // eval loss of the global batch = mean of the per-rank means (equal shares)
        float* tmp = m->d_loss + 3;
        SERT_HIP(hipMemcpyAsync(tmp, m->d_loss, sizeof(float), hipMemcpyDeviceToDevice, m->stream));
        if (m->host_ar) SERT_TRY(host_allreduce(m, tmp, 1, m->stream));
        else            SERT_NCCL(g_rccl.AllReduce(tmp, tmp, 1, 7, 0, m->comm, m->stream));
        SERT_HIP(hipMemcpyAsync(m->h_loss, tmp, sizeof(float), hipMemcpyDeviceToHost, m->stream));
        SERT_HIP(hipStreamSynchronize(m->stream));
        v = m->h_loss[0] / (float)m->world;
    }
    timing_collect(m);
    if (loss_out) *loss_out = v;
    return 0;
}

int sert_eval_batches(sert_model* m, int split, const int64_t* batch_indices, int64_t count, float* losses_out) {
    refresh_gemm_choice();
    SERT_TRY(eval_check_args(m, split));
    if (!batch_indices || count < 0) SERT_FAIL("bad argument");
    if (count == 0) return 0;
    invalidate_speculation(m);
    SERT_HIP(hipSetDevice(m->cfg.device));
    SERT_TRY(ensure_full_rw(m));
    const DataSplit& ds = m->split[split];
    const int B = m->cfg.batch_size;
    for (int64_t i = 0; i < count; ++i)
        if (batch_indices[i] < 0 || (batch_indices[i] + 1) * (int64_t)B > ds.N) SERT_FAIL("batch_index out of range");
    if (m->d_losses_cap < count) {
        (void)hipFree(m->d_losses); m->d_losses = nullptr; m->d_losses_cap = 0;
        SERT_TRY(dmalloc(&m->d_losses, (size_t)count * 3));
        m->d_losses_cap = count;
    }
    // every batch writes its mean to its own slot: the host synchronises once per call
    for (int64_t i = 0; i < count; ++i) {
        SERT_TRY(eval_step_async(m, ds, batch_indices[i], nullptr, m->d_losses + 3 * i));
        if (m->timing.enabled) {  // events are single-slot: drain per step when timing
            SERT_HIP(hipStreamSynchronize(m->stream));
            timing_collect(m);
        }
    }
    if (is_dp(m)) {
        // global mean = mean of the per-rank means (equal shares): one collective over all slots
        if (m->host_ar) SERT_TRY(host_allreduce(m, m->d_losses, (size_t)count * 3, m->stream));
        else            SERT_NCCL(g_rccl.AllReduce(m->d_losses, m->d_losses, (size_t)count * 3, 7, 0, m->comm, m->stream));
    }
    std::vector<float> tmp((size_t)count * 3);
    SERT_HIP(hipMemcpyAsync(tmp.data(), m->d_losses, count * 3 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    const float scale = is_dp(m) ? 1.0f / (float)m->world : 1.0f;
    if (losses_out)
        for (int64_t i = 0; i < count; ++i) losses_out[i] = tmp[3 * i] * scale;
    return 0;
}

// grow-only device scratch (floats)
static int pred_reserve(float** buf, size_t* cap, size_t count) {
    if (*cap >= count) return 0;
    (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    SERT_TRY(dmalloc(buf, count));
    *cap = count;
    return 0;
}

int sert_predict_project(sert_model* m, const float* avg, int64_t Q, float* out) {
    refresh_gemm_choice();
    if (!m || !avg || !out) SERT_FAIL("null argument");
    if (!is_vs(m)) SERT_FAIL("sert_predict_project is the vectorspace predict_fn");
    if (Q <= 0) return 0;
    SERT_HIP(hipSetDevice(m->cfg.device));
    const int dw = m->cfg.word_dim, de = m->cfg.entity_dim;
    SERT_HIP(hipStreamSynchronize(m->stream));          // (the scratch may be in use by an earlier call's copy)
    SERT_TRY(pred_reserve(&m->pred_a, &m->pred_a_cap, (size_t)Q * dw));
    SERT_TRY(pred_reserve(&m->pred_b, &m->pred_b_cap, (size_t)Q * de));
    SERT_HIP(hipMemcpyAsync(m->pred_a, avg, (size_t)Q * dw * sizeof(float), hipMemcpyHostToDevice, m->stream));
    launch_gemm<false, false, EPI_BIAS_TANH>(m->stream, m->pred_a, m->W, m->pred_b, m->b, (int)Q, de, dw, dw, de, de);
    SERT_HIP(hipMemcpyAsync(out, m->pred_b, (size_t)Q * de * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    return 0;
}

int sert_predict_tokens(sert_model* m, const void* ids, int64_t rows, float* out) {
    refresh_gemm_choice();
    if (!m || !ids || !out) SERT_FAIL("null argument");
    if (is_vs(m)) SERT_FAIL("sert_predict_tokens is the loglinear predict_fn");
    if (rows <= 0) return 0;
    SERT_HIP(hipSetDevice(m->cfg.device));
    SERT_TRY(ensure_full_rw(m));
    SERT_TRY(ensure_rw_current(m, -1));
    const auto& c = m->cfg;
    const int n = c.window_size, d = c.word_dim, V = c.num_entities;
    const int64_t toks = rows * n;
    {
        bool ok = true;
        SERT_ID_DISPATCH(c.id_bytes, {
            const IdT* xi = (const IdT*)ids;
            for (int64_t i = 0; i < toks && ok; ++i) ok = (uint32_t)xi[i] < (uint32_t)c.vocab_size;
        });
        if (!ok) SERT_FAIL("token id >= vocab_size in ids");
    }
    SERT_HIP(hipStreamSynchronize(m->stream));
    if (m->pred_ids_cap < (size_t)toks * c.id_bytes) {
        (void)hipFree(m->pred_ids);
        m->pred_ids = nullptr; m->pred_ids_cap = 0;
        SERT_HIP(hipMalloc(&m->pred_ids, (size_t)toks * c.id_bytes));
        m->pred_ids_cap = (size_t)toks * c.id_bytes;
    }
    SERT_TRY(pred_reserve(&m->pred_a, &m->pred_a_cap, (size_t)toks * d));
    SERT_TRY(pred_reserve(&m->pred_b, &m->pred_b_cap, (size_t)toks * V));
    float *dG = m->pred_a, *dZ = m->pred_b;
    SERT_HIP(hipMemcpyAsync(m->pred_ids, ids, (size_t)toks * c.id_bytes, hipMemcpyHostToDevice, m->stream));
    SERT_ID_DISPATCH(c.id_bytes, {
        const IdT* X = (const IdT*)m->pred_ids;
        gather_rows(m->stream, X, m->rw, dG, toks, d);
    });
    launch_gemm<false, false, EPI_BIAS>(m->stream, dG, m->W, dZ, m->b, (int)toks, V, d, d, V, V);
    launch(ll_softmax_rows, dim3(cdiv(toks, 4)), dim3(256), 0, m->stream, dZ, toks, V);
    SERT_HIP(hipMemcpyAsync(out, dZ, (size_t)toks * V * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    return 0;
}
