// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: retrieval evaluation
// bound to the live model (include/sert_hip.h: sert_reval_*).  Topics and relevance judgements are uploaded once; a run ranks
// every topic with the parameters as they are on the device and computes the per-topic metrics there (kernels_reval.h).
// Replaces, per evaluated epoch, the reference's dump -> bin/query.py -> trec_eval round trip (product-search.sh:136-170).

struct sert_reval {
    sert_model* m = nullptr;       // borrowed; sert_reval_destroy does not touch it
    int device = -1;
    int64_t Q = 0, T = 0;
    int k = 0, kk = 0;
    // a counted handle (sert_reval_create_counted): no ranking is made; the judged entities' ranks are counted per slab of
    // kScoreRankRows topics in one reused (rows, V) cosine buffer
    bool counted = false, ranks_valid = false;
    int64_t R = 0;                 // judged entities uploaded, rel_indptr[Q]
    int64_t max_judged = 0;        // the longest judgement list
    int32_t* ranks = nullptr;      // (R) 1-based, aligned with rel_ent
    float* slab = nullptr;         // (min(Q, kScoreRankRows), V)
    // topics and judgements (device)
    int32_t* tokens = nullptr;
    int64_t* offsets = nullptr;
    int64_t* rel_indptr = nullptr;
    int32_t* rel_ent = nullptr;
    float* rel_gain = nullptr;
    double* log2tab = nullptr;     // [i] = log2(i + 1), i = 0 .. kk
    double* idcg = nullptr;
    int32_t* num_rel = nullptr;
    // results (device)
    double* metrics = nullptr;     // (Q, REVAL_NUM_METRICS)
    int32_t* status = nullptr;     // (Q)
    // vectorspace: mean word vectors, projections, the scorer on the live entity table, the ranking
    sert_scorer* sc = nullptr;
    float *avg = nullptr, *proj = nullptr, *val = nullptr;
    int32_t* idx = nullptr;
    // loglinear: the chunks of sert_ll_rank_queries with every chunk's inputs resident
    LLRankPlan plan;
    LLRankScratch w;
    uint32_t* ll_ids = nullptr;
    int32_t* ll_tok_row = nullptr;
    int64_t* ll_offs = nullptr;
    std::vector<int64_t> ids_at, tok_at, offs_at, distinct;   // per chunk: where its inputs start, its distinct tokens
};

// device copy of a host array (an empty one still gets an allocation: kernels take the pointer)
static int reval_upload_bytes(void** dst, const void* src, size_t bytes, hipStream_t s) {
    SERT_HIP(hipMalloc(dst, std::max<size_t>(bytes, 16)));
    if (bytes) SERT_HIP(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
}
#define reval_upload(dst, src, count, s) reval_upload_bytes((void**)(dst), (src), (size_t)(count) * sizeof(**(dst)), (s))

int sert_reval_destroy(sert_reval* r) {
    if (!r) return 0;
    if (r->device >= 0) {
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize();
    }
    for (void* p : {(void*)r->tokens, (void*)r->offsets, (void*)r->rel_indptr, (void*)r->rel_ent, (void*)r->rel_gain,
                    (void*)r->log2tab, (void*)r->idcg, (void*)r->num_rel, (void*)r->metrics, (void*)r->status, (void*)r->avg,
                    (void*)r->proj, (void*)r->val, (void*)r->idx, (void*)r->ranks, (void*)r->slab, (void*)r->ll_ids, (void*)r->ll_tok_row, (void*)r->ll_offs})
        (void)hipFree(p);
    sert_scorer_destroy(r->sc);
    delete r;      // (w frees the ranking scratch; its inputs are borrowed)
    return 0;
}

static int reval_create(sert_reval* r, sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t Q,
                        const int64_t* rel_indptr, const int32_t* rel_entities, const float* rel_gains,
                        const double* ideal_dcg, const int32_t* num_rel, int32_t k, bool counted) {
    const auto& c = m->cfg;
    const int V = c.num_entities;
    // ---- validation: nothing below may index outside an array on the device ----
    if (Q <= 0) SERT_FAIL("an evaluator needs at least one topic");
    if (Q > (int64_t)1 << 24) SERT_FAIL("more than 2^24 topics in one evaluator");     // (launch grids and GEMM rows are int)
    SERT_TRY(ll_rank_check_offsets(offsets, Q));     // (offsets[0] = 0, at least one token per topic)
    const int64_t T = offsets[Q];
    SERT_TRY(ll_rank_check_tokens(m, tokens, T));
    if (rel_indptr[0] != 0) SERT_FAIL("rel_indptr[0] must be 0");
    for (int64_t q = 0; q < Q; ++q) {
        if (rel_indptr[q + 1] < rel_indptr[q]) SERT_FAIL("rel_indptr must not decrease");
        for (int64_t i = rel_indptr[q]; i < rel_indptr[q + 1]; ++i) {
            if (rel_entities[i] < 0 || rel_entities[i] >= V) SERT_FAIL("judged entity out of range [0, num_entities)");
            if (i > rel_indptr[q] && rel_entities[i] <= rel_entities[i - 1])
                SERT_FAIL("judged entities must be strictly ascending inside a topic");
        }
        if (!(ideal_dcg[q] >= 0.0) || num_rel[q] < 0) SERT_FAIL("ideal DCG and the number of relevant entities must be >= 0");
    }
    if (counted) {
        if (!is_vs(m))
            SERT_FAIL("the counted evaluator is for the vectorspace kinds: a loglinear model ranks every entity through sert_reval_create");
        if (k == 0 || k < -1) SERT_FAIL("k must be -1 (every entity) or positive");
    } else if (is_vs(m)) {
        if (k < 1 || k > std::min<int>(V, kTopKMax))
            SERT_FAIL("the vectorspace evaluator ranks k in 1 .. min(num_entities, 1024) entities per topic");
    } else if (k == 0 || k < -1) {
        SERT_FAIL("k must be -1 (all entities) or positive");
    }
    SERT_HIP(hipSetDevice(c.device));
    hipStream_t s = m->stream;
    r->m = m; r->device = c.device; r->Q = Q; r->T = T; r->k = k;
    r->kk = (k < 0 || k >= V) ? V : k;
    const int kk = r->kk;
    const int64_t R = rel_indptr[Q];
    r->counted = counted; r->R = R;
    for (int64_t q = 0; q < Q; ++q) r->max_judged = std::max(r->max_judged, rel_indptr[q + 1] - rel_indptr[q]);
    SERT_TRY(reval_upload(&r->tokens, tokens, (size_t)T, s));
    SERT_TRY(reval_upload(&r->offsets, offsets, (size_t)Q + 1, s));
    SERT_TRY(reval_upload(&r->rel_indptr, rel_indptr, (size_t)Q + 1, s));
    SERT_TRY(reval_upload(&r->rel_ent, rel_entities, (size_t)R, s));
    SERT_TRY(reval_upload(&r->rel_gain, rel_gains, (size_t)R, s));
    SERT_TRY(reval_upload(&r->idcg, ideal_dcg, (size_t)Q, s));
    SERT_TRY(reval_upload(&r->num_rel, num_rel, (size_t)Q, s));
    std::vector<double> tab((size_t)kk + 1);
    for (int i = 0; i <= kk; ++i) tab[i] = log2((double)i + 1.0);
    SERT_TRY(reval_upload(&r->log2tab, tab.data(), tab.size(), s));
    SERT_TRY(dmalloc(&r->metrics, (size_t)Q * REVAL_NUM_METRICS));
    SERT_TRY(dzalloc(&r->status, (size_t)Q, s));
    if (counted) {
        // nothing here grows with the depth (log2tab above does)
        SERT_TRY(dmalloc(&r->avg, (size_t)Q * c.word_dim));
        SERT_TRY(dmalloc(&r->proj, (size_t)Q * c.entity_dim));
        SERT_TRY(dmalloc(&r->ranks, (size_t)std::max<int64_t>(R, 4)));
        SERT_TRY(dmalloc(&r->slab, (size_t)std::min<int64_t>(Q, kScoreRankRows) * V));
        SERT_TRY(scorer_alloc(c.device, V, c.entity_dim, &r->sc));
    } else if (is_vs(m)) {
        SERT_TRY(dmalloc(&r->avg, (size_t)Q * c.word_dim));
        SERT_TRY(dmalloc(&r->proj, (size_t)Q * c.entity_dim));
        SERT_TRY(dmalloc(&r->idx, (size_t)Q * kk));
        SERT_TRY(dmalloc(&r->val, (size_t)Q * kk));
        SERT_TRY(scorer_alloc(c.device, V, c.entity_dim, &r->sc));
    } else {
        ll_rank_plan(m, tokens, offsets, Q, k, r->plan);
        r->w.own_inputs = false;
        SERT_TRY(ll_rank_alloc(r->w, r->plan.mode, r->plan.max_rows, r->plan.max_tokens, r->plan.max_queries, V, c.word_dim, kk));
        // every chunk's inputs, back to back
        std::vector<int32_t> row_of(c.vocab_size, -1);
        std::vector<uint32_t> ids, all_ids;
        std::vector<int32_t> tok_row, all_tok_row;
        std::vector<int64_t> offs, all_offs;
        for (size_t ci = 0; ci + 1 < r->plan.bounds.size(); ++ci) {
            const int64_t Dc = ll_rank_chunk_inputs(tokens, offsets, r->plan.bounds[ci], r->plan.bounds[ci + 1], row_of, ids, tok_row, offs);
            r->ids_at.push_back((int64_t)all_ids.size());
            r->tok_at.push_back((int64_t)all_tok_row.size());
            r->offs_at.push_back((int64_t)all_offs.size());
            r->distinct.push_back(Dc);
            all_ids.insert(all_ids.end(), ids.begin(), ids.end());
            all_tok_row.insert(all_tok_row.end(), tok_row.begin(), tok_row.end());
            all_offs.insert(all_offs.end(), offs.begin(), offs.end());
        }
        r->ids_at.push_back((int64_t)all_ids.size());
        SERT_TRY(reval_upload(&r->ll_ids, all_ids.data(), all_ids.size(), s));
        SERT_TRY(reval_upload(&r->ll_tok_row, all_tok_row.data(), all_tok_row.size(), s));
        SERT_TRY(reval_upload(&r->ll_offs, all_offs.data(), all_offs.size(), s));
    }
    SERT_HIP(hipStreamSynchronize(s));      // (the host arrays are borrowed for the call only)
    return 0;
}

static int reval_create_any(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_topics,
                            const int64_t* rel_indptr, const int32_t* rel_entities, const float* rel_gains,
                            const double* ideal_dcg, const int32_t* num_rel, int32_t k, bool counted, sert_reval** out) {
    if (!m || !tokens || !offsets || !rel_indptr || !ideal_dcg || !num_rel || !out) SERT_FAIL("null argument");
    if (num_topics > 0 && rel_indptr[num_topics] > 0 && (!rel_entities || !rel_gains)) SERT_FAIL("null argument");
    *out = nullptr;
    sert_reval* r = new sert_reval();
    const int rc = reval_create(r, m, tokens, offsets, num_topics, rel_indptr, rel_entities, rel_gains, ideal_dcg, num_rel, k, counted);
    if (rc != 0) {
        const std::string keep = g_last_error;
        sert_reval_destroy(r);
        g_last_error = keep;
        return rc;
    }
    *out = r;
    return 0;
}

int sert_reval_create(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_topics,
                      const int64_t* rel_indptr, const int32_t* rel_entities, const float* rel_gains,
                      const double* ideal_dcg, const int32_t* num_rel, int32_t k, sert_reval** out) {
    return reval_create_any(m, tokens, offsets, num_topics, rel_indptr, rel_entities, rel_gains, ideal_dcg, num_rel, k, false, out);
}

int sert_reval_create_counted(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_topics,
                              const int64_t* rel_indptr, const int32_t* rel_entities, const float* rel_gains,
                              const double* ideal_dcg, const int32_t* num_rel, int32_t k, sert_reval** out) {
    return reval_create_any(m, tokens, offsets, num_topics, rel_indptr, rel_entities, rel_gains, ideal_dcg, num_rel, k, true, out);
}

// reval_count_ranks on `rows` cosine rows S (rows, V) of the topics q0 .. q0 + rows, into ranks[] (zero on entry for those
// topics).  max_judged: the longest judgement list among them, or a bound on it -- it picks the tile (8 judged entities in
// registers for the usual handful, 32 beyond).  The row is cut into pieces so that a launch of few rows still fills the
// device, each piece at least 4096 columns.
static void reval_launch_count(hipStream_t s, const float* S, int rows, int64_t V, int64_t q0, const int64_t* rel_indptr,
                               const int32_t* rel_ent, int32_t* ranks, int64_t max_judged) {
    const int splits = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(2048, rows), V / 4096));
    const dim3 grid((unsigned)rows, (unsigned)splits);
    const bool vec = V % 4 == 0;
    if (max_judged <= 8) {
        if (vec) launch((reval_count_ranks<8, true>), grid, dim3(256), 0, s, S, (int)V, q0, rel_indptr, rel_ent, ranks);
        else launch((reval_count_ranks<8, false>), grid, dim3(256), 0, s, S, (int)V, q0, rel_indptr, rel_ent, ranks);
    } else {
        if (vec) launch((reval_count_ranks<32, true>), grid, dim3(256), 0, s, S, (int)V, q0, rel_indptr, rel_ent, ranks);
        else launch((reval_count_ranks<32, false>), grid, dim3(256), 0, s, S, (int)V, q0, rel_indptr, rel_ent, ranks);
    }
}

static void reval_launch_metrics(sert_reval* r, hipStream_t s, const int32_t* idx, int Qc, int64_t q0) {
    launch(reval_metrics, dim3(cdiv(Qc, 4)), dim3(256), 0, s, idx, r->kk, Qc, q0, r->rel_indptr, r->rel_ent,
           r->rel_gain, r->log2tab, r->idcg, r->num_rel, r->metrics);
}

int sert_reval_run(sert_reval* r, double* metrics_out, int32_t* status_out, int32_t* idx_out, float* score_out) {
    refresh_gemm_choice();
    if (!r || !metrics_out || !status_out) SERT_FAIL("null argument");
    if ((idx_out == nullptr) != (score_out == nullptr)) SERT_FAIL("idx_out and score_out go together");
    if (r->counted && idx_out)
        SERT_FAIL("a counted evaluator makes no ranking (idx_out and score_out must be NULL): sert_scorer_rank returns one");
    sert_model* m = r->m;
    const auto& c = m->cfg;
    SERT_HIP(hipSetDevice(c.device));
    // the parameters as a reader must see them (sert_get_tensor): the whole word table here (data parallel: COLLECTIVE), every
    // lazily updated row brought to the model's step, the entity table's and the dense tail's updates landed.  A batch that
    // runs ahead (sert_hint_next_batch) reads parameters and writes activations and gradient scratch only; nothing here
    // touches those, so it stays valid.
    SERT_TRY(ensure_full_rw(m));
    SERT_TRY(ensure_rw_current(m, -1));
    if (m->comm_stream) SERT_HIP(hipStreamSynchronize(m->comm_stream));
    if (m->stream2) SERT_HIP(hipStreamSynchronize(m->stream2));
    SERT_TRY(settle_entity_update(m));
    hipStream_t s = m->stream;
    const int64_t Q = r->Q;
    const int kk = r->kk;
    if (r->counted) {
        const int dw = c.word_dim, de = c.entity_dim;
        const int64_t V = c.num_entities;
        r->ranks_valid = false;
        if (dw % 4 == 0)
            launch(reval_gather_mean<4>, dim3(cdiv(Q, 4)), dim3(256), 0, s, r->tokens, r->offsets, m->rw, (int)Q, dw, r->avg);
        else
            launch(reval_gather_mean<1>, dim3(cdiv(Q, 4)), dim3(256), 0, s, r->tokens, r->offsets, m->rw, (int)Q, dw, r->avg);
        launch_gemm<false, false, EPI_BIAS_TANH>(s, r->avg, m->W, r->proj, m->b, (int)Q, de, dw, dw, de, de);
        SERT_TRY(scorer_load_table(r->sc, m->re, hipMemcpyDeviceToDevice, s));
        launch(l2_normalize_rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, r->proj, Q, de);     // (as sert_scorer_rank normalises its copy)
        if (r->R) SERT_HIP(hipMemsetAsync(r->ranks, 0, (size_t)r->R * sizeof(int32_t), s));
        // sert_scorer_rank's slab call, in launches of at most kScoreRankRows rows (a row's cosines do not depend on the
        // rows launched with it): a judged entity's rank is its position in that call's ranking.  Everything on the model's
        // stream: the slab buffer is reused from slab to slab in stream order.
        for (int64_t q0 = 0; q0 < Q; q0 += kScoreRankRows) {
            const int qn = (int)std::min<int64_t>(kScoreRankRows, Q - q0);
            scorer_cosine_slab(r->sc, s, r->proj + q0 * de, qn, r->slab, r->sc->bf16);
            reval_launch_count(s, r->slab, qn, V, q0, r->rel_indptr, r->rel_ent, r->ranks, r->max_judged);
            launch(reval_metrics_from_ranks, dim3(cdiv(qn, 4)), dim3(256), 0, s, r->ranks, kk, qn, q0, r->rel_indptr,
                   r->rel_gain, r->log2tab, r->idcg, r->num_rel, r->metrics);
        }
        SERT_HIP(hipGetLastError());
    } else if (is_vs(m)) {
        const int dw = c.word_dim, de = c.entity_dim;
        if (dw % 4 == 0)
            launch(reval_gather_mean<4>, dim3(cdiv(Q, 4)), dim3(256), 0, s, r->tokens, r->offsets, m->rw, (int)Q, dw, r->avg);
        else
            launch(reval_gather_mean<1>, dim3(cdiv(Q, 4)), dim3(256), 0, s, r->tokens, r->offsets, m->rw, (int)Q, dw, r->avg);
        // sert_predict_project's launch on the resident block
        launch_gemm<false, false, EPI_BIAS_TANH>(s, r->avg, m->W, r->proj, m->b, (int)Q, de, dw, dw, de, de);
        SERT_TRY(scorer_load_table(r->sc, m->re, hipMemcpyDeviceToDevice, s));
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipStreamSynchronize(s));          // (the scorer works on streams of its own)
        SERT_TRY(scorer_topk_io(r->sc, r->proj, Q, kk, r->idx, r->val, /*dev=*/true));
        reval_launch_metrics(r, s, r->idx, (int)Q, 0);
        SERT_HIP(hipGetLastError());
        if (idx_out) {
            SERT_HIP(hipMemcpyAsync(idx_out, r->idx, (size_t)Q * kk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipMemcpyAsync(score_out, r->val, (size_t)Q * kk * sizeof(float), hipMemcpyDeviceToHost, s));
        }
    } else {
        SERT_HIP(hipStreamSynchronize(s));
        LLRankScratch& w = r->w;
        for (size_t ci = 0; ci + 1 < r->plan.bounds.size(); ++ci) {
            const int64_t a = r->plan.bounds[ci], Qc = r->plan.bounds[ci + 1] - a;
            w.ids = r->ll_ids + r->ids_at[ci];
            w.tok_row = r->ll_tok_row + r->tok_at[ci];
            w.offs = r->ll_offs + r->offs_at[ci];
            SERT_TRY(ll_rank_chunk_device(m, s, w, r->distinct[ci], r->ids_at[ci + 1] - r->ids_at[ci], (int)Qc, kk, r->plan.mode));
            reval_launch_metrics(r, s, w.idx, (int)Qc, a);
            SERT_HIP(hipGetLastError());
            SERT_HIP(hipMemcpyAsync(r->status + a, w.status, (size_t)Qc * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            if (idx_out) {
                SERT_HIP(hipMemcpyAsync(idx_out + a * kk, w.idx, (size_t)Qc * kk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                SERT_HIP(hipMemcpyAsync(score_out + a * kk, w.val, (size_t)Qc * kk * sizeof(float), hipMemcpyDeviceToHost, s));
            }
        }
    }
    SERT_HIP(hipMemcpyAsync(metrics_out, r->metrics, (size_t)Q * REVAL_NUM_METRICS * sizeof(double), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipMemcpyAsync(status_out, r->status, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipStreamSynchronize(s));
    r->ranks_valid = r->counted;
    return 0;
}

int sert_reval_judged_ranks(sert_reval* r, int32_t* ranks_out) {
    if (!r) SERT_FAIL("null argument");
    if (!r->counted) SERT_FAIL("not a counted evaluator (sert_reval_create_counted): it holds rankings, not ranks");
    if (!r->ranks_valid) SERT_FAIL("no sert_reval_run of this evaluator has completed");
    if (r->R == 0) return 0;
    if (!ranks_out) SERT_FAIL("null argument");
    SERT_HIP(hipSetDevice(r->device));
    SERT_HIP(hipMemcpyAsync(ranks_out, r->ranks, (size_t)r->R * sizeof(int32_t), hipMemcpyDeviceToHost, r->m->stream));
    SERT_HIP(hipStreamSynchronize(r->m->stream));
    return 0;
}

// Test hook (include/sert_hip_debug.h): reval_count_ranks alone on a caller's cosine matrix
int sert_debug_count_ranks(int device, const float* cos, int64_t Q, int64_t V, const int64_t* rel_indptr, const int32_t* rel_ent,
                           int32_t* ranks_out) {
    if (!cos || !rel_indptr || Q <= 0 || V <= 0) SERT_FAIL("bad argument");
    if (Q > 65535 || V > ((int64_t)1 << 30) || Q * V > ((int64_t)1 << 31)) SERT_FAIL("matrix too large for the test hook");
    if (rel_indptr[0] != 0) SERT_FAIL("rel_indptr[0] must be 0");
    int64_t max_judged = 0;
    for (int64_t q = 0; q < Q; ++q) {
        if (rel_indptr[q + 1] < rel_indptr[q]) SERT_FAIL("rel_indptr must not decrease");
        max_judged = std::max(max_judged, rel_indptr[q + 1] - rel_indptr[q]);
    }
    const int64_t R = rel_indptr[Q];
    if (R == 0) return 0;
    if (!rel_ent || !ranks_out) SERT_FAIL("bad argument");
    for (int64_t i = 0; i < R; ++i)
        if (rel_ent[i] < 0 || rel_ent[i] >= V) SERT_FAIL("judged entity out of range [0, V)");
    SERT_HIP(hipSetDevice(device));
    float* dS = nullptr; int64_t* dptr = nullptr; int32_t* dent = nullptr; int32_t* dranks = nullptr;
    auto body = [&]() -> int {
        SERT_TRY(dmalloc(&dS, (size_t)(Q * V)));
        SERT_TRY(dmalloc(&dptr, (size_t)Q + 1));
        SERT_TRY(dmalloc(&dent, (size_t)R));
        SERT_TRY(dmalloc(&dranks, (size_t)R));
        SERT_HIP(hipMemcpy(dS, cos, (size_t)(Q * V) * sizeof(float), hipMemcpyHostToDevice));
        SERT_HIP(hipMemcpy(dptr, rel_indptr, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        SERT_HIP(hipMemcpy(dent, rel_ent, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice));
        SERT_HIP(hipMemset(dranks, 0, (size_t)R * sizeof(int32_t)));
        reval_launch_count(0, dS, (int)Q, V, 0, dptr, dent, dranks, max_judged);
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipDeviceSynchronize());
        SERT_HIP(hipMemcpy(ranks_out, dranks, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = body();
    (void)hipFree(dS); (void)hipFree(dptr); (void)hipFree(dent); (void)hipFree(dranks);
    return rc;
}

// Test hook (include/sert_hip_debug.h)
int sert_debug_reval_chunks(sert_reval* r) {
    if (!r) return -1;
    return r->plan.bounds.empty() ? 1 : (int)r->plan.bounds.size() - 1;     // (no plan: a vectorspace kind)
}
