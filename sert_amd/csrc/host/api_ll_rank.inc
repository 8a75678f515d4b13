// Batched loglinear query ranking (include/sert_hip.h: sert_ll_rank_queries; include/sert_hip_debug.h:
// sert_debug_ll_rank_distributions).  Replaces, for all queries of a call at once, the reference's
// WordBatcher -> predict_fn -> LogLinearCallback.process chain (sert/inference.py:28-143, :170-174;
// bin/query.py:199-236): the per-token distributions stay on the device (kernels_ll_rank.h).

// Logits GEMM in slabs of this many rows: every launch has the shape (kLLRankRows, V_e, d_w), whatever the number of
// queries or distinct tokens, so launch_gemm picks the same kernel and tiling for every slab -- a token's distribution
// (and so a query's ranking) does not depend on the other queries of the call or on the chunking.
static const int kLLRankRows = 1024;

// SERT_LL_RANK_BUDGET: device bytes one chunk of a call may use (distributions, gathered rows, joint rows, sort scratch)
static size_t ll_rank_budget() {
    const char* e = knob("SERT_LL_RANK_BUDGET");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)2 << 30);
}

// which kernels rank the joint rows: topk_rows for a proper prefix of up to kTopKMax, a full ranking otherwise (host/rank_rows.inc)
static int ll_rank_mode(int V, int kk) {
    if (kk <= kTopKMax && kk < V) return RANK_TOPK;
    return V <= kRankLdsMax ? RANK_LDS : RANK_CSORT;
}

// device scratch of one call, sized for its largest chunk
struct LLRankScratch {
    uint32_t* ids = nullptr;       // distinct token ids of the chunk (padded to whole slabs with id 0)
    int32_t* tok_row = nullptr;    // row of every token of the chunk
    int64_t* offs = nullptr;       // chunk-relative query offsets
    float *G = nullptr, *P = nullptr, *J = nullptr, *tok_h = nullptr, *joint_h = nullptr, *val = nullptr;
    int32_t *status = nullptr, *idx = nullptr;
    RankSortScratch sort;          // the LSD passes' (kernels_rank.h)
    bool own_inputs = true;        // false: ids / tok_row / offs point into arrays somebody else owns (sert_reval: uploaded once)
    ~LLRankScratch() {
        if (!own_inputs) ids = nullptr, tok_row = nullptr, offs = nullptr;
        for (void* p : {(void*)ids, (void*)tok_row, (void*)offs, (void*)G, (void*)P, (void*)J, (void*)tok_h, (void*)joint_h,
                        (void*)val, (void*)status, (void*)idx})
            (void)hipFree(p);
        rank_scratch_free(sort);
    }
};

static int ll_rank_alloc(LLRankScratch& w, int mode, int64_t rows, int64_t T, int64_t Qc, int V, int d, int kk) {
    if (w.own_inputs) {
        SERT_TRY(dmalloc(&w.ids, (size_t)rows));
        SERT_TRY(dmalloc(&w.tok_row, (size_t)T));
        SERT_TRY(dmalloc(&w.offs, (size_t)Qc + 1));
    }
    if (d > 0) SERT_TRY(dmalloc(&w.G, (size_t)rows * d));
    if (d > 0) SERT_TRY(dmalloc(&w.P, (size_t)rows * V));
    SERT_TRY(dmalloc(&w.J, (size_t)Qc * V));
    SERT_TRY(dmalloc(&w.tok_h, (size_t)rows));
    SERT_TRY(dmalloc(&w.joint_h, (size_t)Qc));
    SERT_TRY(dmalloc(&w.status, (size_t)Qc));
    SERT_TRY(dmalloc(&w.idx, (size_t)Qc * kk));
    SERT_TRY(dmalloc(&w.val, (size_t)Qc * kk));
    if (mode == RANK_CSORT) SERT_TRY(rank_scratch_reserve(w.sort, (int64_t)Qc * V));
    return 0;
}

// the two float32 constants of math_utils.entropy(..., base=2, normalize=True): float(log(2)), float(log(V) / log(2))
static float ll_ln2_f() { return (float)log(2.0); }
static float ll_log2v_f(int V) { return (float)(log((double)V) / log(2.0)); }

// P holds the chunk's per-token distributions (rows indexed by w.tok_row), w.offs its Qc + 1 query offsets: joint rows,
// joint entropies and status on stream s (ll_rank_aggregate: all sert_ll_rank_candidates takes, host/api_ll_rerank.inc), then
// the ranking of the whole rows (w.idx / w.val, Qc x kk)
static void ll_rank_aggregate(hipStream_t s, LLRankScratch& w, const float* P, int Qc, int V) {
    launch(ll_query_aggregate, dim3(Qc), dim3(256), 0, s, P, w.tok_row, w.offs, V, ll_ln2_f(), ll_log2v_f(V),
           w.J, w.joint_h, w.status);
}
static int ll_rank_chunk(hipStream_t s, LLRankScratch& w, const float* P, int Qc, int V, int kk, int mode) {
    ll_rank_aggregate(s, w, P, Qc, V);
    if (mode == RANK_TOPK) {
        launch(topk_rows<true>, dim3(Qc), dim3(256), 0, s, w.J, V, kk, w.idx, w.val, (float*)nullptr);
        SERT_HIP(hipGetLastError());
        return 0;
    }
    return rank_rows_full(s, mode, /*raw=*/true, w.J, Qc, V, kk, w.sort, w.idx, w.val);
}

static int ll_rank_copy_out(hipStream_t s, LLRankScratch& w, int64_t q0, int Qc, int kk, int32_t* idx_out, float* score_out,
                            float* joint_entropy_out, int32_t* status_out) {
    SERT_HIP(hipMemcpyAsync(idx_out + q0 * kk, w.idx, (size_t)Qc * kk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipMemcpyAsync(score_out + q0 * kk, w.val, (size_t)Qc * kk * sizeof(float), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipMemcpyAsync(joint_entropy_out + q0, w.joint_h, (size_t)Qc * sizeof(float), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipMemcpyAsync(status_out + q0, w.status, (size_t)Qc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return 0;
}

static int ll_rank_check_offsets(const int64_t* offsets, int64_t Q) {
    if (offsets[0] != 0) SERT_FAIL("offsets[0] must be 0");
    for (int64_t q = 0; q < Q; ++q)
        if (offsets[q + 1] <= offsets[q]) SERT_FAIL("every query needs at least one token (offsets must increase)");
    return 0;
}

// How a call's queries are cut into chunks: consecutive queries while distinct rows x V_e + joint rows + sort scratch fit
// the budget and, for the LSD passes, one sorted chunk (rank_chunk_fits).  bounds[c] .. bounds[c + 1] are the queries of chunk c; max_* size the scratch for the largest chunk.
struct LLRankPlan {
    std::vector<int64_t> bounds;
    int64_t max_rows = 0, max_tokens = 0, max_queries = 0;
    int kk = 0, mode = 0;
};

static int ll_rank_check_tokens(const sert_model* m, const int32_t* tokens, int64_t T) {
    for (int64_t t = 0; t < T; ++t)
        if (tokens[t] < 0 || tokens[t] >= m->cfg.vocab_size) SERT_FAIL("token id out of range [0, vocab_size)");
    return 0;
}

// The cut itself: a chunk takes the next query q while over(q0, q, D) is false -- q0 the chunk's first query, D its distinct
// tokens with q's -- and its first query always.  Fills bounds and the max_* of plan.
static void ll_rank_cut(const sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_queries,
                        const std::function<bool(int64_t, int64_t, int64_t)>& over, LLRankPlan& plan) {
    const int64_t T = offsets[num_queries];
    std::vector<int64_t>& bounds = plan.bounds;
    bounds.assign(1, 0);
    std::vector<int64_t> chunk_of(m->cfg.vocab_size, -1);
    std::vector<int32_t> qtok;
    int64_t D = 0, q0 = 0, maxD = 0, maxT = 0, maxQ = 0;
    for (int64_t q = 0; q < num_queries; ++q) {
        qtok.assign(tokens + offsets[q], tokens + offsets[q + 1]);
        std::sort(qtok.begin(), qtok.end());
        qtok.erase(std::unique(qtok.begin(), qtok.end()), qtok.end());
        const int64_t chunk = (int64_t)bounds.size() - 1;
        int64_t fresh = 0;
        for (int32_t w : qtok) fresh += chunk_of[w] != chunk;
        if (q > q0 && over(q0, q, D + fresh)) {
            maxD = std::max(maxD, D); maxQ = std::max(maxQ, q - q0); maxT = std::max(maxT, offsets[q] - offsets[q0]);
            bounds.push_back(q);
            q0 = q; D = 0;
            fresh = (int64_t)qtok.size();
        }
        const int64_t cur = (int64_t)bounds.size() - 1;
        for (int32_t w : qtok) chunk_of[w] = cur;
        D += fresh;
    }
    maxD = std::max(maxD, D); maxQ = std::max(maxQ, num_queries - q0); maxT = std::max(maxT, T - offsets[q0]);
    bounds.push_back(num_queries);
    plan.max_rows = (int64_t)cdiv(maxD, kLLRankRows) * kLLRankRows;
    plan.max_tokens = maxT;
    plan.max_queries = maxQ;
}

// bytes of the chain in front of the ranking for D distinct tokens: gathered rows, distributions, token entropies (and ids)
static size_t ll_rank_front_bytes(int64_t D, int d, int V) {
    return (size_t)cdiv(D, kLLRankRows) * kLLRankRows * ((size_t)d + V + 2) * 4;
}

static void ll_rank_plan(const sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_queries, int32_t k,
                         LLRankPlan& plan) {
    const auto& c = m->cfg;
    const int V = c.num_entities, d = c.word_dim;
    const int kk = (k < 0 || k >= V) ? V : k;
    const int mode = ll_rank_mode(V, kk);
    plan.kk = kk; plan.mode = mode;
    const size_t budget = ll_rank_budget();
    auto bytes = [&](int64_t D, int64_t Qc) -> size_t {
        // (the sort scratch without the 8 KiB of its bin totals: they have never been counted, and counting them would move
        //  the chunk bounds of a given budget)
        const size_t sort = mode == RANK_CSORT ? rank_scratch_bytes(Qc * (int64_t)V) - (size_t)kSortMaxBins * 4 : 0;
        return ll_rank_front_bytes(D, d, V) + (size_t)Qc * ((size_t)V * 4 + (size_t)kk * 8) + sort;
    };
    ll_rank_cut(m, tokens, offsets, num_queries, [&](int64_t q0, int64_t q, int64_t D) {
        return (mode == RANK_CSORT && !rank_chunk_fits(q - q0 + 1, V)) || bytes(D, q - q0 + 1) > budget;
    }, plan);
}

// the device inputs of one chunk (queries a .. b): its distinct token ids in order of first appearance, padded to whole
// slabs with id 0 (computed and never read); the row of every token; chunk-relative query offsets.  Returns the number of
// distinct tokens.  row_of: vocab_size entries, all -1 on entry and on return.
static int64_t ll_rank_chunk_inputs(const int32_t* tokens, const int64_t* offsets, int64_t a, int64_t b, std::vector<int32_t>& row_of,
                                    std::vector<uint32_t>& ids, std::vector<int32_t>& tok_row, std::vector<int64_t>& offs) {
    const int64_t Qc = b - a, t0 = offsets[a], Tc = offsets[b] - t0;
    ids.clear(); tok_row.resize(Tc); offs.resize(Qc + 1);
    for (int64_t t = 0; t < Tc; ++t) {
        const int32_t tok = tokens[t0 + t];
        if (row_of[tok] < 0) { row_of[tok] = (int32_t)ids.size(); ids.push_back((uint32_t)tok); }
        tok_row[t] = row_of[tok];
    }
    for (uint32_t id : ids) row_of[id] = -1;
    for (int64_t q = 0; q <= Qc; ++q) offs[q] = offsets[a + q] - t0;
    const int64_t Dc = (int64_t)ids.size();
    ids.resize((size_t)cdiv(Dc, kLLRankRows) * kLLRankRows, 0u);
    return Dc;
}

// The distributions of one chunk, inputs in w.ids / w.tok_row / w.offs: the predict_fn chain of sert_predict_tokens on the Dc
// distinct tokens (`rows` with the padding) into w.P, and their entropies
static void ll_rank_chunk_distributions(sert_model* m, hipStream_t s, LLRankScratch& w, int64_t Dc, int64_t rows) {
    const int V = m->cfg.num_entities, d = m->cfg.word_dim;
    gather_rows(s, w.ids, m->rw, w.G, rows, d);
    for (int64_t r0 = 0; r0 < rows; r0 += kLLRankRows)
        launch_gemm<false, false, EPI_BIAS>(s, w.G + (size_t)r0 * d, m->W, w.P + (size_t)r0 * V, m->b, kLLRankRows, V, d, d, V, V);
    launch(ll_softmax_rows, dim3(cdiv(Dc, 4)), dim3(256), 0, s, w.P, Dc, V);
    launch(ll_row_entropy, dim3((unsigned)Dc), dim3(256), 0, s, w.P, V, ll_ln2_f(), ll_log2v_f(V), w.tok_h);
}
// One chunk on the device: its distributions, then ll_rank_chunk.  sert_ll_rank_queries and sert_reval_run rank through here,
// and sert_ll_rank_candidates takes its joint rows from the same two steps (ll_rank_chunk_distributions, ll_rank_aggregate), so
// a query's scores do not depend on the caller.
static int ll_rank_chunk_device(sert_model* m, hipStream_t s, LLRankScratch& w, int64_t Dc, int64_t rows, int Qc, int kk, int mode) {
    ll_rank_chunk_distributions(m, s, w, Dc, rows);
    return ll_rank_chunk(s, w, w.P, Qc, m->cfg.num_entities, kk, mode);
}

int sert_ll_rank_queries(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_queries, int32_t k,
                         int32_t* idx_out, float* score_out, float* joint_entropy_out, float* token_entropy_out,
                         int32_t* status_out) {
    refresh_gemm_choice();
    if (!m || !tokens || !offsets || !idx_out || !score_out || !joint_entropy_out || !token_entropy_out || !status_out)
        SERT_FAIL("null argument");
    if (is_vs(m)) SERT_FAIL("sert_ll_rank_queries ranks with the loglinear model");
    if (k == 0 || k < -1) SERT_FAIL("k must be -1 (all entities) or positive");
    if (num_queries <= 0) return 0;
    SERT_TRY(ll_rank_check_offsets(offsets, num_queries));
    const auto& c = m->cfg;
    const int V = c.num_entities, d = c.word_dim;
    SERT_TRY(ll_rank_check_tokens(m, tokens, offsets[num_queries]));
    SERT_HIP(hipSetDevice(c.device));
    SERT_TRY(ensure_full_rw(m));
    SERT_TRY(ensure_rw_current(m, -1));
    LLRankPlan plan;
    ll_rank_plan(m, tokens, offsets, num_queries, k, plan);
    const int kk = plan.kk, mode = plan.mode;

    hipStream_t s = m->stream;
    SERT_HIP(hipStreamSynchronize(s));
    LLRankScratch w;
    SERT_TRY(ll_rank_alloc(w, mode, plan.max_rows, plan.max_tokens, plan.max_queries, V, d, kk));

    std::vector<int32_t> row_of(c.vocab_size, -1);
    std::vector<uint32_t> ids;
    std::vector<int32_t> tok_row;
    std::vector<int64_t> offs;
    std::vector<float> tok_h;
    for (size_t ci = 0; ci + 1 < plan.bounds.size(); ++ci) {
        const int64_t a = plan.bounds[ci], b = plan.bounds[ci + 1], Qc = b - a, t0 = offsets[a], Tc = offsets[b] - t0;
        const int64_t Dc = ll_rank_chunk_inputs(tokens, offsets, a, b, row_of, ids, tok_row, offs);
        const int64_t rows = (int64_t)ids.size();
        SERT_HIP(hipMemcpyAsync(w.ids, ids.data(), rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemcpyAsync(w.tok_row, tok_row.data(), Tc * sizeof(int32_t), hipMemcpyHostToDevice, s));
        SERT_HIP(hipMemcpyAsync(w.offs, offs.data(), (Qc + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        SERT_TRY(ll_rank_chunk_device(m, s, w, Dc, rows, (int)Qc, kk, mode));
        SERT_TRY(ll_rank_copy_out(s, w, a, (int)Qc, kk, idx_out, score_out, joint_entropy_out, status_out));
        tok_h.resize(Dc);
        SERT_HIP(hipMemcpyAsync(tok_h.data(), w.tok_h, Dc * sizeof(float), hipMemcpyDeviceToHost, s));
        SERT_HIP(hipStreamSynchronize(s));
        for (int64_t t = 0; t < Tc; ++t) token_entropy_out[t0 + t] = tok_h[tok_row[t]];
    }
    return 0;
}

// Test hook: the aggregate and ranking kernels of sert_ll_rank_queries on per-token distributions the caller provides.
int sert_debug_ll_rank_distributions(int device, const float* P, const int64_t* offsets, int64_t num_queries, int32_t V,
                                     int32_t k, int32_t* idx_out, float* score_out, float* joint_entropy_out,
                                     float* token_entropy_out, int32_t* status_out) {
    if (!P || !offsets || !idx_out || !score_out || !joint_entropy_out || !token_entropy_out || !status_out || V <= 0 ||
        k == 0 || k < -1)
        SERT_FAIL("bad argument");
    if (num_queries <= 0) return 0;
    SERT_TRY(ll_rank_check_offsets(offsets, num_queries));
    const int64_t T = offsets[num_queries];
    const int kk = (k < 0 || k >= V) ? V : k;
    const int mode = ll_rank_mode(V, kk);
    if (mode == RANK_CSORT && !rank_chunk_fits(num_queries, V))
        SERT_FAIL("too many queries x entities for one sorted chunk");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int rc = 0;
    {
        LLRankScratch w;
        float* dP = nullptr;
        auto body = [&]() -> int {
            SERT_TRY(ll_rank_alloc(w, mode, T, T, num_queries, V, 0, kk));
            SERT_TRY(dmalloc(&dP, (size_t)T * V));
            std::vector<int32_t> rows(T);
            for (int64_t t = 0; t < T; ++t) rows[t] = (int32_t)t;
            SERT_HIP(hipMemcpyAsync(dP, P, (size_t)T * V * sizeof(float), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.tok_row, rows.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.offs, offsets, (num_queries + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
            launch(ll_row_entropy, dim3((unsigned)T), dim3(256), 0, s, dP, V, ll_ln2_f(), ll_log2v_f(V), w.tok_h);
            SERT_TRY(ll_rank_chunk(s, w, dP, (int)num_queries, V, kk, mode));
            SERT_TRY(ll_rank_copy_out(s, w, 0, (int)num_queries, kk, idx_out, score_out, joint_entropy_out, status_out));
            SERT_HIP(hipMemcpyAsync(token_entropy_out, w.tok_h, T * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipStreamSynchronize(s));
            return 0;
        };
        rc = body();
        (void)hipStreamSynchronize(s);
        (void)hipFree(dP);
    }
    (void)hipStreamDestroy(s);
    return rc;
}
