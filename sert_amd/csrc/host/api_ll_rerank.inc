// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block, behind api_ll_rank.inc and
// api_scorer_rerank.inc): C ABI: per-query candidate lists ranked with the loglinear model (include/sert_hip.h:
// sert_ll_rank_candidates; include/sert_hip_debug.h: sert_debug_ll_rank_candidates_distributions, sert_debug_ll_rerank_counts).
// Kernels: csrc/kernels_ll_rerank.h.  The joint rows come from the chain of sert_ll_rank_queries (api_ll_rank.inc:
// ll_rank_chunk_inputs, ll_rank_chunk_distributions, ll_rank_aggregate) -- the scores stay normalised over all entities --
// and only the listed entries of a row are sorted and copied out: no Qc x V_e sort scratch, no (Qc, V_e) outputs.

// What the candidate calls of this PROCESS did (sert_debug_ll_rerank_counts): [0] calls that passed their argument checks,
// [1] their chunks, lists ranked by [2] the LDS kernel, [3] the slab and the counting-sort passes, [4] empty lists.
// Process-wide, not per model: the debug call has no model, and one scope serves both (a test takes differences).
static std::atomic<int64_t> g_ll_rerank_counts[5];

// device scratch behind the joint rows, sized for the largest chunk of a call
struct LLRerankScratch {
    int64_t* cptr = nullptr;        // chunk-relative cand_indptr (Qc + 1), then the chunk-relative output offsets (Qc + 1)
    int32_t *ents = nullptr, *qlist = nullptr, *idx = nullptr, *pos = nullptr;
    float *val = nullptr, *slab = nullptr, *pval = nullptr;
    RankSortScratch sort;
    ~LLRerankScratch() {
        for (void* p : {(void*)cptr, (void*)ents, (void*)qlist, (void*)idx, (void*)pos, (void*)val, (void*)slab, (void*)pval})
            (void)hipFree(p);
        rank_scratch_free(sort);
    }
};

// what of a chunk sizes the scratch: candidates, ranked entries, and the slab of its lists beyond LDS (rows x the longest)
struct LLRerankShape {
    int64_t pairs = 0, outs = 0, rows = 0, lmax = 0;
    int64_t kkc(int32_t k) const { return k < 0 ? lmax : std::min<int64_t>(k, lmax); }
    size_t bytes(int32_t k) const {
        size_t b = (size_t)pairs * 4 + (size_t)outs * 8;
        if (rows) b += (size_t)rows * lmax * 4 + rank_scratch_bytes(rows * lmax) + (size_t)rows * kkc(k) * 8;
        return b;
    }
};
static LLRerankShape ll_rerank_shape(const int64_t* indptr, const int64_t* out_ptr, int64_t a, int64_t b) {
    LLRerankShape sh;
    sh.pairs = indptr[b] - indptr[a];
    sh.outs = out_ptr[b] - out_ptr[a];
    for (int64_t q = a; q < b; ++q) {
        const int64_t len = indptr[q + 1] - indptr[q];
        if (len > kRankLdsMax) { sh.rows += 1; sh.lmax = std::max(sh.lmax, len); }
    }
    return sh;
}

// the largest of every array over the chunks of a call
struct LLRerankSizes {
    int64_t pairs = 0, outs = 0, slab = 0, pos = 0;
    void cover(const LLRerankShape& sh, int32_t k) {
        pairs = std::max(pairs, sh.pairs); outs = std::max(outs, sh.outs);
        slab = std::max(slab, sh.rows * sh.lmax); pos = std::max(pos, sh.rows * sh.kkc(k));
    }
};
static int ll_rerank_alloc(LLRerankScratch& r, int64_t Qc, const LLRerankSizes& mx) {
    SERT_TRY(dmalloc(&r.cptr, (size_t)(2 * (Qc + 1))));
    SERT_TRY(dmalloc(&r.qlist, (size_t)Qc));
    SERT_TRY(dmalloc(&r.ents, (size_t)mx.pairs));
    SERT_TRY(dmalloc(&r.idx, (size_t)mx.outs));
    SERT_TRY(dmalloc(&r.val, (size_t)mx.outs));
    SERT_TRY(dmalloc(&r.slab, (size_t)mx.slab));
    SERT_TRY(dmalloc(&r.pos, (size_t)mx.pos));
    SERT_TRY(dmalloc(&r.pval, (size_t)mx.pos));
    if (mx.slab) SERT_TRY(rank_scratch_reserve(r.sort, mx.slab));
    return 0;
}

// The lists of queries a .. b ranked on their joint rows J (b - a, V), stream s: kernels and the copies of the ragged
// results to idx_out / score_out (at out_ptr[a]).  cptr / qlist: host staging, valid until the caller has synchronised s.
static int ll_rerank_chunk(hipStream_t s, const float* J, int V, LLRerankScratch& r, const int64_t* indptr, const int32_t* ents,
                           const int64_t* out_ptr, int64_t a, int64_t b, int32_t k, std::vector<int64_t>& cptr,
                           std::vector<int32_t>& qlist, int32_t* idx_out, float* score_out) {
    const int64_t Qc = b - a, e0 = indptr[a], o0 = out_ptr[a];
    const LLRerankShape sh = ll_rerank_shape(indptr, out_ptr, a, b);
    g_ll_rerank_counts[1] += 1;
    if (sh.pairs == 0) return 0;                  // (a chunk of empty lists)
    cptr.resize((size_t)(2 * (Qc + 1)));
    for (int64_t q = 0; q <= Qc; ++q) { cptr[(size_t)q] = indptr[a + q] - e0; cptr[(size_t)(Qc + 1 + q)] = out_ptr[a + q] - o0; }
    // the chunk's queries by kernel: the four LDS sizes, then the slab's rows
    int64_t cnt[5] = {0, 0, 0, 0, 0}, at[5], fill[5];
    auto klass = [&](int64_t q) { const int64_t len = indptr[q + 1] - indptr[q]; return len > kRankLdsMax ? 4 : rerank_lds_class(len); };
    for (int64_t q = a; q < b; ++q) cnt[klass(q)] += indptr[q + 1] > indptr[q];
    at[0] = 0;
    for (int i = 1; i < 5; ++i) at[i] = at[i - 1] + cnt[i - 1];
    for (int i = 0; i < 5; ++i) fill[i] = at[i];
    const int64_t nq = at[4] + cnt[4];
    qlist.assign((size_t)nq, 0);
    for (int64_t q = a; q < b; ++q)
        if (indptr[q + 1] > indptr[q]) qlist[(size_t)fill[klass(q)]++] = (int32_t)(q - a);
    SERT_HIP(hipMemcpyAsync(r.cptr, cptr.data(), cptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SERT_HIP(hipMemcpyAsync(r.ents, ents + e0, (size_t)sh.pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SERT_HIP(hipMemcpyAsync(r.qlist, qlist.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int64_t* d_indptr = r.cptr;
    const int64_t* d_out_ptr = r.cptr + Qc + 1;
    if (cnt[0]) launch(ll_rerank_lds<1024>, dim3((unsigned)cnt[0]), dim3(256), 0, s, J, V, r.ents, d_indptr, d_out_ptr, r.qlist + at[0], r.idx, r.val);
    if (cnt[1]) launch(ll_rerank_lds<2048>, dim3((unsigned)cnt[1]), dim3(256), 0, s, J, V, r.ents, d_indptr, d_out_ptr, r.qlist + at[1], r.idx, r.val);
    if (cnt[2]) launch(ll_rerank_lds<4096>, dim3((unsigned)cnt[2]), dim3(256), 0, s, J, V, r.ents, d_indptr, d_out_ptr, r.qlist + at[2], r.idx, r.val);
    if (cnt[3]) launch(ll_rerank_lds<kRankLdsMax>, dim3((unsigned)cnt[3]), dim3(256), 0, s, J, V, r.ents, d_indptr, d_out_ptr, r.qlist + at[3], r.idx, r.val);
    if (sh.rows) {
        // the lists beyond LDS: their joints into a (rows, lmax) slab, -inf behind every list, ordered by the counting-sort
        // passes as positions (stable: equal joints stay in list order, which is entity order), mapped back to entities
        const int rows = (int)sh.rows, lmax = (int)sh.lmax, kkc = (int)sh.kkc(k);
        launch(ll_rerank_gather_slab, dim3(grid_for((int64_t)rows * lmax)), dim3(256), 0, s, J, V, r.ents, d_indptr,
               r.qlist + at[4], rows, lmax, r.slab);
        SERT_TRY(rank_rows_full(s, RANK_CSORT, /*raw=*/true, r.slab, rows, lmax, kkc, r.sort, r.pos, r.pval));
        launch(rerank_compact, dim3(grid_for((int64_t)rows * kkc)), dim3(256), 0, s, r.pos, r.pval, rows, kkc, r.qlist + at[4],
               r.ents, (int64_t)0, d_indptr, d_out_ptr, (int64_t)0, r.idx, r.val);
    }
    SERT_HIP(hipGetLastError());
    SERT_HIP(hipMemcpyAsync(idx_out + o0, r.idx, (size_t)sh.outs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipMemcpyAsync(score_out + o0, r.val, (size_t)sh.outs * sizeof(float), hipMemcpyDeviceToHost, s));
    g_ll_rerank_counts[2] += at[4]; g_ll_rerank_counts[3] += cnt[4];
    return 0;
}

// where every query's results start (the ragged layout of sert_scorer_rank_candidates); counts the empty lists
static void ll_rerank_out_ptr(const int64_t* indptr, int64_t Q, int32_t k, std::vector<int64_t>& out_ptr) {
    out_ptr.assign((size_t)Q + 1, 0);
    for (int64_t q = 0; q < Q; ++q) {
        const int64_t len = indptr[q + 1] - indptr[q];
        out_ptr[(size_t)q + 1] = out_ptr[(size_t)q] + (k < 0 ? len : std::min<int64_t>(k, len));
        g_ll_rerank_counts[4] += len == 0;
    }
}

int sert_ll_rank_candidates(sert_model* m, const int32_t* tokens, const int64_t* offsets, int64_t num_queries,
                            const int64_t* cand_indptr, const int32_t* cand_entities, int32_t k, int32_t* idx_out,
                            float* score_out, float* joint_entropy_out, float* token_entropy_out, int32_t* status_out) {
    refresh_gemm_choice();
    if (!m || !tokens || !offsets || !cand_indptr || !cand_entities || !idx_out || !score_out || !joint_entropy_out ||
        !token_entropy_out || !status_out)
        SERT_FAIL("null argument");
    if (is_vs(m)) SERT_FAIL("sert_ll_rank_candidates ranks with the loglinear model");
    if (k == 0 || k < -1) SERT_FAIL("k must be -1 (the whole list) or positive");
    if (num_queries <= 0) return 0;
    SERT_TRY(ll_rank_check_offsets(offsets, num_queries));
    const auto& c = m->cfg;
    const int V = c.num_entities, d = c.word_dim;
    SERT_TRY(ll_rank_check_tokens(m, tokens, offsets[num_queries]));
    SERT_TRY(rerank_check_csr(V, num_queries, cand_indptr, cand_entities, true));
    g_ll_rerank_counts[0] += 1;
    std::vector<int64_t> out_ptr;
    ll_rerank_out_ptr(cand_indptr, num_queries, k, out_ptr);
    SERT_HIP(hipSetDevice(c.device));
    SERT_TRY(ensure_full_rw(m));
    SERT_TRY(ensure_rw_current(m, -1));

    // Chunks of consecutive queries while distinct-token rows x (d + V_e + 2) floats, the joint rows, the candidates (4 bytes a
    // pair), the results (8 an entry) and the slab of the lists beyond LDS with its sort scratch fit SERT_LL_RANK_BUDGET; a
    // chunk's slab is one sorted chunk of the counting-sort passes (rank_chunk_fits).
    const size_t budget = ll_rank_budget();
    LLRankPlan plan;
    {
        int64_t from = -1, upto = 0;            // the slab of queries from .. upto - 1, extended query by query
        LLRerankShape sh;
        ll_rank_cut(m, tokens, offsets, num_queries, [&](int64_t q0, int64_t q, int64_t D) {
            if (from != q0) { from = upto = q0; sh = LLRerankShape(); }
            for (; upto <= q; ++upto) {
                const int64_t len = cand_indptr[upto + 1] - cand_indptr[upto];
                if (len > kRankLdsMax) { sh.rows += 1; sh.lmax = std::max(sh.lmax, len); }
            }
            sh.pairs = cand_indptr[q + 1] - cand_indptr[q0];
            sh.outs = out_ptr[(size_t)q + 1] - out_ptr[(size_t)q0];
            return (sh.rows && !rank_chunk_fits(sh.rows, sh.lmax)) ||
                   ll_rank_front_bytes(D, d, V) + (size_t)(q - q0 + 1) * V * 4 + sh.bytes(k) > budget;
        }, plan);
    }
    LLRerankSizes mx;
    for (size_t ci = 0; ci + 1 < plan.bounds.size(); ++ci)
        mx.cover(ll_rerank_shape(cand_indptr, out_ptr.data(), plan.bounds[ci], plan.bounds[ci + 1]), k);

    hipStream_t s = m->stream;
    SERT_HIP(hipStreamSynchronize(s));
    LLRankScratch w;
    LLRerankScratch r;
    auto body = [&]() -> int {
        SERT_TRY(ll_rank_alloc(w, RANK_LDS, plan.max_rows, plan.max_tokens, plan.max_queries, V, d, 0));
        SERT_TRY(ll_rerank_alloc(r, plan.max_queries, mx));
        std::vector<int32_t> row_of(c.vocab_size, -1), tok_row, qlist;
        std::vector<uint32_t> ids;
        std::vector<int64_t> offs, cptr;
        std::vector<float> tok_h;
        for (size_t ci = 0; ci + 1 < plan.bounds.size(); ++ci) {
            const int64_t a = plan.bounds[ci], b = plan.bounds[ci + 1], Qc = b - a, t0 = offsets[a], Tc = offsets[b] - t0;
            const int64_t Dc = ll_rank_chunk_inputs(tokens, offsets, a, b, row_of, ids, tok_row, offs);
            const int64_t rows = (int64_t)ids.size();
            SERT_HIP(hipMemcpyAsync(w.ids, ids.data(), rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.tok_row, tok_row.data(), Tc * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.offs, offs.data(), (Qc + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
            ll_rank_chunk_distributions(m, s, w, Dc, rows);
            ll_rank_aggregate(s, w, w.P, (int)Qc, V);
            SERT_HIP(hipGetLastError());
            SERT_TRY(ll_rerank_chunk(s, w.J, V, r, cand_indptr, cand_entities, out_ptr.data(), a, b, k, cptr, qlist, idx_out, score_out));
            SERT_HIP(hipMemcpyAsync(joint_entropy_out + a, w.joint_h, (size_t)Qc * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipMemcpyAsync(status_out + a, w.status, (size_t)Qc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            tok_h.resize(Dc);
            SERT_HIP(hipMemcpyAsync(tok_h.data(), w.tok_h, Dc * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipStreamSynchronize(s));
            for (int64_t t = 0; t < Tc; ++t) token_entropy_out[t0 + t] = tok_h[tok_row[t]];
        }
        return 0;
    };
    return rerank_finish(s, body());
}

// Test hook: sert_debug_ll_rank_distributions with candidate lists -- ll_query_aggregate and the kernels of
// sert_ll_rank_candidates on per-token distributions the caller provides, as ONE chunk.
int sert_debug_ll_rank_candidates_distributions(int device, const float* P, const int64_t* offsets, int64_t num_queries,
                                                int32_t V, const int64_t* cand_indptr, const int32_t* cand_entities, int32_t k,
                                                int32_t* idx_out, float* score_out, float* joint_entropy_out,
                                                float* token_entropy_out, int32_t* status_out) {
    if (!P || !offsets || !cand_indptr || !cand_entities || !idx_out || !score_out || !joint_entropy_out ||
        !token_entropy_out || !status_out || V <= 0 || k == 0 || k < -1)
        SERT_FAIL("bad argument");
    if (num_queries <= 0) return 0;
    SERT_TRY(ll_rank_check_offsets(offsets, num_queries));
    SERT_TRY(rerank_check_csr(V, num_queries, cand_indptr, cand_entities, true));
    const int64_t T = offsets[num_queries];
    g_ll_rerank_counts[0] += 1;
    std::vector<int64_t> out_ptr;
    ll_rerank_out_ptr(cand_indptr, num_queries, k, out_ptr);
    const LLRerankShape sh = ll_rerank_shape(cand_indptr, out_ptr.data(), 0, num_queries);
    if (sh.rows && !rank_chunk_fits(sh.rows, sh.lmax)) SERT_FAIL("too many long lists for one sorted chunk");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int rc = 0;
    {
        LLRankScratch w;
        LLRerankScratch r;
        float* dP = nullptr;
        std::vector<int64_t> cptr;
        std::vector<int32_t> qlist;
        auto body = [&]() -> int {
            SERT_TRY(ll_rank_alloc(w, RANK_LDS, T, T, num_queries, V, 0, 0));
            LLRerankSizes mx;
            mx.cover(sh, k);
            SERT_TRY(ll_rerank_alloc(r, num_queries, mx));
            SERT_TRY(dmalloc(&dP, (size_t)T * V));
            std::vector<int32_t> rows(T);
            for (int64_t t = 0; t < T; ++t) rows[t] = (int32_t)t;
            SERT_HIP(hipMemcpyAsync(dP, P, (size_t)T * V * sizeof(float), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.tok_row, rows.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.offs, offsets, (num_queries + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
            launch(ll_row_entropy, dim3((unsigned)T), dim3(256), 0, s, dP, V, ll_ln2_f(), ll_log2v_f(V), w.tok_h);
            ll_rank_aggregate(s, w, dP, (int)num_queries, V);
            SERT_HIP(hipGetLastError());
            SERT_TRY(ll_rerank_chunk(s, w.J, V, r, cand_indptr, cand_entities, out_ptr.data(), 0, num_queries, k, cptr, qlist,
                                     idx_out, score_out));
            SERT_HIP(hipMemcpyAsync(joint_entropy_out, w.joint_h, (size_t)num_queries * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipMemcpyAsync(status_out, w.status, (size_t)num_queries * sizeof(int32_t), hipMemcpyDeviceToHost, s));
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

int sert_debug_ll_rerank_counts(int64_t out[5]) {
    if (!out) SERT_FAIL("null argument");
    for (int i = 0; i < 5; ++i) out[i] = g_ll_rerank_counts[i].load();
    return 0;
}
