// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block, behind api_ll_rank.inc and
// api_scorer_rerank.inc): C ABI: per-query candidate lists ranked with the loglinear model (include/sert_hip.h:
// sert_ll_rank_candidates; include/sert_hip_debug.h: sert_debug_ll_rank_candidates_distributions, sert_debug_ll_rerank_counts).
// Kernels: csrc/kernels_ll_rerank.h; the host chain behind the joint rows: host/rank_lists.inc.  The joint rows come from the
// chain of sert_ll_rank_queries (api_ll_rank.inc: ll_rank_chunk_inputs, ll_rank_chunk_distributions, ll_rank_aggregate) -- the
// scores stay normalised over all entities -- and only the listed entries of a row are sorted and copied out: no Qc x V_e
// sort scratch, no (Qc, V_e) outputs.

// What the candidate calls of this PROCESS did (sert_debug_ll_rerank_counts): [0] calls that passed their argument checks,
// [1] their chunks, lists ranked by [2] the LDS kernel, [3] the slab and the counting-sort passes, [4] empty lists.
// Process-wide, not per model: the debug call has no model, and one scope serves both (a test takes differences).
static std::atomic<int64_t> g_ll_rerank_counts[5];

// The lists of queries a .. b ranked on their joint rows J (b - a, V), stream s, through the shared chain (rank_lists.inc).
// The slab's padding is -inf: a DEVICE query's joints are finite and >= 0, a HOST query's row is zero, so it ranks last.
static int ll_rerank_chunk(hipStream_t s, const float* J, int V, ListScratch& r, const int64_t* indptr, const int32_t* ents,
                           const int64_t* out_ptr, int64_t a, int64_t b, int32_t k, int32_t* idx_out, float* score_out) {
    auto lds = [&](auto n, unsigned count, const int32_t* qlist) {
        launch(ll_rerank_lds<decltype(n)::value>, dim3(count), dim3(256), 0, s, J, V, r.ents.p, r.cptr.p, r.cptr.p + (b - a + 1),
               qlist, r.idx.p, r.val.p);
    };
    auto fill_slab = [&](const int32_t*, const int32_t* d_rows, int rows, int lmax) -> int {
        launch(ll_rerank_gather_slab, dim3(grid_for((int64_t)rows * lmax)), dim3(256), 0, s, J, V, r.ents.p, r.cptr.p, d_rows,
               rows, lmax, r.slab.p);
        return 0;
    };
    int64_t ranked[2] = {0, 0};
    g_ll_rerank_counts[1] += 1;
    SERT_TRY(rank_lists_chunk(s, r, indptr, ents, out_ptr, a, b, k, /*raw=*/true, lds, fill_slab, idx_out, score_out, ranked));
    g_ll_rerank_counts[2] += ranked[0]; g_ll_rerank_counts[3] += ranked[1];
    return 0;
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
    g_ll_rerank_counts[4] += list_out_ptr(cand_indptr, num_queries, k, out_ptr);
    SERT_HIP(hipSetDevice(c.device));
    SERT_TRY(ensure_full_rw(m));
    SERT_TRY(ensure_rw_current(m, -1));

    // Chunks of consecutive queries while distinct-token rows x (d + V_e + 2) floats, the joint rows, the candidates (4 bytes a
    // pair), the results (8 an entry) and the slab of the lists beyond LDS with its sort scratch fit SERT_LL_RANK_BUDGET; a
    // chunk's slab is one sorted chunk of the counting-sort passes (rank_chunk_fits).
    const size_t budget = ll_rank_budget();
    LLRankPlan plan;
    {
        int64_t from = -1, upto = 0;            // the shape of queries from .. upto - 1, extended query by query
        ListShape sh;
        ll_rank_cut(m, tokens, offsets, num_queries, [&](int64_t q0, int64_t q, int64_t D) {
            if (from != q0) { from = upto = q0; sh = ListShape(); }
            for (; upto <= q; ++upto)
                sh = sh.plus(cand_indptr[upto + 1] - cand_indptr[upto], out_ptr[(size_t)upto + 1] - out_ptr[(size_t)upto]);
            return (sh.rows && !rank_chunk_fits(sh.rows, sh.lmax)) ||
                   ll_rank_front_bytes(D, d, V) + (size_t)(q - q0 + 1) * V * 4 + sh.bytes(k) > budget;
        }, plan);
    }

    hipStream_t s = m->stream;
    SERT_HIP(hipStreamSynchronize(s));
    LLRankScratch w;
    ListScratch r;
    auto body = [&]() -> int {
        SERT_TRY(ll_rank_alloc(w, RANK_LDS, plan.max_rows, plan.max_tokens, plan.max_queries, V, d, 0));
        std::vector<int32_t> row_of(c.vocab_size, -1), tok_row;
        std::vector<uint32_t> ids;
        std::vector<int64_t> offs;
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
            SERT_TRY(ll_rerank_chunk(s, w.J, V, r, cand_indptr, cand_entities, out_ptr.data(), a, b, k, idx_out, score_out));
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
    g_ll_rerank_counts[4] += list_out_ptr(cand_indptr, num_queries, k, out_ptr);
    ListShape sh;
    for (int64_t q = 0; q < num_queries; ++q) sh = sh.plus(cand_indptr[q + 1] - cand_indptr[q], out_ptr[(size_t)q + 1] - out_ptr[(size_t)q]);
    if (sh.rows && !rank_chunk_fits(sh.rows, sh.lmax)) SERT_FAIL("too many long lists for one sorted chunk");
    SERT_HIP(hipSetDevice(device));
    hipStream_t s;
    SERT_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int rc = 0;
    {
        LLRankScratch w;
        ListScratch r;
        float* dP = nullptr;
        auto body = [&]() -> int {
            SERT_TRY(ll_rank_alloc(w, RANK_LDS, T, T, num_queries, V, 0, 0));
            SERT_TRY(dmalloc(&dP, (size_t)T * V));
            std::vector<int32_t> rows(T);
            for (int64_t t = 0; t < T; ++t) rows[t] = (int32_t)t;
            SERT_HIP(hipMemcpyAsync(dP, P, (size_t)T * V * sizeof(float), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.tok_row, rows.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(w.offs, offsets, (num_queries + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
            launch(ll_row_entropy, dim3((unsigned)T), dim3(256), 0, s, dP, V, ll_ln2_f(), ll_log2v_f(V), w.tok_h);
            ll_rank_aggregate(s, w, dP, (int)num_queries, V);
            SERT_HIP(hipGetLastError());
            SERT_TRY(ll_rerank_chunk(s, w.J, V, r, cand_indptr, cand_entities, out_ptr.data(), 0, num_queries, k, idx_out,
                                     score_out));
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
