// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: cosines and rankings of
// per-query candidate lists (include/sert_hip.h: sert_scorer_pairs, sert_scorer_rank_candidates; include/sert_hip_debug.h:
// sert_debug_scorer_rerank_counts).  Kernels: csrc/kernels_rerank.h; the ranker's host chain: host/rank_lists.inc.  The scratch
// is the scorer's (model.h: rP, lists, csptr); lists.slab / lists.sort are sert_scorer_rank's too: every call of a scorer
// returns with nothing queued, so the two never hold them at once.

// The faults of a candidate CSR over V entities, found before anything is launched.  ascending: the rankers' lists (strictly
// ascending, hence free of duplicates).  Also sert_ll_rank_candidates' check (api_ll_rerank.inc).
static int rerank_check_csr(int64_t V, int64_t Q, const int64_t* indptr, const int32_t* ents, bool ascending) {
    if (Q < 0 || Q >= ((int64_t)1 << 31) - 1) SERT_FAIL("bad sizes");
    if (indptr[0] != 0) SERT_FAIL("cand_indptr[0] must be 0");
    for (int64_t q = 0; q < Q; ++q)
        if (indptr[q + 1] < indptr[q]) SERT_FAIL("cand_indptr decreases at query " + std::to_string(q));
    for (int64_t q = 0; q < Q; ++q)
        for (int64_t j = indptr[q]; j < indptr[q + 1]; ++j) {
            if (ents[j] < 0 || ents[j] >= V)
                SERT_FAIL("candidate entity out of range: " + std::to_string(ents[j]) + " in the list of query " + std::to_string(q));
            if (ascending && j > indptr[q] && ents[j] <= ents[j - 1])
                SERT_FAIL("candidate list not strictly ascending (unsorted or duplicated) at query " + std::to_string(q));
        }
    return 0;
}
static int rerank_check(const sert_scorer* sc, const float* proj, int64_t Q, const int64_t* indptr, const int32_t* ents,
                        const void* out_a, const void* out_b, bool ascending) {
    if (!sc || !proj || !indptr || !ents || !out_a || !out_b) SERT_FAIL("null argument");
    return rerank_check_csr(sc->V, Q, indptr, ents, ascending);
}

// the call's projections, normalised, in rP
static int rerank_upload_queries(sert_scorer* sc, hipStream_t s, const float* proj, int64_t Q) {
    SERT_TRY(sc->rP.reserve(Q * sc->dim));
    SERT_HIP(hipMemcpyAsync(sc->rP.p, proj, (size_t)Q * sc->dim * sizeof(float), hipMemcpyHostToDevice, s));
    launch(l2_normalize_rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, sc->rP.p, Q, sc->dim);
    return 0;
}

// workgroups of the pair kernel: eight per CU's worth at most, and at least four trips per half-wave behind its one bisection
static unsigned rerank_pair_grid(int64_t items) { return (unsigned)std::min<int64_t>(cdiv(items, 4 * kRerankTile), 2048); }

// nothing of a failed call stays queued on its stream s (sert_scorer_rank's rule; also sert_ll_rank_candidates')
static int rerank_finish(hipStream_t s, int rc) {
    if (rc == 0) return 0;
    const std::string keep = g_last_error;
    (void)hipStreamSynchronize(s);
    g_last_error = keep;
    return rc;
}

int sert_scorer_pairs(sert_scorer* sc, const float* proj, int64_t Q, const int64_t* indptr, const int32_t* ents, int raw,
                      float* out) {
    SERT_TRY(rerank_check(sc, proj, Q, indptr, ents, out, out, false));
    sc->rerank_counts[0] += 1;
    if (Q == 0) return 0;
    const int64_t N = indptr[Q];
    for (int64_t q = 0; q < Q; ++q) sc->rerank_counts[5] += indptr[q + 1] == indptr[q];
    if (N == 0) return 0;
    SERT_HIP(hipSetDevice(sc->device));
    hipStream_t s = sc->stream;
    // pairs per chunk: the candidates in, the values out (8 bytes a pair) under the budget; at least one
    const int64_t Nc = std::min<int64_t>(N, std::max<int64_t>(1, (int64_t)(score_rank_budget() / 8)));
    ListScratch& r = sc->lists;             // (cptr: the call's indptr; ents / val: a chunk's candidates and their values)
    auto body = [&]() -> int {
        SERT_TRY(r.ents.reserve(Nc));
        SERT_TRY(r.val.reserve(Nc));
        SERT_TRY(r.cptr.reserve(Q + 1));
        SERT_TRY(rerank_upload_queries(sc, s, proj, Q));
        SERT_HIP(hipMemcpyAsync(r.cptr.p, indptr, (size_t)(Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        for (int64_t j0 = 0; j0 < N; j0 += Nc) {
            const int64_t j1 = std::min(N, j0 + Nc);
            SERT_HIP(hipMemcpyAsync(r.ents.p, ents + j0, (size_t)(j1 - j0) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            launch(rerank_pair_cosines<false>, dim3(rerank_pair_grid(j1 - j0)), dim3(256), 0, s, sc->rP.p, sc->E, sc->dim,
                   r.ents.p, j0, r.cptr.p, r.cptr.p, (int)Q, (const int32_t*)nullptr, j0, j1, r.val.p, (int64_t)0, raw ? 1 : 0);
            SERT_HIP(hipGetLastError());
            SERT_HIP(hipMemcpyAsync(out + j0, r.val.p, (size_t)(j1 - j0) * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipStreamSynchronize(s));
            sc->rerank_counts[1] += 1; sc->rerank_counts[4] += j1 - j0;
        }
        return 0;
    };
    return rerank_finish(s, body());
}

int sert_scorer_rank_candidates(sert_scorer* sc, const float* proj, int64_t Q, const int64_t* indptr, const int32_t* ents,
                                int32_t k, int32_t* idx_out, float* score_out) {
    if (k == 0 || k < -1) SERT_FAIL("k must be -1 (the whole list) or positive");
    SERT_TRY(rerank_check(sc, proj, Q, indptr, ents, idx_out, score_out, true));
    sc->rerank_counts[0] += 1;
    if (Q == 0) return 0;
    std::vector<int64_t> out_ptr;              // ranked depth per query and where its results start
    sc->rerank_counts[5] += list_out_ptr(indptr, Q, k, out_ptr);
    if (indptr[Q] == 0) return 0;
    // Chunks of consecutive queries under the budget: the candidates (4 bytes a pair), the results (8 a ranked entry) and, for
    // the lists beyond LDS, their padded slab (rows x the longest of them), the scratch of its counting-sort passes and the
    // (rows, kkc) positions and scores they emit (ListShape::bytes).  A chunk takes the next query while it fits; its first
    // one always.
    const size_t budget = score_rank_budget();
    std::vector<int64_t> bounds(1, 0);
    for (int64_t q = 0; q < Q;) {
        ListShape sh;
        for (const int64_t q0 = q; q < Q; ++q) {
            const ListShape next = sh.plus(indptr[q + 1] - indptr[q], out_ptr[(size_t)q + 1] - out_ptr[(size_t)q]);
            if (q > q0 && ((next.rows && !rank_chunk_fits(next.rows, next.lmax)) || next.bytes(k) > budget)) break;
            sh = next;
        }
        if (sh.lmax >= ((int64_t)1 << 31) || (sh.rows && !rank_chunk_fits(sh.rows, sh.lmax))) SERT_FAIL("a candidate list is too long to rank");
        bounds.push_back(q);
    }
    SERT_HIP(hipSetDevice(sc->device));
    hipStream_t s = sc->stream;
    const int dim = sc->dim;
    ListScratch& r = sc->lists;
    std::vector<int64_t> sptr;
    auto body = [&]() -> int {
        SERT_TRY(rerank_upload_queries(sc, s, proj, Q));
        for (size_t ci = 0; ci + 1 < bounds.size(); ++ci) {
            const int64_t a = bounds[ci], b = bounds[ci + 1];
            const float* P = sc->rP.p + a * dim;       // (the chunk's rows: its kernels index them from its first query)
            auto lds = [&](auto n, unsigned count, const int32_t* qlist) {
                launch(rerank_lds<decltype(n)::value>, dim3(count), dim3(256), 0, s, P, sc->E, dim, r.ents.p, r.cptr.p,
                       r.cptr.p + (b - a + 1), qlist, r.idx.p, r.val.p);
            };
            // the slab's padding is NaN (every byte 0xff) -- behind every real position of its row, so it ranks last; the
            // pair kernel walks the rows by the prefix of their lengths
            auto fill_slab = [&](const int32_t* h_rows, const int32_t* d_rows, int rows, int lmax) -> int {
                sptr.assign((size_t)rows + 1, 0);
                for (int i = 0; i < rows; ++i) sptr[(size_t)i + 1] = sptr[(size_t)i] + indptr[a + h_rows[i] + 1] - indptr[a + h_rows[i]];
                SERT_TRY(sc->csptr.reserve(rows + 1));
                SERT_HIP(hipMemcpyAsync(sc->csptr.p, sptr.data(), (size_t)(rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
                SERT_HIP(hipMemsetAsync(r.slab.p, 0xff, (size_t)rows * lmax * sizeof(float), s));
                launch(rerank_pair_cosines<true>, dim3(rerank_pair_grid(sptr[(size_t)rows])), dim3(256), 0, s, P, sc->E, dim, r.ents.p,
                       (int64_t)0, r.cptr.p, sc->csptr.p, rows, d_rows, (int64_t)0, sptr[(size_t)rows], r.slab.p, (int64_t)lmax, 1);
                return 0;
            };
            sc->rerank_counts[1] += 1;
            SERT_TRY(rank_lists_chunk(s, r, indptr, ents, out_ptr.data(), a, b, k, /*raw=*/false, lds, fill_slab, idx_out, score_out,
                                      &sc->rerank_counts[2]));
            SERT_HIP(hipStreamSynchronize(s));       // (the staging and the scratch are the next chunk's too)
            sc->rerank_counts[4] += indptr[b] - indptr[a];
        }
        return 0;
    };
    return rerank_finish(s, body());
}
