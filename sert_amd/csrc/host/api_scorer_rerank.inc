// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: cosines and rankings of
// per-query candidate lists (include/sert_hip.h: sert_scorer_pairs, sert_scorer_rank_candidates; include/sert_hip_debug.h:
// sert_debug_scorer_rerank_counts).  Kernels: csrc/kernels_rerank.h.  The scratch is the scorer's (model.h, c*), together with
// the ranker's rP / rS / rsort: every call of a scorer returns with nothing queued, so the two never hold them at once.

// grow-only device array of a scorer (a template: C++ linkage inside this extern "C" block)
extern "C++" {
template <typename T>
static int rerank_reserve(T** p, int64_t* cap, int64_t n) {
    if (*cap >= n) return 0;
    (void)hipFree(*p); *p = nullptr; *cap = 0;
    SERT_TRY(dmalloc(p, (size_t)n));
    *cap = n;
    return 0;
}
}

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

// the call's projections, normalised, in rP; its indptr (and, ranker, the output offsets behind it) in cptr
static int rerank_upload_queries(sert_scorer* sc, hipStream_t s, const float* proj, int64_t Q, const int64_t* indptr,
                                 const int64_t* out_ptr) {
    if (sc->cap_rp < Q) {       // (cap_rp counts rows, as score_rank_scratch keeps it)
        (void)hipFree(sc->rP); sc->rP = nullptr; sc->cap_rp = 0;
        SERT_TRY(dmalloc(&sc->rP, (size_t)Q * sc->dim));
        sc->cap_rp = Q;
    }
    SERT_TRY(rerank_reserve(&sc->cptr, &sc->cap_cptr, 2 * (Q + 1)));
    SERT_HIP(hipMemcpyAsync(sc->rP, proj, (size_t)Q * sc->dim * sizeof(float), hipMemcpyHostToDevice, s));
    launch(l2_normalize_rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, sc->rP, Q, sc->dim);
    SERT_HIP(hipMemcpyAsync(sc->cptr, indptr, (size_t)(Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (out_ptr) SERT_HIP(hipMemcpyAsync(sc->cptr + Q + 1, out_ptr, (size_t)(Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
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
    auto body = [&]() -> int {
        SERT_TRY(rerank_reserve(&sc->cents, &sc->cap_cents, Nc));
        SERT_TRY(rerank_reserve(&sc->cval, &sc->cap_cval, Nc));
        SERT_TRY(rerank_upload_queries(sc, s, proj, Q, indptr, nullptr));
        for (int64_t j0 = 0; j0 < N; j0 += Nc) {
            const int64_t j1 = std::min(N, j0 + Nc);
            SERT_HIP(hipMemcpyAsync(sc->cents, ents + j0, (size_t)(j1 - j0) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            launch(rerank_pair_cosines<false>, dim3(rerank_pair_grid(j1 - j0)), dim3(256), 0, s, sc->rP, sc->E, sc->dim,
                   sc->cents, j0, sc->cptr, sc->cptr, (int)Q, (const int32_t*)nullptr, j0, j1, sc->cval, (int64_t)0, raw ? 1 : 0);
            SERT_HIP(hipGetLastError());
            SERT_HIP(hipMemcpyAsync(out + j0, sc->cval, (size_t)(j1 - j0) * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipStreamSynchronize(s));
            sc->rerank_counts[1] += 1; sc->rerank_counts[4] += j1 - j0;
        }
        return 0;
    };
    return rerank_finish(s, body());
}

// the LDS size a list of len candidates is sorted in (rank_rows_lds' sizes), as an index 0 .. 3
static int rerank_lds_class(int64_t len) { return len <= 1024 ? 0 : len <= 2048 ? 1 : len <= 4096 ? 2 : 3; }

int sert_scorer_rank_candidates(sert_scorer* sc, const float* proj, int64_t Q, const int64_t* indptr, const int32_t* ents,
                                int32_t k, int32_t* idx_out, float* score_out) {
    if (k == 0 || k < -1) SERT_FAIL("k must be -1 (the whole list) or positive");
    SERT_TRY(rerank_check(sc, proj, Q, indptr, ents, idx_out, score_out, true));
    sc->rerank_counts[0] += 1;
    if (Q == 0) return 0;
    // ranked depth per query and where its results start
    std::vector<int64_t> out_ptr((size_t)Q + 1, 0);
    for (int64_t q = 0; q < Q; ++q) {
        const int64_t len = indptr[q + 1] - indptr[q];
        out_ptr[q + 1] = out_ptr[q] + (k < 0 ? len : std::min<int64_t>(k, len));
        sc->rerank_counts[5] += len == 0;
    }
    if (indptr[Q] == 0) return 0;
    // Chunks of consecutive queries under the budget: the candidates (4 bytes a pair), the results (8 a ranked entry) and, for
    // the lists beyond LDS, their padded slab (rows x the longest of them), the scratch of its counting-sort passes and the
    // (rows, kkc) positions and scores they emit.  A chunk takes the next query while it fits; its first one always.
    const size_t budget = score_rank_budget();
    struct Chunk { int64_t q0, q1, rows, lmax; };
    std::vector<Chunk> chunks;
    auto chunk_bytes = [&](int64_t pairs, int64_t outs, int64_t rows, int64_t lmax) -> size_t {
        size_t b = (size_t)pairs * 4 + (size_t)outs * 8;
        if (rows) b += (size_t)rows * lmax * 4 + rank_scratch_bytes(rows * lmax) + (size_t)rows * (k < 0 ? lmax : std::min<int64_t>(k, lmax)) * 8;
        return b;
    };
    for (int64_t q = 0; q < Q;) {
        Chunk c = {q, q, 0, 0};
        for (; q < Q; ++q) {
            const int64_t len = indptr[q + 1] - indptr[q];
            const bool slab = len > kRankLdsMax;
            const int64_t rows = c.rows + slab, lmax = slab ? std::max(c.lmax, len) : c.lmax;
            if (q > c.q0 && ((rows && !rank_chunk_fits(rows, lmax)) ||
                             chunk_bytes(indptr[q + 1] - indptr[c.q0], out_ptr[q + 1] - out_ptr[c.q0], rows, lmax) > budget))
                break;
            c.rows = rows; c.lmax = lmax;
        }
        c.q1 = q;
        if (c.lmax >= ((int64_t)1 << 31) || (c.rows && !rank_chunk_fits(c.rows, c.lmax))) SERT_FAIL("a candidate list is too long to rank");
        chunks.push_back(c);
    }
    SERT_HIP(hipSetDevice(sc->device));
    hipStream_t s = sc->stream;
    const int dim = sc->dim;
    std::vector<int32_t> qlist;
    std::vector<int64_t> sptr;
    auto body = [&]() -> int {
        SERT_TRY(rerank_upload_queries(sc, s, proj, Q, indptr, out_ptr.data()));
        const int64_t* d_indptr = sc->cptr;
        const int64_t* d_out_ptr = sc->cptr + Q + 1;
        for (const Chunk& c : chunks) {
            const int64_t e0 = indptr[c.q0], pairs = indptr[c.q1] - e0, o0 = out_ptr[c.q0], outs = out_ptr[c.q1] - o0;
            sc->rerank_counts[1] += 1;
            if (pairs == 0) continue;                  // (a chunk of empty lists)
            // the chunk's queries by kernel: the four LDS sizes, then the slab's rows (with the prefix of their lengths)
            int64_t cnt[5] = {0, 0, 0, 0, 0}, at[5];
            auto klass = [&](int64_t q) { const int64_t len = indptr[q + 1] - indptr[q]; return len > kRankLdsMax ? 4 : rerank_lds_class(len); };
            for (int64_t q = c.q0; q < c.q1; ++q) cnt[klass(q)] += indptr[q + 1] > indptr[q];
            at[0] = 0;
            for (int i = 1; i < 5; ++i) at[i] = at[i - 1] + cnt[i - 1];
            const int64_t nq = at[4] + cnt[4];
            qlist.assign((size_t)nq, 0);
            sptr.assign((size_t)c.rows + 1, 0);
            {
                int64_t fill[5] = {at[0], at[1], at[2], at[3], at[4]};
                for (int64_t q = c.q0; q < c.q1; ++q) {
                    const int64_t len = indptr[q + 1] - indptr[q];
                    if (len == 0) continue;
                    const int kl = klass(q);
                    if (kl == 4) sptr[(size_t)(fill[4] - at[4]) + 1] = sptr[(size_t)(fill[4] - at[4])] + len;
                    qlist[(size_t)fill[kl]++] = (int32_t)q;
                }
            }
            SERT_TRY(rerank_reserve(&sc->cents, &sc->cap_cents, pairs));
            SERT_TRY(rerank_reserve(&sc->cidx, &sc->cap_cidx, outs));
            SERT_TRY(rerank_reserve(&sc->cval, &sc->cap_cval, outs));
            SERT_TRY(rerank_reserve(&sc->cq, &sc->cap_cq, nq));
            SERT_HIP(hipMemcpyAsync(sc->cents, ents + e0, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(sc->cq, qlist.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
            if (cnt[0]) launch(rerank_lds<1024>, dim3((unsigned)cnt[0]), dim3(256), 0, s, sc->rP, sc->E, dim, sc->cents, e0, d_indptr, d_out_ptr, o0, sc->cq + at[0], sc->cidx, sc->cval);
            if (cnt[1]) launch(rerank_lds<2048>, dim3((unsigned)cnt[1]), dim3(256), 0, s, sc->rP, sc->E, dim, sc->cents, e0, d_indptr, d_out_ptr, o0, sc->cq + at[1], sc->cidx, sc->cval);
            if (cnt[2]) launch(rerank_lds<4096>, dim3((unsigned)cnt[2]), dim3(256), 0, s, sc->rP, sc->E, dim, sc->cents, e0, d_indptr, d_out_ptr, o0, sc->cq + at[2], sc->cidx, sc->cval);
            if (cnt[3]) launch(rerank_lds<kRankLdsMax>, dim3((unsigned)cnt[3]), dim3(256), 0, s, sc->rP, sc->E, dim, sc->cents, e0, d_indptr, d_out_ptr, o0, sc->cq + at[3], sc->cidx, sc->cval);
            if (c.rows) {
                // the lists beyond LDS: their cosines into a (rows, lmax) slab whose padding is NaN (every byte 0xff) -- behind
                // every real position of its row, so it ranks last -- ordered by the counting-sort passes as positions
                const int rows = (int)c.rows, lmax = (int)c.lmax, kkc = k < 0 ? lmax : (int)std::min<int64_t>(k, lmax);
                const int64_t items = sptr[(size_t)rows];
                SERT_TRY(rerank_reserve(&sc->rS, &sc->cap_rs, (int64_t)rows * lmax));
                SERT_TRY(rerank_reserve(&sc->csptr, &sc->cap_csptr, rows + 1));
                SERT_TRY(rerank_reserve(&sc->cpos, &sc->cap_cpos, (int64_t)rows * kkc));
                SERT_TRY(rerank_reserve(&sc->cpval, &sc->cap_cpval, (int64_t)rows * kkc));
                SERT_TRY(rank_scratch_reserve(sc->rsort, (int64_t)rows * lmax));
                SERT_HIP(hipMemcpyAsync(sc->csptr, sptr.data(), (size_t)(rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
                SERT_HIP(hipMemsetAsync(sc->rS, 0xff, (size_t)rows * lmax * sizeof(float), s));
                launch(rerank_pair_cosines<true>, dim3(rerank_pair_grid(items)), dim3(256), 0, s, sc->rP, sc->E, dim, sc->cents, e0,
                       d_indptr, sc->csptr, rows, sc->cq + at[4], (int64_t)0, items, sc->rS, (int64_t)lmax, 1);
                SERT_TRY(rank_rows_full(s, RANK_CSORT, /*raw=*/false, sc->rS, rows, lmax, kkc, sc->rsort, sc->cpos, sc->cpval));
                launch(rerank_compact, dim3(grid_for((int64_t)rows * kkc)), dim3(256), 0, s, sc->cpos, sc->cpval, rows, kkc,
                       sc->cq + at[4], sc->cents, e0, d_indptr, d_out_ptr, o0, sc->cidx, sc->cval);
            }
            SERT_HIP(hipGetLastError());
            SERT_HIP(hipMemcpyAsync(idx_out + o0, sc->cidx, (size_t)outs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipMemcpyAsync(score_out + o0, sc->cval, (size_t)outs * sizeof(float), hipMemcpyDeviceToHost, s));
            SERT_HIP(hipStreamSynchronize(s));       // (qlist / sptr are rebuilt for the next chunk; its scratch is this one's)
            sc->rerank_counts[2] += at[4]; sc->rerank_counts[3] += cnt[4]; sc->rerank_counts[4] += pairs;
        }
        return 0;
    };
    return rerank_finish(s, body());
}
