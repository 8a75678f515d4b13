// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: full rankings of the cosine
// scorer on the device (include/sert_hip.h: sert_scorer_rank; include/sert_hip_debug.h: sert_debug_scorer_rank_*).  Replaces
// the host ordering of VectorSpaceCallback for --top unset, above 1024 or above the table size (bin/query.py:250-260).

// The slab GEMM runs in launches of at most this many rows.  Every fp32 kernel launch_gemm picks at splits = 1 computes an
// output element from its own row and column only, with one and the same MFMA sequence over k, so their results agree bit for
// bit; the split-bf16 kernels (gemm_x3.h) do not, and they take a product of 1024 rows or more.  Below that a chunk's cosines
// are the fp32 kernels' whatever the number of queries: a query's ranking does not depend on the chunking or on the other
// queries of the call, and the cosines are those sert_scorer_cosines returns for a block of fewer than 1024 queries.
static const int kScoreRankRows = 512;

// SERT_SCORE_RANK_BUDGET: device bytes one query chunk of sert_scorer_rank may use (score_rank_bytes)
static size_t score_rank_budget() {
    const char* e = knob("SERT_SCORE_RANK_BUDGET");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)2 << 30);
}

// which kernels rank the rows of a call: topk_rows up to kTopKMax results, a full ranking above (host/rank_rows.inc)
static int score_rank_mode(int64_t V, int kk) {
    if (kk <= kTopKMax) return RANK_TOPK;
    return V <= kRankLdsMax ? RANK_LDS : RANK_CSORT;
}

// device footprint of a chunk of Qc queries: the slab, the two (Qc, kk) result sets and, for the LSD passes, their scratch
static size_t score_rank_bytes(int mode, int64_t Qc, int64_t V, int kk) {
    size_t b = (size_t)Qc * V * 4 + (size_t)Qc * kk * 16;
    if (mode == RANK_CSORT) b += rank_scratch_bytes(Qc * V);
    return b;
}

// queries per chunk of a call of Q: as many as fit the budget and, for the LSD passes, one sorted chunk (rank_chunk_fits);
// at least one
static int64_t score_rank_chunk_queries(int mode, int64_t Q, int64_t V, int kk) {
    const size_t budget = score_rank_budget();
    int64_t lo = 1, hi = std::max<int64_t>(Q, 1);      // (both conditions are monotone in Qc: the largest Qc in [1, hi] meeting them)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if ((mode != RANK_CSORT || rank_chunk_fits(mid, V)) && score_rank_bytes(mode, mid, V, kk) <= budget) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the scratch of a call whose largest chunk holds Qc queries (sert_scorer members r* and, shared with the candidate calls,
// lists.slab / lists.sort: nothing the top-k and score calls use)
static int score_rank_scratch(sert_scorer* sc, int mode, int64_t Q, int64_t Qc, int kk) {
    const int64_t V = sc->V;
    for (int b = 0; b < 2; ++b) {
        if (!sc->ev_rsorted[b]) SERT_HIP(hipEventCreateWithFlags(&sc->ev_rsorted[b], hipEventDisableTiming));
        if (!sc->ev_rcopy0[b]) SERT_HIP(hipEventCreate(&sc->ev_rcopy0[b]));      // (timed: the pair brackets a chunk's copies)
        if (!sc->ev_rcopied[b]) SERT_HIP(hipEventCreate(&sc->ev_rcopied[b]));
    }
    SERT_TRY(sc->rP.reserve(Q * sc->dim));
    SERT_TRY(sc->lists.slab.reserve(Qc * V));
    for (int b = 0; b < 2; ++b) {
        SERT_TRY(sc->ridx[b].reserve(Qc * kk));
        SERT_TRY(sc->rval[b].reserve(Qc * kk));
    }
    if (mode == RANK_CSORT) SERT_TRY(rank_scratch_reserve(sc->lists.sort, Qc * V));
    return 0;
}

int sert_scorer_rank(sert_scorer* sc, const float* proj, int64_t Q, int32_t k, int32_t* idx_out, float* score_out) {
    if (!sc || !proj || !idx_out || !score_out) SERT_FAIL("null argument");
    if (k == 0 || k < -1) SERT_FAIL("k must be -1 (every entity) or positive");
    if (Q < 0) SERT_FAIL("bad sizes");
    if (Q == 0) return 0;
    const int64_t V = sc->V;
    const int dim = sc->dim;
    const int kk = (k < 0 || k >= V) ? (int)V : k;
    const int mode = score_rank_mode(V, kk);
    const int64_t Qc = score_rank_chunk_queries(mode, Q, V, kk);
    const int64_t nchunks = cdiv(Q, Qc);
    sc->rank_counts[0] += 1;
    if (mode == RANK_TOPK) {
        // sert_scorer_topk itself on every chunk.  One chunk (any call the budget holds whole) is sert_scorer_topk(kk) of the
        // call; a call the budget cuts equals it as long as that call's own GEMM keeps one kernel family whatever its row
        // count -- not for d_e >= 256, where a block of 1024 rows or more goes to the split-bf16 kernels and its chunks may not
        for (int64_t q0 = 0; q0 < Q; q0 += Qc) {
            const int64_t qn = std::min(Qc, Q - q0);
            SERT_TRY(scorer_topk_io(sc, proj + q0 * dim, qn, kk, idx_out + q0 * kk, score_out + q0 * kk, false));
            sc->rank_counts[1] += 1; sc->rank_counts[2] += qn;
        }
        return 0;
    }
    SERT_HIP(hipSetDevice(sc->device));
    SERT_TRY(score_rank_scratch(sc, mode, Q, Qc, kk));
    hipStream_t s = sc->stream, s2 = sc->stream2;
    double copy_ms = 0.0;
    bool timed[2] = {false, false};
    // the time the copies of result set b took on the second stream, between the two events around them
    auto harvest = [&](int b) -> int {
        if (!timed[b]) return 0;
        float ms = 0.f;
        SERT_HIP(hipEventSynchronize(sc->ev_rcopied[b]));
        SERT_HIP(hipEventElapsedTime(&ms, sc->ev_rcopy0[b], sc->ev_rcopied[b]));
        copy_ms += ms;
        timed[b] = false;
        return 0;
    };
    // chunk c's results to the caller's arrays on the second stream, behind its sort (a pageable destination: the call
    // returns when the bytes have arrived -- the next chunk's sort, enqueued before, runs meanwhile)
    auto copy_out = [&](int64_t c) -> int {
        const int b = (int)(c & 1);
        const int64_t q0 = c * Qc, qn = std::min(Qc, Q - q0);
        SERT_TRY(harvest(b));                                     // (chunk c - 2's copies: long done)
        SERT_HIP(hipStreamWaitEvent(s2, sc->ev_rsorted[b], 0));
        SERT_HIP(hipEventRecord(sc->ev_rcopy0[b], s2));
        SERT_HIP(hipMemcpyAsync(idx_out + q0 * kk, sc->ridx[b].p, (size_t)qn * kk * sizeof(int32_t), hipMemcpyDeviceToHost, s2));
        SERT_HIP(hipMemcpyAsync(score_out + q0 * kk, sc->rval[b].p, (size_t)qn * kk * sizeof(float), hipMemcpyDeviceToHost, s2));
        SERT_HIP(hipEventRecord(sc->ev_rcopied[b], s2));
        timed[b] = true;
        return 0;
    };
    auto body = [&]() -> int {
        SERT_HIP(hipMemcpyAsync(sc->rP.p, proj, (size_t)Q * dim * sizeof(float), hipMemcpyHostToDevice, s));
        launch(l2_normalize_rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, sc->rP.p, Q, dim);
        for (int64_t c = 0; c < nchunks; ++c) {
            const int b = (int)(c & 1);
            const int64_t q0 = c * Qc, qn = std::min(Qc, Q - q0);
            if (c >= 2) SERT_HIP(hipStreamWaitEvent(s, sc->ev_rcopied[b], 0));      // (chunk c - 2 has left this result set)
            for (int64_t r0 = 0; r0 < qn; r0 += kScoreRankRows)
                scorer_cosine_slab(sc, s, sc->rP.p + (q0 + r0) * dim, std::min<int64_t>(kScoreRankRows, qn - r0), sc->lists.slab.p + (size_t)r0 * V, sc->bf16);
            SERT_TRY(rank_rows_full(s, mode, /*raw=*/false, sc->lists.slab.p, (int)qn, (int)V, kk, sc->lists.sort, sc->ridx[b].p, sc->rval[b].p));
            SERT_HIP(hipEventRecord(sc->ev_rsorted[b], s));
            if (c >= 1) SERT_TRY(copy_out(c - 1));
            sc->rank_counts[1] += 1; sc->rank_counts[mode == RANK_LDS ? 3 : 4] += qn;
        }
        SERT_TRY(copy_out(nchunks - 1));
        SERT_HIP(hipStreamSynchronize(s2));
        SERT_HIP(hipStreamSynchronize(s));
        SERT_TRY(harvest(0));
        SERT_TRY(harvest(1));
        return 0;
    };
    const int rc = body();
    if (rc != 0) {      // nothing of this call stays queued: the next one reuses the scratch, and the caller its arrays
        const std::string keep = g_last_error;
        (void)hipStreamSynchronize(s2);
        (void)hipStreamSynchronize(s);
        g_last_error = keep;
        return rc;
    }
    sc->rank_counts[5] += (int64_t)(copy_ms * 1000.0);
    return 0;
}
