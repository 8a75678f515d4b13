// Part of sert_hip.hip (one translation unit; included there, inside its namespace): the host chain of the full-ranking kernels
// (kernels_rank.h), shared by the cosine scorer's ranker (api_scorer_rank.inc) and the loglinear one (api_ll_rank.inc).

// How the rows of a call are ranked.  TOPK (kk <= kTopKMax: topk_rows, kernels_score.h) is each caller's own branch; the two
// choose it differently (score_rank_mode, ll_rank_mode).
enum { RANK_TOPK = 0, RANK_LDS = 1, RANK_CSORT = 2 };

// room for the LSD passes over n elements (grow-only; the caller has nothing queued that reads the old arrays)
static int rank_scratch_reserve(RankSortScratch& r, int64_t n) {
    if (r.cap >= n) return 0;
    (void)hipFree(r.keys); (void)hipFree(r.hist);
    r.keys = nullptr; r.hist = nullptr; r.cap = 0;
    SERT_TRY(dmalloc(&r.keys, (size_t)(4 * n)));
    SERT_TRY(dmalloc(&r.hist, (size_t)rank_hist_ints(n)));
    r.cap = n;
    return 0;
}

template <bool RAW>
static void rank_rows_launch(hipStream_t s, int mode, const float* S, int Qc, int V, int kk, const RankSortScratch& r, int32_t* idx,
                             float* val) {
    if (mode == RANK_LDS) {
        if (V <= 1024)      launch((rank_rows_lds<1024, RAW>), dim3(Qc), dim3(256), 0, s, S, V, kk, idx, val);
        else if (V <= 2048) launch((rank_rows_lds<2048, RAW>), dim3(Qc), dim3(256), 0, s, S, V, kk, idx, val);
        else if (V <= 4096) launch((rank_rows_lds<4096, RAW>), dim3(Qc), dim3(256), 0, s, S, V, kk, idx, val);
        else                launch((rank_rows_lds<kRankLdsMax, RAW>), dim3(Qc), dim3(256), 0, s, S, V, kk, idx, val);
        return;
    }
    // key in 11 + 11 + 10-bit digits over iota values, then the query index: stability keeps, inside a query, the key order
    // and, among equal keys, the entity order
    const int n = Qc * V;
    int32_t *ka = r.keys, *va = r.keys + (size_t)n, *kb = r.keys + (size_t)2 * n, *vb = r.keys + (size_t)3 * n;
    int32_t* bin_total = r.hist + (size_t)kSortMaxBins * cdiv(n, kSortTile);
    launch(rank_keys<RAW>, dim3(grid_for(n)), dim3(256), 0, s, S, n, ka);
    csort_pass(s, ka, nullptr, kb, vb, n, 0, 11, r.hist, bin_total);
    csort_pass(s, kb, vb, ka, va, n, 11, 11, r.hist, bin_total);
    csort_pass(s, ka, va, kb, vb, n, 22, 10, r.hist, bin_total);
    int qbits = 1;
    while ((1 << qbits) < Qc) ++qbits;
    launch(rank_query_keys, dim3(grid_for(n)), dim3(256), 0, s, vb, n, V, kb);
    csort_pass(s, kb, vb, ka, va, n, 0, qbits, r.hist, bin_total);
    launch(rank_emit<RAW>, dim3(grid_for((int64_t)Qc * kk)), dim3(256), 0, s, va, S, Qc, V, kk, idx, val);
}

// The ranking kernels on the rows of S (Qc, V), stream s: the first kk of every row into idx / val (Qc, kk), ordered and
// emitted in the RAW or the scorer form.  mode RANK_LDS: V <= kRankLdsMax.  mode RANK_CSORT: rank_chunk_fits(Qc, V), and r
// reserved for Qc V elements.
static int rank_rows_full(hipStream_t s, int mode, bool raw, const float* S, int Qc, int V, int kk, const RankSortScratch& r,
                          int32_t* idx, float* val) {
    if (raw) rank_rows_launch<true>(s, mode, S, Qc, V, kk, r, idx, val);
    else rank_rows_launch<false>(s, mode, S, Qc, V, kk, r, idx, val);
    SERT_HIP(hipGetLastError());
    return 0;
}
