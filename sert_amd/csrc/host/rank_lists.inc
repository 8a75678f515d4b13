// Part of sert_hip.hip (one translation unit; included there, inside its namespace, behind rank_rows.inc): the host chain that
// ranks per-query candidate lists, shared by the cosine re-ranker (api_scorer_rerank.inc) and the loglinear one
// (api_ll_rerank.inc).  Kernels: kernels_rerank.h, kernels_ll_rerank.h; the scratch is ListScratch (model.h).  The callers
// keep what differs: how they cut a call into chunks, and the two kernels each that produce their scores.

// What of a chunk sizes its scratch: candidates, ranked entries, and the slab of its lists beyond LDS (rows x the longest)
struct ListShape {
    int64_t pairs = 0, outs = 0, rows = 0, lmax = 0;
    // the shape with one more query: a list of len candidates, `ranked` of them written out
    ListShape plus(int64_t len, int64_t ranked) const {
        const bool slab = len > kRankLdsMax;
        return {pairs + len, outs + ranked, rows + slab, slab ? std::max(lmax, len) : lmax};
    }
    int64_t kkc(int32_t k) const { return k < 0 ? lmax : std::min<int64_t>(k, lmax); }
    size_t bytes(int32_t k) const {
        size_t b = (size_t)pairs * 4 + (size_t)outs * 8;
        if (rows) b += (size_t)rows * lmax * 4 + rank_scratch_bytes(rows * lmax) + (size_t)rows * kkc(k) * 8;
        return b;
    }
};

// where every query's results start: the ragged layout of the ranked lists, min(k, length) entries each (k < 0: all of them).
// Returns the number of empty lists.
static int64_t list_out_ptr(const int64_t* indptr, int64_t Q, int32_t k, std::vector<int64_t>& out_ptr) {
    int64_t empty = 0;
    out_ptr.assign((size_t)Q + 1, 0);
    for (int64_t q = 0; q < Q; ++q) {
        const int64_t len = indptr[q + 1] - indptr[q];
        out_ptr[(size_t)q + 1] = out_ptr[(size_t)q] + (k < 0 ? len : std::min<int64_t>(k, len));
        empty += len == 0;
    }
    return empty;
}

// The lists of queries a .. b ranked on stream s: uploads, kernels and the copies of the ragged results to idx_out / score_out
// (at out_ptr[a]).  The device sees the chunk alone: cptr = indptr - indptr[a], then out_ptr - out_ptr[a]; qlist = the
// chunk-local indices of its non-empty queries grouped by kernel -- the four LDS sizes, then the rows of the slab.
//   lds(N, n, qlist)                     launches the caller's LDS kernel of size N (a std::integral_constant) on n queries
//   fill_slab(h_rows, d_rows, rows, lmax) queues what fills r.slab (rows, lmax) -- row i the scores of query h_rows[i]'s
//                                        list, in list order, and behind them a padding that ranks last -- and returns a code
//   raw                                  the order and the form of the emitted scores (rank_rows_full)
// counts: += {lists ranked by the LDS kernels, by the slab path}.  r grows to this chunk's sizes, so nothing queued may still
// read it, and its host staging is read until the caller has synchronised s: the caller does so before the next chunk.
template <typename Lds, typename FillSlab>
static int rank_lists_chunk(hipStream_t s, ListScratch& r, const int64_t* indptr, const int32_t* ents, const int64_t* out_ptr,
                            int64_t a, int64_t b, int32_t k, bool raw, Lds&& lds, FillSlab&& fill_slab, int32_t* idx_out,
                            float* score_out, int64_t counts[2]) {
    const int64_t Qc = b - a, e0 = indptr[a], o0 = out_ptr[a], pairs = indptr[b] - e0, outs = out_ptr[b] - o0;
    if (pairs == 0) return 0;                  // (a chunk of empty lists)
    std::vector<int64_t>& cptr = r.h_cptr;
    std::vector<int32_t>& qlist = r.h_qlist;
    cptr.resize((size_t)(2 * (Qc + 1)));
    for (int64_t q = 0; q <= Qc; ++q) { cptr[(size_t)q] = indptr[a + q] - e0; cptr[(size_t)(Qc + 1 + q)] = out_ptr[a + q] - o0; }
    int64_t cnt[5] = {0, 0, 0, 0, 0}, at[5], fill[5], lmax = 0;
    auto klass = [&](int64_t q) { const int64_t len = cptr[(size_t)q + 1] - cptr[(size_t)q]; return len > kRankLdsMax ? 4 : len <= 1024 ? 0 : len <= 2048 ? 1 : len <= 4096 ? 2 : 3; };
    for (int64_t q = 0; q < Qc; ++q) {
        cnt[klass(q)] += cptr[(size_t)q + 1] > cptr[(size_t)q];
        lmax = std::max(lmax, cptr[(size_t)q + 1] - cptr[(size_t)q]);
    }
    at[0] = 0;
    for (int i = 1; i < 5; ++i) at[i] = at[i - 1] + cnt[i - 1];
    for (int i = 0; i < 5; ++i) fill[i] = at[i];
    const int64_t nq = at[4] + cnt[4];
    qlist.assign((size_t)nq, 0);
    for (int64_t q = 0; q < Qc; ++q)
        if (cptr[(size_t)q + 1] > cptr[(size_t)q]) qlist[(size_t)fill[klass(q)]++] = (int32_t)q;
    SERT_TRY(r.cptr.reserve(2 * (Qc + 1)));
    SERT_TRY(r.ents.reserve(pairs));
    SERT_TRY(r.qlist.reserve(nq));
    SERT_TRY(r.idx.reserve(outs));
    SERT_TRY(r.val.reserve(outs));
    SERT_HIP(hipMemcpyAsync(r.cptr.p, cptr.data(), cptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SERT_HIP(hipMemcpyAsync(r.ents.p, ents + e0, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SERT_HIP(hipMemcpyAsync(r.qlist.p, qlist.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (cnt[0]) lds(std::integral_constant<int, 1024>(), (unsigned)cnt[0], r.qlist.p + at[0]);
    if (cnt[1]) lds(std::integral_constant<int, 2048>(), (unsigned)cnt[1], r.qlist.p + at[1]);
    if (cnt[2]) lds(std::integral_constant<int, 4096>(), (unsigned)cnt[2], r.qlist.p + at[2]);
    if (cnt[3]) lds(std::integral_constant<int, kRankLdsMax>(), (unsigned)cnt[3], r.qlist.p + at[3]);
    if (cnt[4]) {
        // the lists beyond LDS: their scores in a padded (rows, lmax) slab, its rows ordered by the counting-sort passes as
        // POSITIONS in the list (stable: equal scores stay in list order, which is entity order), mapped back to entities
        const int rows = (int)cnt[4], lm = (int)lmax, kkc = k < 0 ? lm : (int)std::min<int64_t>(k, lmax);
        SERT_TRY(r.slab.reserve((int64_t)rows * lm));
        SERT_TRY(r.pos.reserve((int64_t)rows * kkc));
        SERT_TRY(r.pval.reserve((int64_t)rows * kkc));
        SERT_TRY(rank_scratch_reserve(r.sort, (int64_t)rows * lm));
        SERT_TRY(fill_slab(qlist.data() + at[4], r.qlist.p + at[4], rows, lm));
        SERT_TRY(rank_rows_full(s, RANK_CSORT, raw, r.slab.p, rows, lm, kkc, r.sort, r.pos.p, r.pval.p));
        launch(rerank_compact, dim3(grid_for((int64_t)rows * kkc)), dim3(256), 0, s, r.pos.p, r.pval.p, rows, kkc,
               r.qlist.p + at[4], r.ents.p, r.cptr.p, r.cptr.p + Qc + 1, r.idx.p, r.val.p);
    }
    SERT_HIP(hipGetLastError());
    SERT_HIP(hipMemcpyAsync(idx_out + o0, r.idx.p, (size_t)outs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipMemcpyAsync(score_out + o0, r.val.p, (size_t)outs * sizeof(float), hipMemcpyDeviceToHost, s));
    counts[0] += at[4]; counts[1] += cnt[4];
    return 0;
}
