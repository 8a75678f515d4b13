// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): C ABI: the query-time scorer (normalise, bf16 prefilter, exact re-scoring, top-k), pinned host memory.

// streams, events and the table buffers of a scorer for a (V, dim) entity table; the table itself comes from scorer_load_table
static int scorer_alloc(int device, int64_t V, int32_t dim, sert_scorer** out) {
    SERT_HIP(hipSetDevice(device));
    sert_scorer* sc = new sert_scorer();
    *out = sc;                    // (set first: a caller that fails below destroys what was made so far)
    sc->device = device;
    sc->V = V;
    sc->dim = dim;
    SERT_HIP(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
    SERT_HIP(hipStreamCreateWithFlags(&sc->stream2, hipStreamNonBlocking));
    SERT_HIP(hipEventCreateWithFlags(&sc->ev_ready, hipEventDisableTiming));
    SERT_HIP(hipEventCreateWithFlags(&sc->ev_done, hipEventDisableTiming));
    SERT_TRY(dmalloc(&sc->E, (size_t)V * dim));
    // large tables: bf16 copy for the prefilter GEMM (SERT_SCORE_FP32=1 keeps the fp32 filter)
    static const bool fp32_only = knob("SERT_SCORE_FP32") != nullptr;
    sc->bf16 = !fp32_only && V >= 32768 && dim % 4 == 0;
    if (sc->bf16) {
        sc->kp = (int)round_up(dim, 32);
        SERT_TRY(dmalloc(&sc->E16, (size_t)V * sc->kp));
    }
    return 0;
}

// (Re)load the entity table from `entities` (host or device, un-normalised, not modified): copy, L2-normalise, bf16 copy --
// enqueued on stream s, which the caller synchronises before the scorer's own streams use the table.
static int scorer_load_table(sert_scorer* sc, const float* entities, hipMemcpyKind kind, hipStream_t s) {
    const int64_t V = sc->V;
    const int dim = sc->dim;
    SERT_HIP(hipMemcpyAsync(sc->E, entities, (size_t)V * dim * sizeof(float), kind, s));
    launch(l2_normalize_rows, dim3(cdiv(V, 4)), dim3(256), 0, s, sc->E, V, dim);
    if (sc->bf16)
        launch(to_bf16_rows, dim3(grid_for(V * sc->kp)), dim3(256), 0, s, sc->E, V, dim,
               sc->kp, sc->E16);
    sc->bf16_demoted = false;     // (a verdict on the previous table's rows)
    return 0;
}

int sert_scorer_create(int device, const float* entities, int64_t V, int32_t dim, sert_scorer** out) {
    if (!entities || !out) SERT_FAIL("null argument");
    if (V <= 0 || dim <= 0) SERT_FAIL("bad sizes");
    sert_scorer* sc = nullptr;
    auto body = [&]() -> int {
        SERT_TRY(scorer_alloc(device, V, dim, &sc));
        SERT_TRY(scorer_load_table(sc, entities, hipMemcpyHostToDevice, sc->stream));
        SERT_HIP(hipStreamSynchronize(sc->stream));
        return 0;
    };
    const int rc = body();
    if (rc != 0) {
        const std::string keep = g_last_error;
        sert_scorer_destroy(sc);
        g_last_error = keep;
        return rc;
    }
    *out = sc;
    return 0;
}

int sert_scorer_destroy(sert_scorer* sc) {
    if (!sc) return 0;
    (void)hipSetDevice(sc->device);
    (void)hipFree(sc->E); (void)hipFree(sc->E16);
    sc->P.release(); sc->S.release(); sc->val.release(); sc->idx.release();
    sc->Ss.release(); sc->thr.release(); sc->cand.release(); sc->cnt.release(); sc->nflag.release(); sc->flag_list.release();
    sc->Pc.release(); sc->idx_c.release(); sc->val_c.release(); sc->P16.release();
    sc->rP.release(); sc->lists.release(); sc->csptr.release();
    for (int b = 0; b < 2; ++b) {
        sc->ridx[b].release(); sc->rval[b].release();
        if (sc->ev_rsorted[b]) (void)hipEventDestroy(sc->ev_rsorted[b]);
        if (sc->ev_rcopy0[b]) (void)hipEventDestroy(sc->ev_rcopy0[b]);
        if (sc->ev_rcopied[b]) (void)hipEventDestroy(sc->ev_rcopied[b]);
    }
    if (sc->ev_ready) (void)hipEventDestroy(sc->ev_ready);
    if (sc->ev_done) (void)hipEventDestroy(sc->ev_done);
    if (sc->stream2) (void)hipStreamDestroy(sc->stream2);
    if (sc->stream) (void)hipStreamDestroy(sc->stream);
    delete sc;
    return 0;
}

// SERT_SCORE_BIG_TILE=1 (opt-in, measured slower at d_e = 128 -- DESIGN.md): score through
// gemm_big.h (256x256 tiles, one wave per SIMD).  Both the fused path and its exact fallback
// then use that kernel, so a row's scores never depend on which path produced them.
static int scorer_big_tile(const sert_scorer* sc) {   // 0 no, 1 = 256x256, 2 = 256x128 (two workgroups per CU)
#ifdef SERT_VARIANTS
    static const int big_tile = variant_knob("SERT_SCORE_BIG_TILE") ? atoi(variant_knob("SERT_SCORE_BIG_TILE")) : 0;
    return (sc->V >= 32768 && gemm_big_ok(sc->dim, sc->dim, sc->dim)) ? big_tile : 0;
#else
    (void)sc;
    return 0;
#endif
}

// Materialising path: (QT, V) cosine slabs + per-row selection, for a device-resident
// block of normalised projections.  Query tiles alternate between two streams; on return
// everything is ordered on sc->stream.
static int scorer_topk_materialised(sert_scorer* sc, const float* P, int64_t Q, int k, int32_t* idx,
                                    float* val) {
    hipStream_t s = sc->stream;
    const int64_t V = sc->V;
    const int dim = sc->dim;
    static const int64_t slab_elems = [] {
        const char* e = variant_knob("SERT_SCORE_SLAB_MB");   // tuning knob
        const int64_t mb = e ? atoll(e) : 0;
        return mb > 0 ? (mb << 20) / 4 : ((int64_t)1 << 27);
    }();
    // query tile: bounds one materialised score slab to ~0.5 GiB (two slabs alternate)
    const int64_t QT = std::min<int64_t>(Q, std::max<int64_t>(128, slab_elems / V / 128 * 128));
    if (sc->S.cap < 2 * QT * V) SERT_HIP(hipStreamSynchronize(s));      // (reserve does not synchronise)
    SERT_TRY(sc->S.reserve(2 * QT * V));
    SERT_HIP(hipEventRecord(sc->ev_ready, s));
    SERT_HIP(hipStreamWaitEvent(sc->stream2, sc->ev_ready, 0));
    int t = 0;
    for (int64_t q0 = 0; q0 < Q; q0 += QT, ++t) {
        const int64_t qn = std::min(QT, Q - q0);
        hipStream_t st = (t & 1) ? sc->stream2 : s;
        float* S = sc->S.p + (size_t)(t & 1) * QT * V;
        // S = P.E^T  (cosines), then per-row selection
        // (same kernel family as the fused path, so a row's scores do not depend on the path)
#ifdef SERT_VARIANTS
        if (scorer_big_tile(sc))
            launch_gemm_big_nt(st, P + q0 * dim, sc->E, S, (int)qn, (int)V, dim, dim, dim, (int)V, scorer_big_tile(sc) == 2);
        else
#endif
            launch_gemm<false, true, EPI_STORE>(st, P + q0 * dim, sc->E, S, nullptr, (int)qn, (int)V, dim,
                                                dim, dim, (int)V);
        launch(topk_rows<false>, dim3((unsigned)qn), dim3(256), 0, st, S, (int)V, k, idx + q0 * k,
               val + q0 * k, (float*)nullptr);
        if (sc->bf16) {   // same exact_dot scores and order as the bf16-prefiltered path reports
            int sn = 2;
            while (sn < k) sn <<= 1;
            launch(rescore_topk_rows, dim3((unsigned)qn), dim3(256), (size_t)sn * sizeof(unsigned long long),
                   st, P + q0 * dim, sc->E, dim, k, idx + q0 * k, val + q0 * k, nullptr);
        }
    }
    SERT_HIP(hipEventRecord(sc->ev_done, sc->stream2));
    SERT_HIP(hipStreamWaitEvent(s, sc->ev_done, 0));
    return 0;
}

// Fused path (kernels_score.h): sampled thresholds, GEMM with a filtering epilogue,
// selection from the candidate lists; flagged rows are redone by the materialising path.
// proj / idx_out / score_out: the caller's arrays, all three on the host or (dev) all three on the
// scorer's device.  The projections are brought in chunk by chunk and each chunk's results are
// copied out while later chunks compute; *copied_out tells the caller that the output arrays are
// complete (no row needed the exact fallback).  The kernels do not depend on where the arrays live.
static int scorer_topk_fused(sert_scorer* sc, const float* proj, int64_t Q, int k, int rs, int32_t* idx_out,
                             float* score_out, bool* copied_out, bool dev) {
    *copied_out = false;
    const hipMemcpyKind kind_in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind kind_out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    hipStream_t s = sc->stream;
    const int64_t V = sc->V;
    const int dim = sc->dim;
    const int64_t Vs = cdiv(V, kScoreStride);
    // Query chunks of <= 8192 rows alternate between two streams, each with its own set of
    // scratch buffers: the selection kernel of one chunk (latency / random-row bound) runs under
    // the filter GEMM of the next (VALU / L2 bound).  An even number of equal chunks.
    static const int64_t chunk_rows = variant_knob("SERT_SCORE_CHUNK") ? atoll(variant_knob("SERT_SCORE_CHUNK")) : 8192;   // tuning knob
    const int64_t nchunks = Q <= 1024 ? 1 : 2 * cdiv(Q, 2 * chunk_rows);
    const int64_t QT = std::min<int64_t>(Q, round_up(cdiv(Q, nchunks), 128));
    SERT_TRY(sc->Ss.reserve(2 * QT * Vs));
    // per-(row, 64-entity group) candidate lists: 8 slots for ~0.5 expected entries per
    // group (k <= 128), 16 beyond
    const int ngroups = 2 * cdiv((int)V, GN);
    const int gcap = k <= 128 ? 8 : 16;
    SERT_TRY(sc->thr.reserve(2 * QT));
    const int64_t cand_set = QT * ngroups * gcap, cnt_set = QT * ngroups;
    SERT_TRY(sc->cand.reserve(2 * cand_set));
    SERT_TRY(sc->cnt.reserve(2 * QT * ngroups * 16 / 8));   // sized for either gcap
    SERT_TRY(sc->flag_list.reserve(2 * Q));   // the list, and behind it (at Q) one flag per row (topk_from_groups)
    SERT_TRY(sc->nflag.reserve(1));
    int* const row_flags = sc->flag_list.p + Q;
    // the bf16 prefilter needs a gap of 2 delta between the k-th score and the filter threshold;
    // a table whose rows mostly lack it (very high d_e, heavy ties) is scored in fp32 from then on
    const bool use_bf16 = sc->bf16 && !sc->bf16_demoted;
    if (use_bf16) SERT_TRY(sc->P16.reserve(2 * QT * sc->kp));
    SERT_HIP(hipMemsetAsync(sc->nflag.p, 0, sizeof(int), s));
    SERT_HIP(hipEventRecord(sc->ev_ready, s));           // nflag zeroed, earlier work on s done
    SERT_HIP(hipStreamWaitEvent(sc->stream2, sc->ev_ready, 0));
    auto copy_out = [&](int64_t q0, int64_t qn, hipStream_t st) {   // (host, pageable: returns when done; device: asynchronous on st -- ev_done and the synchronisation of s below join both streams before this function returns)
        hipError_t e = hipMemcpyAsync(idx_out + q0 * k, sc->idx.p + q0 * k, (size_t)qn * k * sizeof(int32_t), kind_out, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(score_out + q0 * k, sc->val.p + q0 * k, (size_t)qn * k * sizeof(float), kind_out, st);
        return e;
    };
    int64_t t = 0;
    for (int64_t q0 = 0; q0 < Q; q0 += QT, ++t) {
        const int64_t qn = std::min(QT, Q - q0);
        const int set = (int)(t & 1);
        hipStream_t st = set ? sc->stream2 : s;
        float* Pw = sc->P.p + q0 * dim;
        SERT_HIP(hipMemcpyAsync(Pw, proj + q0 * dim, (size_t)qn * dim * sizeof(float), kind_in, st));
        launch(l2_normalize_rows, dim3(cdiv(qn, 4)), dim3(256), 0, st, Pw, qn, dim);
        const float* P = Pw;
        float* Ss = sc->Ss.p + (size_t)set * QT * Vs;
        float* thr = sc->thr.p + (size_t)set * QT;
        unsigned long long* cand = sc->cand.p + (size_t)set * cand_set;
        unsigned char* cnt = sc->cnt.p + (size_t)set * cnt_set;
        uint16_t* P16 = use_bf16 ? sc->P16.p + (size_t)set * QT * sc->kp : nullptr;
        SERT_HIP(hipMemsetAsync(cnt, 0, (size_t)qn * ngroups, st));
        // 1. cosines against every kScoreStride-th entity; threshold = rs-th best of the sample
        // (bf16 scorer: approximate sample scores are as good for choosing a threshold)
        if (use_bf16) {
            launch(to_bf16_rows, dim3(grid_for(qn * sc->kp)), dim3(256), 0, st, P, qn, dim, sc->kp, P16);
            launch_score_sample_bf16(st, P16, sc->E16, Ss, (int)qn, (int)Vs, sc->kp, kScoreStride);
        } else
            launch_gemm<false, true, EPI_STORE>(st, P, sc->E, Ss, nullptr, (int)qn, (int)Vs, dim, dim,
                                                dim * kScoreStride, (int)Vs);
        if (rs <= 64 && Vs >= 2048)
            launch(approx_kth_rows, dim3((unsigned)qn), dim3(256), 0, st, Ss, (int)Vs, rs, thr);
        else
            launch(kth_largest_rows, dim3((unsigned)qn), dim3(256), 0, st, Ss, (int)Vs, rs, thr);
        // 2. full GEMM, filtering epilogue
        if (use_bf16) {
            launch_score_filter_bf16(st, P16, sc->E16, thr, (uint32_t*)cand, cnt, ngroups, gcap, (int)qn, (int)V, sc->kp);
        } else
#ifdef SERT_VARIANTS
        if (scorer_big_tile(sc))
            launch_gemm_big_filter(st, P, sc->E, thr, cand, cnt, ngroups, gcap, (int)qn, (int)V, dim, dim, dim,
                                   scorer_big_tile(sc) == 2);
        else
#endif
            launch_gemm<false, true, EPI_FILTER>(st, P, sc->E, nullptr, thr, (int)qn, (int)V, dim, dim, dim,
                                                 (int)V, 1, 0, 0, cand, cnt, gcap);
        // 3. selection from the candidate lists
        // candidate capacity: expected 2k+400, sigma ~ 16 sqrt(rs): the next power of two above +6 sigma
        int ccap = 1024;
        while (ccap < 2 * k + 400 + 6 * 16 * (int)ceilf(sqrtf((float)rs)) && ccap < kCandCap) ccap <<= 1;
        if (use_bf16)
            launch(topk_from_groups_rescore, dim3((unsigned)qn), dim3(256), (size_t)ccap * sizeof(unsigned long long), st,
                   (const uint32_t*)cand, cnt, ngroups, gcap, k, sc->idx.p + q0 * k, sc->val.p + q0 * k, (int)q0,
                   sc->nflag.p, sc->flag_list.p, ccap, P, sc->E, dim, thr, bf16_delta(dim));
        else {
            launch(topk_from_groups, dim3((unsigned)qn), dim3(256), (size_t)ccap * sizeof(unsigned long long), st,
                   cand, cnt, ngroups, gcap, k, sc->idx.p + q0 * k, sc->val.p + q0 * k, (int)q0,
                   sc->nflag.p, sc->flag_list.p, ccap, row_flags);
            if (sc->bf16) {   // demoted table: its scores stay the exact_dot ones every other path of this scorer reports
                int sn = 2;
                while (sn < k) sn <<= 1;
                launch(rescore_topk_rows, dim3((unsigned)qn), dim3(256), (size_t)sn * sizeof(unsigned long long),
                       st, P, sc->E, dim, k, sc->idx.p + q0 * k, sc->val.p + q0 * k, row_flags + q0);
            }
        }
        // results of the previous chunk (other stream) travel while this one computes
        if (t >= 1) SERT_HIP(copy_out(q0 - QT, QT, set ? s : sc->stream2));
    }
    {
        const int64_t q_last = (t - 1) * QT;
        SERT_HIP(copy_out(q_last, Q - q_last, ((t - 1) & 1) ? sc->stream2 : s));
    }
    SERT_HIP(hipEventRecord(sc->ev_done, sc->stream2));
    SERT_HIP(hipStreamWaitEvent(s, sc->ev_done, 0));
    int nf = 0;
    SERT_HIP(hipMemcpyAsync(&nf, sc->nflag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    SERT_HIP(hipStreamSynchronize(s));
    sc->path_counts[0] += 1; sc->path_counts[1] += use_bf16 ? 1 : 0; sc->path_counts[2] += t; sc->path_counts[3] += nf;
    if (nf == 0) { *copied_out = true; return 0; }
    if (use_bf16 && (int64_t)nf * 4 > Q && Q >= 64) sc->bf16_demoted = true;
    // rows the sample misjudged: recompute exactly (ascending order, for reproducibility)
    std::vector<int> list((size_t)nf);
    SERT_HIP(hipMemcpy(list.data(), sc->flag_list.p, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost));
    std::sort(list.begin(), list.end());
    SERT_HIP(hipMemcpyAsync(sc->flag_list.p, list.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
    SERT_TRY(sc->Pc.reserve((int64_t)nf * dim));
    SERT_TRY(sc->idx_c.reserve((int64_t)nf * k));
    SERT_TRY(sc->val_c.reserve((int64_t)nf * k));
    launch(gather_rows_f32, dim3(grid_for((int64_t)nf * dim)), dim3(256), 0, s, sc->P.p,
           sc->flag_list.p, nf, dim, sc->Pc.p);
    SERT_TRY(scorer_topk_materialised(sc, sc->Pc.p, nf, k, sc->idx_c.p, sc->val_c.p));
    launch(scatter_topk_rows, dim3(grid_for((int64_t)nf * k)), dim3(256), 0, s, sc->idx_c.p,
           sc->val_c.p, sc->flag_list.p, nf, k, sc->idx.p, sc->val.p);
    return 0;
}

// sert_scorer_topk on the caller's host arrays, or (dev) on arrays of the scorer's device (sert_reval_run: the projections
// never leave it).  Same path choice and kernels either way.
static int scorer_topk_io(sert_scorer* sc, const float* proj, int64_t Q, int32_t k, int32_t* idx_out, float* score_out, bool dev) {
    if (!sc || !proj || !idx_out || !score_out) SERT_FAIL("null argument");
    if (Q < 0 || k <= 0) SERT_FAIL("bad sizes");
    if (k > sc->V) SERT_FAIL("k exceeds the number of entities");
    if (k > kTopKMax) SERT_FAIL("k > 1024 is not supported");
    if (Q == 0) return 0;
    SERT_HIP(hipSetDevice(sc->device));
    hipStream_t s = sc->stream;
    const int64_t V = sc->V;
    const int dim = sc->dim;
    SERT_TRY(sc->P.reserve(Q * dim));
    SERT_TRY(sc->val.reserve(Q * k));
    SERT_TRY(sc->idx.reserve(Q * k));
    // fused path for large entity tables: the sample must be big enough for a stable
    // threshold: rank rs among the V/16 sampled entities, i.e. an expected 2k+400 (std ~
    // sqrt(rs)*16) candidates of V -- at k=100: 608 +- 99, >= k at 5 sigma, <= 1024 at 4
    const int rs = cdiv(2 * k + 400, kScoreStride);
    static const bool never_fuse = knob("SERT_SCORE_MATERIALISE") != nullptr;   // cross-check knob
    const bool fused = !never_fuse && V >= 32768 && dim % 4 == 0 && rs <= kTopKMax &&
                       cdiv(V, kScoreStride) >= 8 * (int64_t)rs;
    bool copied = false;
    if (fused) SERT_TRY(scorer_topk_fused(sc, proj, Q, k, rs, idx_out, score_out, &copied, dev));
    else {
        SERT_HIP(hipMemcpyAsync(sc->P.p, proj, (size_t)Q * dim * sizeof(float), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        launch(l2_normalize_rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, sc->P.p, Q, dim);
        SERT_TRY(scorer_topk_materialised(sc, sc->P.p, Q, k, sc->idx.p, sc->val.p));
        sc->path_counts[4] += Q;
    }
    SERT_HIP(hipGetLastError());
    if (copied) return 0;
    const hipMemcpyKind kind_out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    SERT_HIP(hipMemcpyAsync(idx_out, sc->idx.p, (size_t)Q * k * sizeof(int32_t), kind_out, s));
    SERT_HIP(hipMemcpyAsync(score_out, sc->val.p, (size_t)Q * k * sizeof(float), kind_out, s));
    SERT_HIP(hipStreamSynchronize(s));
    return 0;
}

int sert_scorer_topk(sert_scorer* sc, const float* proj, int64_t Q, int32_t k, int32_t* idx_out, float* score_out) {
    return scorer_topk_io(sc, proj, Q, k, idx_out, score_out, false);
}

// S (qn, V) = the cosines of qn normalised projections P against the table, on stream st: the exact_dot32 ones (`exact`: what
// the top-k of a bf16-prefiltered table reports) or the GEMM's.  The one place sert_scorer_scores, sert_scorer_cosines and
// sert_scorer_rank fill a slab, so the three agree bit for bit.
static void scorer_cosine_slab(sert_scorer* sc, hipStream_t st, const float* P, int64_t qn, float* S, bool exact) {
    const int64_t V = sc->V;
    const int dim = sc->dim;
    if (exact)
        launch(exact_cosine_rows, dim3((unsigned)std::min<int64_t>(cdiv(V, 8), 1024), (unsigned)qn), dim3(256), 0, st,
               P, sc->E, V, dim, S);
    else
        launch_gemm<false, true, EPI_STORE>(st, P, sc->E, S, nullptr, (int)qn, (int)V, dim, dim, dim, (int)V);
}

// every entity's value for Q queries: (cos + 1)/2 of the GEMM's cosine, or (raw) the cosine itself AS sert_scorer_topk ORDERS
// AND REPORTS IT -- the exact_dot32 one for a bf16-prefiltered table, the GEMM's otherwise
static int scorer_all(sert_scorer* sc, const float* proj, int64_t Q, float* score_out, bool raw) {
    if (!sc || !proj || !score_out) SERT_FAIL("null argument");
    if (Q <= 0) return 0;
    SERT_HIP(hipSetDevice(sc->device));
    hipStream_t s = sc->stream;
    const int64_t V = sc->V;
    const int dim = sc->dim;
    const int64_t QT = std::min<int64_t>(Q, std::max<int64_t>(128, ((int64_t)1 << 28) / V / 128 * 128));
    SERT_TRY(sc->P.reserve(Q * dim));
    SERT_TRY(sc->S.reserve(QT * V));
    SERT_HIP(hipMemcpyAsync(sc->P.p, proj, (size_t)Q * dim * sizeof(float), hipMemcpyHostToDevice, s));
    launch(l2_normalize_rows, dim3(cdiv(Q, 4)), dim3(256), 0, s, sc->P.p, Q, dim);
    for (int64_t q0 = 0; q0 < Q; q0 += QT) {
        const int64_t qn = std::min(QT, Q - q0);
        scorer_cosine_slab(sc, s, sc->P.p + q0 * dim, qn, sc->S.p, raw && sc->bf16);
        if (!raw) launch(cos_to_score, dim3(grid_for(qn * V)), dim3(256), 0, s, sc->S.p, (size_t)(qn * V));
        SERT_HIP(hipMemcpyAsync(score_out + q0 * V, sc->S.p, (size_t)qn * V * sizeof(float), hipMemcpyDeviceToHost, s));
        SERT_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

int sert_scorer_scores(sert_scorer* sc, const float* proj, int64_t Q, float* score_out) {
    return scorer_all(sc, proj, Q, score_out, false);
}
int sert_scorer_cosines(sert_scorer* sc, const float* proj, int64_t Q, float* cos_out) {
    return scorer_all(sc, proj, Q, cos_out, true);
}

int sert_host_alloc(void** out, size_t bytes) {
    if (!out || bytes == 0) SERT_FAIL("bad argument");
    *out = nullptr;
    static const int flags = variant_knob("SERT_PIN_FLAGS") ? atoi(variant_knob("SERT_PIN_FLAGS")) : (int)hipHostMallocDefault;   // tuning knob
    SERT_HIP(hipHostMalloc(out, bytes, (unsigned)flags));
    return 0;
}
int sert_host_free(void* p) {
    if (p) SERT_HIP(hipHostFree(p));
    return 0;
}

int sert_score_topk(int device, const float* entities, int64_t V, int32_t dim, const float* proj,
                    int64_t Q, int32_t k, int32_t* idx_out, float* score_out) {
    sert_scorer* sc = nullptr;
    SERT_TRY(sert_scorer_create(device, entities, V, dim, &sc));
    const int rc = sert_scorer_topk(sc, proj, Q, k, idx_out, score_out);
    sert_scorer_destroy(sc);
    return rc;
}
