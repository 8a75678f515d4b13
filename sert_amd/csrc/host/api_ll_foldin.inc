// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: folding unseen entities
// into a trained loglinear model (include/sert_hip_ll_foldin.h: sert_ll_foldin_*; kernels_ll_foldin.h).  Like sert_foldin the
// handle copies the model's parameters when it is created and runs on a stream of its own.

struct sert_ll_foldin : FoldLl {
    sert_ll_foldin_config cfg;
    int N = 0;                           // FoldLl::Ve: the FROZEN columns V_f; N: the trainable ones Nt (the kernels' V_e and N)
    // the public columns: Ve_pub trained entities of the model, of which R are refreshed (slots [0, R) of the N trainable
    // columns), and N - R new ones; internal_of (Ve_pub + N - R): public column -> internal column (ll_label_remap.h)
    int Ve_pub = 0, R = 0;
    std::vector<int32_t> internal_of;
    // (the frozen snapshot's W (d, Ve) and b (Ve) are null when every trained column is refreshed)
    // the new columns Wn (d, N) and biases bn (N), Adadelta's accumulators, the gradients
    float *Wn = nullptr, *bn = nullptr, *accu_w = nullptr, *accu_b = nullptr, *delta_w = nullptr, *delta_b = nullptr;
    float *g_w = nullptr, *g_b = nullptr;
    // ---- the upload (FoldBase: M instances; FoldLl: the labels, INTERNAL columns in [0, V_f + Nt), and w) ----
    int64_t D = 0;                       // distinct words of the upload
    float* G = nullptr;                  // (D, d) = R_w[distinct words]
    float* Zold = nullptr;               // (D, V_e) the logit cache
    float2* stat = nullptr;              // (D) (max, sum exp) of a cache row
    int32_t* Lb = nullptr;               // per batch: the sorted distinct words of the batch, as rows of the cache
    int32_t* tok = nullptr;              // (batches, B, n): a token's slot in its batch's list
    int32_t* wptr = nullptr;             // per batch: U + 1 offsets into wpos
    int32_t* wpos = nullptr;             // (batches, B n): the token positions of each word of the batch, ascending
    std::vector<int64_t> lb_off, ptr_off;    // where a batch's Lb / wptr start
    std::vector<int32_t> U;                  // a batch's number of distinct words
    // per-step scratch, sized by the upload's largest U
    float *Gb = nullptr, *Zn = nullptr, *lse = nullptr, *dZ = nullptr, *dZu = nullptr, *part = nullptr;
    // (FoldLl::red_sq: [kOptBlocks] sums of squares of Wn, then [kOptBlocks] of bn, which are not in the loss)
};

static void llf_free_upload(sert_ll_foldin* f) {
    fold_free_labels(f);
    for (void* p : {(void*)f->G, (void*)f->Zold, (void*)f->stat, (void*)f->Lb, (void*)f->tok, (void*)f->wptr, (void*)f->wpos, (void*)f->Gb,
                    (void*)f->Zn, (void*)f->lse, (void*)f->dZ, (void*)f->dZu, (void*)f->part})
        (void)hipFree(p);
    f->G = nullptr; f->Zold = nullptr; f->stat = nullptr; f->Lb = nullptr; f->tok = nullptr;
    f->wptr = nullptr; f->wpos = nullptr; f->Gb = nullptr; f->Zn = nullptr; f->lse = nullptr; f->dZ = nullptr; f->dZu = nullptr;
    f->part = nullptr;
    f->lb_off.clear(); f->ptr_off.clear(); f->U.clear();
    f->M = 0; f->D = 0;
}

int sert_ll_foldin_destroy(sert_ll_foldin* f) {
    if (!f) return 0;
    return fold_destroy(f, llf_free_upload, {f->rw, f->W, f->b, f->Wn, f->bn, f->accu_w, f->accu_b, f->delta_w, f->delta_b, f->g_w,
                                             f->g_b, f->rowloss, f->red_sq});
}

// Both creators.  refresh == false: sert_ll_foldin_create, its arguments and its wording.  The trainable columns are SLOTS --
// the num_refresh refreshed trained columns, then the new ones -- and the handle's Ve / N are V_f / Nt of the internal column
// order (ll_label_remap.h).  num_refresh == 0: W and b are copied whole, as ever; otherwise llf_compact writes the frozen
// columns and the refreshed slots in one pass over the model's W, b.
static int llf_create(sert_ll_foldin* f, sert_model* m, bool refresh, const int32_t* refresh_ids, int32_t num_refresh,
                      int32_t num_new, const float* init_W, const float* init_b, const sert_ll_foldin_config* cfg) {
    const auto& c = m->cfg;
    // ---- validation: everything the kernels index with is checked here ----
    if (c.kind == SERT_KIND_VECTORSPACE)
        SERT_FAIL("a loglinear fold-in needs a loglinear model: a vectorspace model folds in through sert_foldin_create");
    if (c.kind != SERT_KIND_LOGLINEAR)
        SERT_FAIL("a loglinear fold-in needs a loglinear model: the full-softmax variant (SERT_KIND_VECTORSPACE_SOFTMAX) is not supported");
    if (m->comm || m->host_ar || m->world > 1)
        SERT_FAIL("a fold-in of a data-parallel model (a communicator is attached) is not supported");
    if (!refresh) {
        if (num_new < 1) SERT_FAIL("a fold-in needs at least one new entity (num_new >= 1)");
        if (!init_W) SERT_FAIL("null argument");
    } else {
        if (num_refresh < 0 || num_new < 0) SERT_FAIL("a refresh needs num_refresh >= 0 and num_new >= 0");
        if ((int64_t)num_refresh + num_new < 1) SERT_FAIL("a refresh needs at least one trainable column (num_refresh + num_new >= 1)");
        if ((num_refresh > 0) != (refresh_ids != nullptr))
            SERT_FAIL(num_refresh > 0 ? "null refresh_ids with num_refresh > 0" : "refresh_ids must be NULL when num_refresh == 0");
        if ((num_new > 0) != (init_W != nullptr))
            SERT_FAIL(num_new > 0 ? "null init_new_W with num_new > 0" : "init_new_W must be NULL when num_new == 0");
    }
    const int64_t nt = (int64_t)num_refresh + num_new;
    if (c.window_size > 32) SERT_FAIL("a loglinear fold-in supports window sizes up to 32");
    if (cfg->batch_size < 1) SERT_FAIL("a fold-in needs batch_size >= 1");
    if (!(cfg->lambda_ >= 0.f)) SERT_FAIL("regularization lambda must be >= 0");
    if (!(cfg->rho >= 0.f && cfg->rho < 1.f) || !(cfg->eps > 0.f)) SERT_FAIL("Adadelta needs 0 <= rho < 1 and eps > 0");
    if ((int64_t)c.num_entities + num_new > INT32_MAX) SERT_FAIL("more than 2^31 - 1 columns in the extended model");
    if ((int64_t)cfg->batch_size * c.window_size * nt > INT32_MAX)
        SERT_FAIL(refresh ? "batch_size * window_size * (num_refresh + num_new) > 2^31 - 1" : "batch_size * window_size * num_new > 2^31 - 1");
    if ((int64_t)c.word_dim * nt > INT32_MAX)
        SERT_FAIL(refresh ? "word_dim * (num_refresh + num_new) > 2^31 - 1" : "word_dim * num_new > 2^31 - 1");
    switch (ll_layout(c.num_entities, num_new, refresh_ids, num_refresh, f->internal_of)) {
        case LL_LAYOUT_ID_RANGE: SERT_FAIL("refresh id out of range [0, num_entities)");
        case LL_LAYOUT_ID_DUPLICATE: SERT_FAIL("duplicate refresh id");
        default: break;
    }
    SERT_HIP(hipSetDevice(c.device));
    f->device = c.device; f->cfg = *cfg;
    f->Vw = c.vocab_size; f->Ve_pub = c.num_entities; f->R = num_refresh; f->d = c.word_dim; f->n = c.window_size;
    f->Ve = c.num_entities - num_refresh; f->N = (int)nt;
    const int R = f->R, Vf = f->Ve, Nt = f->N, d = f->d;
    const size_t n_w = (size_t)d * Nt, n_b = (size_t)Nt;
    SERT_TRY(fold_settle_model(m, false));
    SERT_TRY(fold_snapshot(m, &f->rw, m->rw, m->n_rw, m->n_rw));
    if (R == 0) {
        SERT_TRY(fold_snapshot(m, &f->W, m->W, m->n_w, m->n_w));
        SERT_TRY(fold_snapshot(m, &f->b, m->b, m->n_b, m->n_b));
    } else {
        SERT_TRY(dmalloc(&f->W, (size_t)d * Vf));      // (V_f == 0: no allocation, the pointers stay null and are never read)
        SERT_TRY(dmalloc(&f->b, (size_t)Vf));
    }
    SERT_HIP(hipStreamCreate(&f->stream));
    hipStream_t s = f->stream;
    SERT_TRY(dmalloc(&f->Wn, n_w));
    SERT_TRY(dzalloc(&f->bn, n_b, s));
    SERT_TRY(dzalloc(&f->accu_w, n_w, s));
    SERT_TRY(dzalloc(&f->accu_b, n_b, s));
    SERT_TRY(dzalloc(&f->delta_w, n_w, s));
    SERT_TRY(dzalloc(&f->delta_b, n_b, s));
    SERT_TRY(dmalloc(&f->g_w, n_w));
    SERT_TRY(dmalloc(&f->g_b, n_b));
    // the new columns [R, Nt) of Wn (d, Nt) and of bn
    if (num_new > 0) {
        if (R == 0) SERT_HIP(hipMemcpyAsync(f->Wn, init_W, n_w * sizeof(float), hipMemcpyHostToDevice, s));
        else
            SERT_HIP(hipMemcpy2DAsync(f->Wn + R, (size_t)Nt * sizeof(float), init_W, (size_t)num_new * sizeof(float),
                                      (size_t)num_new * sizeof(float), (size_t)d, hipMemcpyHostToDevice, s));
        if (init_b) SERT_HIP(hipMemcpyAsync(f->bn + R, init_b, (size_t)num_new * sizeof(float), hipMemcpyHostToDevice, s));
    }
    SERT_TRY(dmalloc(&f->rowloss, (size_t)cfg->batch_size));
    SERT_TRY(dmalloc(&f->red_sq, (size_t)2 * kOptBlocks));
    SERT_TRY(dmalloc(&f->d_loss, (size_t)3));
    int32_t* d_internal = nullptr;
    if (R > 0) {
        SERT_TRY(dmalloc(&d_internal, (size_t)f->Ve_pub));
        if (hipMemcpyAsync(d_internal, f->internal_of.data(), (size_t)f->Ve_pub * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess) {
            (void)hipFree(d_internal);
            SERT_FAIL("copying the column layout to the device failed");
        }
    }
    hipError_t e = hipStreamSynchronize(s);            // (init_W, init_b are borrowed for the call only; bn's zeros are in place)
    if (e == hipSuccess && R > 0) {
        // the frozen columns and the refreshed slots, from the model's own W and b: behind the preamble on the model's queue
        launch(llf_compact, dim3(grid_for(((int64_t)d + 1) * f->Ve_pub)), dim3(256), 0, m->stream, (const float*)m->W,
               (const float*)m->b, (const int32_t*)d_internal, f->W, f->b, f->Wn, f->bn, d, f->Ve_pub, Vf, Nt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);     // (the snapshot is complete: the model may train or go away)
    (void)hipFree(d_internal);
    SERT_HIP(e);
    return 0;
}

int sert_ll_foldin_create(sert_model* m, int32_t num_new, const float* init_W, const float* init_b,
                          const sert_ll_foldin_config* cfg, sert_ll_foldin** out) {
    refresh_gemm_choice();
    return fold_create(m, cfg, out, "sert_ll_foldin_config size mismatch (ABI)", sert_ll_foldin_destroy,
                       [&](sert_ll_foldin* f) { return llf_create(f, m, false, nullptr, 0, num_new, init_W, init_b, cfg); });
}

int sert_ll_foldin_create_refresh(sert_model* m, const int32_t* refresh_ids, int32_t num_refresh, int32_t num_new,
                                  const float* init_new_W, const float* init_new_b, const sert_ll_foldin_config* cfg,
                                  sert_ll_foldin** out) {
    refresh_gemm_choice();
    return fold_create(m, cfg, out, "sert_ll_foldin_config size mismatch (ABI)", sert_ll_foldin_destroy, [&](sert_ll_foldin* f) {
        return llf_create(f, m, true, refresh_ids, num_refresh, num_new, init_new_W, init_new_b, cfg);
    });
}

// the split-K shape of dWn = Gb^T dZu over `rows` distinct words (the loglinear step's rule, step_softmax_loglinear.inc)
static void llf_dw_splits(const sert_ll_foldin* f, int64_t rows, int* splits, int* kper) {
    const int tiles = cdiv(f->N, GN) * cdiv(f->d, GM);
    int sp = std::max(1, std::min(cdiv(rows, GK), cdiv(1024, tiles)));
    const int kp = (int)round_up((size_t)cdiv(std::max<int64_t>(rows, 1), sp), GK);
    sp = std::max(1, cdiv(rows, kp));
    *splits = sp; *kper = kp;
}

// What an upload of either label form does once its labels are known to be good: the tokens are validated; then the distinct
// words, the per-batch word lists (Lb, tok, wptr / wpos), the logit cache with llf_row_stat, and the copies of those lists, of
// the labels and of w.  Nothing of the handle is touched before every host-side check has passed.
static int llf_upload(sert_ll_foldin* f, const int32_t* x, const FoldLabels& lab, const float* w, int64_t M) {
    const int n = f->n, d = f->d, Ve = f->Ve, N = f->N, B = f->cfg.batch_size;
    for (int64_t i = 0; i < M * n; ++i)
        if (x[i] < 0 || x[i] >= f->Vw) SERT_FAIL("token id out of range [0, vocab_size)");
    // ---- the distinct words D of x (sorted) and the row of the cache of every token ----
    FoldWordTable cache;
    SERT_TRY(fold_word_table(x, M * n, f->Vw, Ve, f->cfg.max_cache_bytes, "logit cache", "distinct words", &cache));
    const std::vector<int32_t>& row_of = cache.row_of;
    const int64_t D = (int64_t)cache.words.size();
    // ---- per batch: the sorted list of its distinct words, a slot per token, the token positions per word ----
    const int64_t nb = M / B, bt = (int64_t)B * n;
    std::vector<int32_t> Lb, tok((size_t)(nb * bt)), wptr, wpos((size_t)(nb * bt)), local((size_t)D, -1), fill;
    std::vector<int64_t> lb_off((size_t)nb), ptr_off((size_t)nb);
    std::vector<int32_t> Us((size_t)nb);
    int Umax = 1;
    for (int64_t bi = 0; bi < nb; ++bi) {
        const int32_t* xb = x + (size_t)bi * bt;
        const size_t l0 = Lb.size();
        for (int64_t t = 0; t < bt; ++t) {
            const int32_t r = row_of[(size_t)xb[t]];
            if (local[(size_t)r] < 0) { local[(size_t)r] = 0; Lb.push_back(r); }
        }
        std::sort(Lb.begin() + (std::ptrdiff_t)l0, Lb.end());
        const int U = (int)(Lb.size() - l0);
        for (int u = 0; u < U; ++u) local[(size_t)Lb[l0 + u]] = u;
        lb_off[(size_t)bi] = (int64_t)l0; ptr_off[(size_t)bi] = (int64_t)wptr.size(); Us[(size_t)bi] = U;
        Umax = std::max(Umax, U);
        std::vector<int32_t> cnt((size_t)U + 1, 0);
        int32_t* tb = tok.data() + (size_t)bi * bt;
        for (int64_t t = 0; t < bt; ++t) { tb[t] = local[(size_t)row_of[(size_t)xb[t]]]; ++cnt[(size_t)tb[t] + 1]; }
        for (int u = 0; u < U; ++u) cnt[(size_t)u + 1] += cnt[(size_t)u];
        wptr.insert(wptr.end(), cnt.begin(), cnt.end());
        fill.assign(cnt.begin(), cnt.end() - 1);
        int32_t* pb = wpos.data() + (size_t)bi * bt;
        for (int64_t t = 0; t < bt; ++t) pb[fill[(size_t)tb[t]]++] = (int32_t)t;     // (ascending t within a word)
        for (int u = 0; u < U; ++u) local[(size_t)Lb[l0 + u]] = -1;
    }
    SERT_HIP(hipSetDevice(f->device));
    hipStream_t s = f->stream;
    SERT_HIP(hipStreamSynchronize(s));
    llf_free_upload(f);
    if (M == 0) return 0;
    uint32_t* dwords = nullptr;
    std::vector<float> ones;
    auto body = [&]() -> int {
        // (V_f == 0, every trained column refreshed: no cache -- Zold stays null and no kernel reads a column of it)
        SERT_TRY(fold_alloc_table(cache, &f->Zold));
        SERT_TRY(fold_upload_labels(f, lab, w, M, ones));
        SERT_TRY(dmalloc(&f->G, (size_t)D * d));
        SERT_TRY(dmalloc(&f->stat, (size_t)D));
        SERT_TRY(dmalloc(&f->Lb, std::max<size_t>(Lb.size(), 1)));
        SERT_TRY(dmalloc(&f->tok, std::max<size_t>(tok.size(), 1)));
        SERT_TRY(dmalloc(&f->wptr, std::max<size_t>(wptr.size(), 1)));
        SERT_TRY(dmalloc(&f->wpos, std::max<size_t>(wpos.size(), 1)));
        SERT_TRY(dmalloc(&dwords, (size_t)D));
        // (llf_dw_splits never gives a batch more slabs than its first guess for the largest one)
        const int max_splits = std::max(1, std::min(cdiv(Umax, GK), cdiv(1024, cdiv(N, GN) * cdiv(d, GM)))) + 1;
        SERT_TRY(dmalloc(&f->Gb, (size_t)Umax * d));
        SERT_TRY(dmalloc(&f->Zn, (size_t)Umax * N));
        SERT_TRY(dmalloc(&f->lse, (size_t)Umax));
        SERT_TRY(dmalloc(&f->dZ, (size_t)bt * N));
        SERT_TRY(dmalloc(&f->dZu, (size_t)Umax * N));
        SERT_TRY(dmalloc(&f->part, (size_t)max_splits * ((size_t)d * N + N)));
        SERT_HIP(hipMemcpyAsync(dwords, cache.words.data(), (size_t)D * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!Lb.empty()) SERT_HIP(hipMemcpyAsync(f->Lb, Lb.data(), Lb.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!tok.empty()) SERT_HIP(hipMemcpyAsync(f->tok, tok.data(), tok.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!wptr.empty()) SERT_HIP(hipMemcpyAsync(f->wptr, wptr.data(), wptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!wpos.empty()) SERT_HIP(hipMemcpyAsync(f->wpos, wpos.data(), wpos.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        // G = R_w[D]; Zold = G W + b, a slab of rows at a time so that no launch sees 2 GiB of either operand: the slabs'
        // offsets into the cache are 64 bits wide
        gather_rows(s, (const uint32_t*)dwords, f->rw, f->G, D, d);
        const int64_t slab = std::max<int64_t>(1, std::min<int64_t>(D, (((int64_t)1 << 29) - 1) / std::max(Ve, d)));
        for (int64_t r0 = 0; Ve > 0 && r0 < D; r0 += slab) {
            const int rows = (int)std::min<int64_t>(slab, D - r0);
            launch_gemm<false, false, EPI_BIAS>(s, f->G + (size_t)r0 * d, f->W, f->Zold + (size_t)r0 * Ve, f->b, rows, Ve, d, d, Ve, Ve);
        }
        launch(llf_row_stat, dim3((unsigned)D), dim3(256), 0, s, (const float*)f->Zold, Ve, f->stat);
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipStreamSynchronize(s));     // (x, the labels, w and the host lists are borrowed for the call only)
        return 0;
    };
    const int rc = body();
    (void)hipFree(dwords);
    if (rc != 0) return fold_upload_failed(f, rc, llf_free_upload);
    f->M = M; f->D = D;
    f->lb_off.swap(lb_off); f->ptr_off.swap(ptr_off); f->U.swap(Us);
    return 0;
}

static int llf_upload_check_sizes(sert_ll_foldin* f, int64_t M) {
    if (M > ((int64_t)1 << 31) - 1) SERT_FAIL("more than 2^31 - 1 fold-in instances");
    if (M * f->n > ((int64_t)1 << 31) - 1) SERT_FAIL("more than 2^31 - 1 fold-in tokens");
    return 0;
}

int sert_ll_foldin_upload(sert_ll_foldin* f, const int32_t* x, const int32_t* y, const float* w, int64_t M) {
    refresh_gemm_choice();
    if (!f || M < 0 || (M > 0 && (!x || !y))) SERT_FAIL("bad argument");
    SERT_TRY(llf_upload_check_sizes(f, M));
    // host-side validation: no kernel is launched on bad ids
    for (int64_t i = 0; i < M; ++i)
        if (y[i] < 0 || y[i] >= f->N)
            SERT_FAIL(f->R > 0 ? "fold-in label out of range [0, num_refresh + num_new): y is a slot"
                               : "fold-in label out of range [0, num_new)");
    // (a slot is the label's trainable column as the step counts it, behind the V_f frozen ones: nothing to remap)
    return llf_upload(f, x, FoldLabels{y, nullptr, nullptr, nullptr}, w, M);
}

int sert_ll_foldin_upload_csr(sert_ll_foldin* f, const int32_t* x, const int64_t* indptr, const int32_t* indices,
                              const float* data, const float* w, int64_t M) {
    refresh_gemm_choice();
    if (!f || M < 0 || (M > 0 && (!x || !indptr))) SERT_FAIL("bad argument");
    SERT_TRY(llf_upload_check_sizes(f, M));
    // host-side validation over the PUBLIC columns V_e + num_new: no kernel is launched on a bad row
    if (M > 0)
        SERT_TRY(check_csr_rows(indptr, indices, data, M, (int64_t)f->internal_of.size(),
                                "label column out of range [0, V_e + num_new) in csr_indices", INT32_MAX));
    if (f->R > 0 && M > 0 && indptr[M] > 0) {
        // public -> internal columns: a refreshed column leaves the frozen ones for the trainable tail, which llf_row_csr
        // finds by bisection at V_f, so every row is brought back to strictly increasing columns (ll_label_remap.h)
        std::vector<int32_t> cols((size_t)indptr[M]);
        std::vector<float> vals((size_t)indptr[M]);
        ll_remap_csr(indptr, indices, data, M, f->internal_of, f->Ve, cols.data(), vals.data());
        return llf_upload(f, x, FoldLabels{nullptr, indptr, cols.data(), vals.data()}, w, M);
    }
    return llf_upload(f, x, FoldLabels{nullptr, indptr, indices, data}, w, M);
}

int64_t sert_ll_foldin_num_batches(sert_ll_foldin* f) { return fold_num_batches(f); }

static int llf_check_batch(sert_ll_foldin* f, int64_t batch) {
    return fold_check_batch(f, &sert_ll_foldin::G, "sert_ll_foldin_upload", batch);
}

// the forward of batch `batch` on the handle's stream: the new logits, the tokens' log-sum-exp, the row kernel (TRAIN: dZ of
// the new columns as well); the rows' losses are left in f->rowloss
static int llf_forward(sert_ll_foldin* f, int64_t batch, bool train) {
    const int B = f->cfg.batch_size, n = f->n, d = f->d, N = f->N, U = f->U[(size_t)batch];
    hipStream_t s = f->stream;
    const int32_t* Lb = f->Lb + f->lb_off[(size_t)batch];
    const int32_t* tok = f->tok + (size_t)batch * B * n;
    // Gb = G[L_b]; Zn = Gb Wn + bn
    gather_rows(s, reinterpret_cast<const uint32_t*>(Lb), f->G, f->Gb, U, d);
    launch_gemm<false, false, EPI_BIAS>(s, f->Gb, f->Wn, f->Zn, f->bn, U, N, d, d, N, N);
    launch(llf_lse, dim3(cdiv(U, 4)), dim3(256), 0, s, f->Zn, (const float2*)f->stat, Lb, f->lse, U, N);
    const size_t row0 = (size_t)batch * B;
    auto go = [&](auto training, auto evaluation) {
        if (train)
            launch(training, dim3(B), dim3(256), 0, s, (const float*)f->Zold, (const float*)f->Zn, (const float*)f->lse, Lb, tok,
                   (const int32_t*)(f->y + row0), (const float*)(f->w + row0), f->rowloss, f->dZ, n, f->Ve, N, 1.0f / (float)B);
        else
            launch(evaluation, dim3(B), dim3(256), 0, s, (const float*)f->Zold, (const float*)f->Zn, (const float*)f->lse, Lb, tok,
                   (const int32_t*)(f->y + row0), (const float*)nullptr, f->rowloss, f->dZ, n, f->Ve, N, 1.0f / (float)B);
    };
    // label rows (sert_ll_foldin_upload_csr): the same launch shape, the batch's slice of indptr
    auto go_csr = [&](auto training, auto evaluation) {
        if (train)
            launch(training, dim3(B), dim3(256), 0, s, (const float*)f->Zold, (const float*)f->Zn, (const float*)f->lse, Lb, tok,
                   (const int64_t*)(f->indptr + row0), (const int32_t*)f->indices, (const float*)f->data, (const float*)(f->w + row0),
                   f->rowloss, f->labfix, f->dZ, n, f->Ve, N, 1.0f / (float)B);
        else
            launch(evaluation, dim3(B), dim3(256), 0, s, (const float*)f->Zold, (const float*)f->Zn, (const float*)f->lse, Lb, tok,
                   (const int64_t*)(f->indptr + row0), (const int32_t*)f->indices, (const float*)f->data, (const float*)nullptr,
                   f->rowloss, (float*)nullptr, f->dZ, n, f->Ve, N, 1.0f / (float)B);
    };
    if (f->indptr) {
        if (n <= 8) go_csr(llf_row_csr<true, 8>, llf_row_csr<false, 8>);
        else if (n <= 16) go_csr(llf_row_csr<true, 16>, llf_row_csr<false, 16>);
        else go_csr(llf_row_csr<true, 32>, llf_row_csr<false, 32>);
    } else if (n <= 8) go(llf_row<true, 8>, llf_row<false, 8>);
    else if (n <= 16) go(llf_row<true, 16>, llf_row<false, 16>);
    else go(llf_row<true, 32>, llf_row<false, 32>);
    return 0;
}

// one step enqueued on the handle's stream; dst: 3 floats on the device (finalize_loss: loss, data term, regulariser)
static int llf_step_async(sert_ll_foldin* f, int64_t batch, float* dst) {
    const auto& c = f->cfg;
    const int B = c.batch_size, d = f->d, N = f->N, U = f->U[(size_t)batch];
    hipStream_t s = f->stream;
    SERT_TRY(llf_forward(f, batch, true));
    // dZu = per-word sums of dZ; dWn = Gb^T dZu with db = the column sums of dZu, split-K with an order-fixed combine
    launch(llf_word_sum, dim3(grid_for((int64_t)U * N)), dim3(256), 0, s, (const float*)f->dZ,
           (const int32_t*)(f->wptr + f->ptr_off[(size_t)batch]), (const int32_t*)(f->wpos + (size_t)batch * B * f->n), f->dZu, U, N);
    int splits = 1, kper = 0;
    llf_dw_splits(f, U, &splits, &kper);
    const size_t mn = (size_t)d * N, stride = mn + N;
    launch_gemm<true, false, EPI_STORE, true>(s, f->Gb, f->dZu, f->part, nullptr, d, N, U, d, N, N, splits, kper, stride);
    launch_reduce_partials(s, f->part, splits, stride, stride, f->g_w, mn, f->g_b);
    // Adadelta: L2 on Wn, none on bn, whose sums of squares are not in the loss
    const int nb = fold_adadelta(f, f->Wn, f->g_w, f->accu_w, f->delta_w, mn, true, f->red_sq);
    fold_adadelta(f, f->bn, f->g_b, f->accu_b, f->delta_b, (size_t)N, false, f->red_sq + kOptBlocks);
    fold_finalize(f, f->rowloss, B, nb, dst);
    return 0;
}

int sert_ll_foldin_train_batch(sert_ll_foldin* f, int64_t batch, float* loss_out) {
    return fold_run_batch(f, batch, loss_out, llf_check_batch, llf_step_async);
}

int sert_ll_foldin_train_batches(sert_ll_foldin* f, const int64_t* batches, int64_t count, float* losses_out) {
    return fold_train_batches(f, batches, count, losses_out, llf_check_batch, llf_step_async);
}

int sert_ll_foldin_eval_batch(sert_ll_foldin* f, int64_t batch, float* loss_out) {
    return fold_run_batch(f, batch, loss_out, llf_check_batch, [](sert_ll_foldin* h, int64_t b, float* dst) {
        SERT_TRY(llf_forward(h, b, false));
        fold_eval_finalize(h, (const float*)h->rowloss, h->cfg.batch_size, dst);
        return 0;
    });
}

static float* llf_tensor_ref(sert_ll_foldin* f, int which, size_t* count) {
    const size_t n_w = (size_t)f->d * f->N, n_b = (size_t)f->N;
    switch (which) {
        case SERT_LL_FOLDIN_W: *count = n_w; return f->Wn;
        case SERT_LL_FOLDIN_B: *count = n_b; return f->bn;
        case SERT_LL_FOLDIN_ACCU_W: *count = n_w; return f->accu_w;
        case SERT_LL_FOLDIN_ACCU_B: *count = n_b; return f->accu_b;
        case SERT_LL_FOLDIN_DELTA_W: *count = n_w; return f->delta_w;
        case SERT_LL_FOLDIN_DELTA_B: *count = n_b; return f->delta_b;
        default: return nullptr;
    }
}

static const char* const kLlfWhich = "which must be one of SERT_LL_FOLDIN_W, _B, _ACCU_W, _ACCU_B, _DELTA_W, _DELTA_B";

int sert_ll_foldin_get_tensor(sert_ll_foldin* f, int which, float* host, size_t count) {
    return fold_copy_tensor(f, which, host, count, true, llf_tensor_ref, kLlfWhich);
}
int sert_ll_foldin_set_tensor(sert_ll_foldin* f, int which, const float* host, size_t count) {
    return fold_copy_tensor(f, which, const_cast<float*>(host), count, false, llf_tensor_ref, kLlfWhich);
}

int sert_debug_ll_foldin_layout(sert_ll_foldin* f, int32_t* V_f, int32_t* Nt, int32_t* internal_of_public, int64_t count) {
    if (!f) SERT_FAIL("null argument");
    if (count != (int64_t)f->internal_of.size() || (count > 0 && !internal_of_public))
        SERT_FAIL("count must be V_e + num_new, the public columns of the handle");
    if (V_f) *V_f = f->Ve;
    if (Nt) *Nt = f->N;
    for (int64_t i = 0; i < count; ++i) internal_of_public[i] = f->internal_of[(size_t)i];
    return 0;
}
