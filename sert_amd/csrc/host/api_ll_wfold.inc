// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block, behind api_wfold.inc): C ABI:
// folding unseen WORDS into a trained loglinear model (include/sert_hip_ll_wfold.h: sert_ll_wfold_*; kernels_ll_wfold.h;
// wfold_index.h).  Like sert_wfold the handle copies the model's parameters when it is created and runs on a stream of its
// own: it shares nothing with the model's step schedule.

struct sert_ll_wfold : FoldLl {
    sert_ll_wfold_config cfg;
    int Nw = 0;
    // the new word rows, Adadelta's accumulators, the gradient
    float *Nv = nullptr, *accu = nullptr, *delta = nullptr, *G = nullptr;
    // ---- the upload (FoldBase: M instances; FoldLl: the labels, columns in [0, V_e), and w) ----
    int64_t Df = 0;                  // distinct frozen words of the upload
    int32_t* slot = nullptr;         // (M, n)  >= 0: row of Lf; < 0: new word ~slot
    float* Lf = nullptr;             // (Df, V_e) the frozen table (null when the upload holds no frozen word)
    // the inverted index new word -> batch rows (wfold_index.h)
    std::vector<WfoldBatch> idx_batches;
    int32_t* idx_rows = nullptr;
    int4* idx_items = nullptr;
    float* part = nullptr;           // (max_part_rows, V_e)
    // per-step scratch
    float* Ln = nullptr;             // (Nw, V_e)  the step table
    float* S = nullptr;              // (Nw, V_e)  sums of dJ, then dZ
    float* DJ = nullptr;             // (B, V_e)
    DevBuf<float> skbuf;             // the k ranges of G = dZ W^T (gemm_long_k)
    // what the last step launched, recorded where the launches are made: sert_debug_ll_wfold_plan (sert_hip_debug.h)
    int32_t plan[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

static void llw_free_upload(sert_ll_wfold* f) {
    fold_free_labels(f);
    for (void* p : {(void*)f->slot, (void*)f->Lf, (void*)f->idx_rows, (void*)f->idx_items, (void*)f->part}) (void)hipFree(p);
    f->slot = nullptr; f->Lf = nullptr; f->idx_rows = nullptr; f->idx_items = nullptr; f->part = nullptr;
    f->idx_batches.clear();
    f->M = 0; f->Df = 0;
}

int sert_ll_wfold_destroy(sert_ll_wfold* f) {
    if (!f) return 0;
    float* sk = f->skbuf.p;
    f->skbuf.p = nullptr; f->skbuf.cap = 0;
    return fold_destroy(f, llw_free_upload,
                        {f->rw, f->W, f->b, f->Nv, f->accu, f->delta, f->G, f->Ln, f->S, f->DJ, f->rowloss, f->red_sq, sk});
}

static int llw_create(sert_ll_wfold* f, sert_model* m, int32_t num_new_words, const float* init_rows,
                      const sert_ll_wfold_config* cfg) {
    const auto& c = m->cfg;
    // ---- validation: everything the kernels index with is checked here ----
    if (c.kind == SERT_KIND_VECTORSPACE)
        SERT_FAIL("a loglinear word fold-in needs a loglinear model: a vectorspace model folds words in through sert_wfold_create");
    if (c.kind != SERT_KIND_LOGLINEAR)
        SERT_FAIL("a loglinear word fold-in needs a loglinear model: the full-softmax variant (SERT_KIND_VECTORSPACE_SOFTMAX) is not supported");
    if (m->comm || m->host_ar || m->world > 1)
        SERT_FAIL("a word fold-in of a data-parallel model (a communicator is attached) is not supported");
    if (num_new_words < 1) SERT_FAIL("a word fold-in needs at least one new word (num_new_words >= 1)");
    if (!init_rows) SERT_FAIL("null argument");
    if (c.window_size > 32) SERT_FAIL("a loglinear word fold-in supports window sizes up to 32");
    if (cfg->batch_size < 1) SERT_FAIL("a word fold-in needs batch_size >= 1");
    if (!(cfg->lambda_ >= 0.f)) SERT_FAIL("regularization lambda must be >= 0");
    if (!(cfg->rho >= 0.f && cfg->rho < 1.f) || !(cfg->eps > 0.f)) SERT_FAIL("Adadelta needs 0 <= rho < 1 and eps > 0");
    if ((int64_t)c.vocab_size + num_new_words > INT32_MAX) SERT_FAIL("more than 2^31 - 1 rows in the extended word table");
    if ((int64_t)cfg->batch_size * c.window_size > INT32_MAX) SERT_FAIL("batch_size * window_size > 2^31 - 1");
    if ((int64_t)cfg->batch_size * c.num_entities > INT32_MAX) SERT_FAIL("batch_size * num_entities > 2^31 - 1");
    if ((int64_t)num_new_words * c.num_entities > INT32_MAX) SERT_FAIL("num_new_words * num_entities > 2^31 - 1");
    if ((int64_t)num_new_words * c.word_dim > INT32_MAX) SERT_FAIL("num_new_words * word_dim > 2^31 - 1");
    SERT_HIP(hipSetDevice(c.device));
    f->device = c.device; f->cfg = *cfg;
    f->Vw = c.vocab_size; f->Ve = c.num_entities; f->Nw = num_new_words; f->d = c.word_dim; f->n = c.window_size;
    const int B = cfg->batch_size, Ve = f->Ve, Nw = f->Nw;
    const size_t n_v = (size_t)Nw * f->d;
    SERT_TRY(fold_settle_model(m, false));
    SERT_TRY(fold_snapshot(m, &f->rw, m->rw, m->n_rw, m->n_rw));
    SERT_TRY(fold_snapshot(m, &f->W, m->W, m->n_w, m->n_w));
    SERT_TRY(fold_snapshot(m, &f->b, m->b, m->n_b, m->n_b));
    SERT_HIP(hipStreamCreate(&f->stream));
    hipStream_t s = f->stream;
    SERT_TRY(dmalloc(&f->Nv, round_up(n_v, 4)));
    SERT_TRY(dzalloc(&f->accu, round_up(n_v, 4), s));
    SERT_TRY(dzalloc(&f->delta, round_up(n_v, 4), s));
    SERT_TRY(dmalloc(&f->G, round_up(n_v, 4)));
    SERT_HIP(hipMemcpyAsync(f->Nv, init_rows, n_v * sizeof(float), hipMemcpyHostToDevice, s));
    SERT_TRY(dmalloc(&f->Ln, (size_t)Nw * Ve));
    SERT_TRY(dmalloc(&f->S, (size_t)Nw * Ve));
    SERT_TRY(dmalloc(&f->DJ, (size_t)B * Ve));
    SERT_TRY(dmalloc(&f->rowloss, (size_t)B));
    SERT_TRY(dmalloc(&f->red_sq, (size_t)kOptBlocks));
    SERT_TRY(dmalloc(&f->d_loss, (size_t)3));
    return fold_created(f, m);      // (init_rows is borrowed for the call only)
}

int sert_ll_wfold_create(sert_model* m, int32_t num_new_words, const float* init_rows, const sert_ll_wfold_config* cfg,
                         sert_ll_wfold** out) {
    refresh_gemm_choice();
    return fold_create(m, cfg, out, "sert_ll_wfold_config size mismatch (ABI)", sert_ll_wfold_destroy,
                       [&](sert_ll_wfold* f) { return llw_create(f, m, num_new_words, init_rows, cfg); });
}

// What an upload of either label form does once its labels are known to be good: the tokens are validated; then the distinct
// frozen words, the frozen table in slabs, the slots, the inverted index, and the copies of those, of the labels and of w.
// Nothing of the handle is touched before every host-side check has passed and the new table is allocated.
static int llw_upload(sert_ll_wfold* f, const int32_t* x, const FoldLabels& lab, const float* w, int64_t M) {
    const int n = f->n, d = f->d, Ve = f->Ve, B = f->cfg.batch_size;
    const int64_t ext = (int64_t)f->Vw + f->Nw;
    for (int64_t i = 0; i < M * n; ++i)
        if (x[i] < 0 || x[i] >= ext) SERT_FAIL("token id out of range [0, vocab_size + num_new_words)");
    // ---- the distinct frozen words Df of x (sorted) and the row of its table of every position ----
    FoldWordTable t;
    SERT_TRY(fold_word_table(x, M * n, f->Vw, Ve, f->cfg.max_cache_bytes, "frozen table", "distinct frozen words", &t));
    const int64_t Df = (int64_t)t.words.size();
    std::vector<int32_t> slot((size_t)(M * n));
    for (size_t k = 0; k < slot.size(); ++k) slot[k] = x[k] < f->Vw ? t.row_of[(size_t)x[k]] : ~(x[k] - f->Vw);
    // the inverted index of the complete batches (host; a function of the upload alone)
    const int64_t nbatches = M / B;
    WfoldIndex index;
    {
        std::vector<int32_t> tok((size_t)(nbatches * B) * n);
        for (size_t k = 0; k < tok.size(); ++k) tok[k] = x[k] < f->Vw ? -1 : x[k] - f->Vw;
        build_wfold_index(tok.data(), nbatches, B, n, f->Nw, index);
    }
    SERT_HIP(hipSetDevice(f->device));
    hipStream_t s = f->stream;
    // the new table first: an upload whose table cannot be allocated keeps the earlier one
    float* table = nullptr;
    SERT_TRY(fold_alloc_table(t, &table));
    if (hipStreamSynchronize(s) != hipSuccess) {
        (void)hipFree(table);
        SERT_FAIL("hipStreamSynchronize failed");
    }
    llw_free_upload(f);
    if (M == 0) return 0;
    f->Lf = table;
    uint32_t* dwords = nullptr;
    float* Gs = nullptr;
    std::vector<float> ones;
    auto body = [&]() -> int {
        SERT_TRY(fold_upload_labels(f, lab, w, M, ones));
        SERT_TRY(dmalloc(&f->slot, (size_t)M * n));
        SERT_TRY(dmalloc(&f->idx_rows, std::max<size_t>(index.rows.size(), 1)));
        SERT_TRY(dmalloc(&f->idx_items, std::max<size_t>(index.items.size(), 1)));
        SERT_TRY(dmalloc(&f->part, std::max<size_t>((size_t)index.max_part_rows * Ve, 4)));
        SERT_HIP(hipMemcpyAsync(f->slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!index.rows.empty())
            SERT_HIP(hipMemcpyAsync(f->idx_rows, index.rows.data(), index.rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!index.items.empty())
            SERT_HIP(hipMemcpyAsync(f->idx_items, index.items.data(), index.items.size() * sizeof(SegItem), hipMemcpyHostToDevice, s));
        // the frozen table by the model's own forward kernels, a slab of rows at a time so that no launch sees 2 GiB of
        // either operand: the slabs' offsets into the table are 64 bits wide
        const int64_t slab = std::max<int64_t>(1, std::min<int64_t>(Df, (((int64_t)1 << 29) - 1) / std::max(Ve, d)));
        if (Df > 0) {
            SERT_TRY(dmalloc(&dwords, (size_t)Df));
            SERT_TRY(dmalloc(&Gs, (size_t)slab * d));
            SERT_HIP(hipMemcpyAsync(dwords, t.words.data(), (size_t)Df * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        for (int64_t r0 = 0; r0 < Df; r0 += slab) {
            const int64_t rows = std::min<int64_t>(slab, Df - r0);
            gather_rows(s, (const uint32_t*)(dwords + r0), f->rw, Gs, rows, d);
            float* dst = f->Lf + (size_t)r0 * Ve;
            launch_gemm<false, false, EPI_BIAS>(s, Gs, f->W, dst, f->b, (int)rows, Ve, d, d, Ve, Ve);
            logsoftmax_rows(s, dst, rows, Ve);
        }
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipStreamSynchronize(s));     // (x, the labels, w and the host lists are borrowed for the call only)
        return 0;
    };
    const int rc = body();
    (void)hipFree(dwords); (void)hipFree(Gs);
    if (rc != 0) return fold_upload_failed(f, rc, llw_free_upload);
    f->idx_batches.swap(index.batches);
    f->M = M; f->Df = Df;
    return 0;
}

static int llw_upload_check_sizes(int64_t M) {
    if (M > ((int64_t)1 << 31) - 1) SERT_FAIL("more than 2^31 - 1 fold-in instances");
    return 0;
}

int sert_ll_wfold_upload(sert_ll_wfold* f, const int32_t* x, const int32_t* y, const float* w, int64_t M) {
    refresh_gemm_choice();
    if (!f || M < 0 || (M > 0 && (!x || !y))) SERT_FAIL("bad argument");
    SERT_TRY(llw_upload_check_sizes(M));
    // host-side validation: no kernel is launched on bad ids
    for (int64_t i = 0; i < M; ++i)
        if (y[i] < 0 || y[i] >= f->Ve) SERT_FAIL("fold-in label out of range [0, num_entities)");
    return llw_upload(f, x, FoldLabels{y, nullptr, nullptr, nullptr}, w, M);
}

int sert_ll_wfold_upload_csr(sert_ll_wfold* f, const int32_t* x, const int64_t* indptr, const int32_t* indices, const float* data,
                             const float* w, int64_t M) {
    refresh_gemm_choice();
    if (!f || M < 0 || (M > 0 && (!x || !indptr))) SERT_FAIL("bad argument");
    SERT_TRY(llw_upload_check_sizes(M));
    // host-side validation: no kernel is launched on a bad row (a word fold-in has no new entity: column V_e is refused)
    if (M > 0)
        SERT_TRY(check_csr_rows(indptr, indices, data, M, f->Ve, "label column out of range [0, num_entities) in csr_indices", INT32_MAX));
    return llw_upload(f, x, FoldLabels{nullptr, indptr, indices, data}, w, M);
}

int64_t sert_ll_wfold_num_batches(sert_ll_wfold* f) { return fold_num_batches(f); }

static int llw_check_batch(sert_ll_wfold* f, int64_t batch) {
    return fold_check_batch(f, &sert_ll_wfold::w, "sert_ll_wfold_upload", batch);
}

// steps 1 and 2 on batch `batch`: Ln = log softmax(Nv W + b) over all Nw rows, then the row kernel (train: weighted, DJ
// written); the rows' losses are left in f->rowloss
static int llw_forward(sert_ll_wfold* f, int64_t batch, bool train) {
    const int B = f->cfg.batch_size, n = f->n, d = f->d, Ve = f->Ve, Nw = f->Nw;
    hipStream_t s = f->stream;
    for (int32_t& v : f->plan) v = 0;
    f->plan[11] = wfold_gemm<false, false, EPI_BIAS>(s, f->Nv, f->W, f->Ln, f->b, Nw, Ve, d, d, Ve, Ve);
    logsoftmax_rows(s, f->Ln, Nw, Ve);
    const size_t row0 = (size_t)batch * B;
    const int vec = Ve % 4 == 0 ? 1 : 0;
    const bool reg = Ve <= 1024;
    const int32_t* slot = f->slot + row0 * n;
    const float* w = train ? f->w + row0 : (const float*)nullptr;
    const float inv_batch = 1.0f / (float)B;
    auto go = [&](auto kernel) {
        launch(kernel, dim3(B), dim3(256), 0, s, (const float*)f->Lf, (const float*)f->Ln, slot, (const int32_t*)(f->y + row0), w,
               f->rowloss, f->DJ, n, Ve, vec, inv_batch);
    };
    // label rows (sert_ll_wfold_upload_csr): the same launch shape, the batch's slice of indptr
    auto go_csr = [&](auto kernel) {
        launch(kernel, dim3(B), dim3(256), 0, s, (const float*)f->Lf, (const float*)f->Ln, slot, (const int64_t*)(f->indptr + row0),
               (const int32_t*)f->indices, (const float*)f->data, w, f->rowloss, train ? f->labfix : (float*)nullptr, f->DJ, n, Ve, vec,
               inv_batch);
    };
    if (f->indptr) {
        if (reg) { if (train) go_csr(llw_row_csr<true, LLW_FORM_REG>); else go_csr(llw_row_csr<false, LLW_FORM_REG>); }
        else { if (train) go_csr(llw_row_csr<true, LLW_FORM_STREAM>); else go_csr(llw_row_csr<false, LLW_FORM_STREAM>); }
    } else if (reg) { if (train) go(llw_row<true, LLW_FORM_REG>); else go(llw_row<false, LLW_FORM_REG>); }
    else { if (train) go(llw_row<true, LLW_FORM_STREAM>); else go(llw_row<false, LLW_FORM_STREAM>); }
    f->plan[0] = reg ? SERT_LL_WFOLD_FORM_REG : SERT_LL_WFOLD_FORM_STREAM; f->plan[1] = vec; f->plan[2] = train ? 1 : 0;
    f->plan[14] = f->indptr ? SERT_LL_WFOLD_LABELS_ROWS : SERT_LL_WFOLD_LABELS_INT;
    return 0;
}

// step 3: S[v] = the sum of the DJ rows of v's occurrences in the batch over the batch's index, level after level -- the
// kernels of the word-gradient tree (kernels_seg.h) as they are; rows of absent words stay exactly zero
static int llw_segsum(sert_ll_wfold* f, int64_t batch) {
    const int Ve = f->Ve;
    hipStream_t s = f->stream;
    const WfoldBatch& bx = f->idx_batches[(size_t)batch];
    SERT_HIP(hipMemsetAsync(f->S, 0, (size_t)f->Nw * Ve * sizeof(float), s));
    f->plan[3] = bx.nlevels;
    for (int l = 0; l < bx.nlevels; ++l) {
        const int nitems = bx.item_cnt[l];
        f->plan[4 + l] = nitems;
        if (nitems == 0) continue;
        const float* in = (l == 0) ? f->DJ : f->part + (size_t)bx.part_off[l - 1] * Ve;
        const int32_t* rows = (l == 0) ? f->idx_rows + bx.rows_off : nullptr;
        const int4* items = f->idx_items + bx.item_off[l];
        float* pout = f->part + (size_t)bx.part_off[l] * Ve;
        if (Ve % 4 == 0) {
            launch((segsum_rows<64>), dim3(cdiv(nitems, 4), cdiv(Ve / 4, 64)), dim3(256), 0, s, in, rows, items, nitems, f->S, pout, Ve,
                   1.0f, (unsigned char*)nullptr, 1, nullptr, nullptr, DenseSlots(), XcdLists());
            f->plan[10] = SERT_WGRAD_FORM_ROWS64;
        } else {
            launch((segsum_rows_scalar<false>), dim3(cdiv(nitems, 4), cdiv(Ve, 64)), dim3(256), 0, s, in, rows, items, nitems, f->S,
                   pout, Ve, 1.0f, (unsigned char*)nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
            f->plan[10] = SERT_WGRAD_FORM_SCALAR;
        }
    }
    return 0;
}

// one step enqueued on the handle's stream; dst: 3 floats on the device (finalize_loss: loss, data term, regulariser)
static int llw_step_async(sert_ll_wfold* f, int64_t batch, float* dst) {
    const int Ve = f->Ve, Nw = f->Nw;
    hipStream_t s = f->stream;
    SERT_TRY(llw_forward(f, batch, true));
    SERT_TRY(llw_segsum(f, batch));
    launch(llw_finish, dim3(cdiv(Nw, 4)), dim3(256), 0, s, (const float*)f->Ln, f->S, Nw, Ve);
    // step 5: G (Nw, d) = dZ W^T, the form of the model's dG: K = V_e is the long side, cut into k ranges with an order-fixed
    // combine; the ranges live in the handle's own buffer
    SERT_TRY((gemm_long_k<false, true>(f->skbuf, s, f->S, f->W, f->G, Nw, f->d, Ve, Ve, Ve, nullptr, nullptr, nullptr, &f->plan[12],
                                       &f->plan[13])));
    const int nb = fold_adadelta(f, f->Nv, f->G, f->accu, f->delta, (size_t)Nw * f->d, true, f->red_sq);
    fold_finalize(f, f->rowloss, f->cfg.batch_size, nb, dst);
    return 0;
}

int sert_ll_wfold_train_batch(sert_ll_wfold* f, int64_t batch, float* loss_out) {
    refresh_gemm_choice();
    return fold_run_batch(f, batch, loss_out, llw_check_batch, llw_step_async);
}

int sert_ll_wfold_train_batches(sert_ll_wfold* f, const int64_t* batches, int64_t count, float* losses_out) {
    refresh_gemm_choice();
    return fold_train_batches(f, batches, count, losses_out, llw_check_batch, llw_step_async);
}

int sert_ll_wfold_eval_batch(sert_ll_wfold* f, int64_t batch, float* loss_out) {
    refresh_gemm_choice();
    return fold_run_batch(f, batch, loss_out, llw_check_batch, [](sert_ll_wfold* h, int64_t b, float* dst) {
        SERT_TRY(llw_forward(h, b, false));
        fold_eval_finalize(h, (const float*)h->rowloss, h->cfg.batch_size, dst);
        return 0;
    });
}

static float* llw_rows_ref(sert_ll_wfold* f, int which, size_t* count) {
    *count = (size_t)f->Nw * f->d;
    return which == SERT_LL_WFOLD_ROWS ? f->Nv : which == SERT_LL_WFOLD_ACCU ? f->accu : which == SERT_LL_WFOLD_DELTA ? f->delta : nullptr;
}
static const char* const kLlwWhich = "which must be SERT_LL_WFOLD_ROWS, SERT_LL_WFOLD_ACCU or SERT_LL_WFOLD_DELTA";

int sert_ll_wfold_get_rows(sert_ll_wfold* f, int which, float* host, size_t count) {
    return fold_copy_tensor(f, which, host, count, true, llw_rows_ref, kLlwWhich);
}
int sert_ll_wfold_set_rows(sert_ll_wfold* f, int which, const float* host, size_t count) {
    return fold_copy_tensor(f, which, const_cast<float*>(host), count, false, llw_rows_ref, kLlwWhich);
}

int sert_debug_ll_wfold_plan(sert_ll_wfold* f, int32_t* out, int n) {
    if (!f || !out || n < 1 || n > 16) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = f->plan[i];
    return 0;
}
