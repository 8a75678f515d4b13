// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: folding unseen WORDS into
// a trained vectorspace model (include/sert_hip_wfold.h: sert_wfold_*; kernels_wfold.h; wfold_index.h).  Like sert_foldin the
// handle copies the model's parameters when it is created and runs on a stream of its own: it shares nothing with the model's
// step schedule.

struct sert_wfold : FoldNce {
    sert_wfold_config cfg;
    int Nw = 0;
    // (FoldNce's snapshot: rw holds V_w + 1 rows here; the last one is zero, what a new position gathers at upload)
    float* Nv = nullptr;             // the new word rows (FoldNce: Adam's moments m1, m2 and the gradient G)
    // the uploaded instances
    float* A0 = nullptr;             // (M, d_e)  hf W + b
    int32_t* tok = nullptr;          // (M, n)    the new word of a position, -1: frozen
    // the inverted index new word -> batch rows (wfold_index.h)
    std::vector<WfoldBatch> idx_batches;
    int32_t* idx_rows = nullptr;
    int4* idx_items = nullptr;
    float* part = nullptr;           // (max_part_rows, d_e)
    // per-step scratch (FoldNce's coef and this cand: written by the loss kernel, read by nobody -- the entity table is frozen)
    float* P = nullptr;              // (Nw, d_e)  Nv W
    float* T = nullptr;              // (B, d_e)
    float* DA = nullptr;             // (B, d_e)
    float* S = nullptr;              // (Nw, d_e)
    int32_t* cand = nullptr;         // (B, 1 + z)
    // what the last step launched, recorded where the launches are made: sert_debug_wfold_plan (sert_hip_debug.h)
    int32_t plan[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

static void wfold_free_upload(sert_wfold* f) {
    for (void* p : {(void*)f->y, (void*)f->w, (void*)f->A0, (void*)f->tok, (void*)f->idx_rows, (void*)f->idx_items, (void*)f->part})
        (void)hipFree(p);
    f->y = nullptr; f->w = nullptr; f->A0 = nullptr; f->tok = nullptr; f->idx_rows = nullptr; f->idx_items = nullptr; f->part = nullptr;
    f->idx_batches.clear();
    f->M = 0;
}

int sert_wfold_destroy(sert_wfold* f) {
    if (!f) return 0;
    return fold_destroy(f, wfold_free_upload,
                        {f->rw, f->W, f->b, f->re, f->Nv, f->m1, f->m2, f->G, f->P, f->T, f->DA, f->S, f->neg, f->neg_stage, f->coef,
                         f->cand, f->rowloss, f->red_loss, f->red_sq});
}

static int wfold_create(sert_wfold* f, sert_model* m, int32_t num_new_words, const float* init_rows, const sert_wfold_config* cfg) {
    const auto& c = m->cfg;
    // ---- validation: everything the kernels index with is checked here ----
    if (c.kind == SERT_KIND_LOGLINEAR) SERT_FAIL("a word fold-in needs a vectorspace model: the loglinear model is not supported");
    if (c.kind != SERT_KIND_VECTORSPACE)
        SERT_FAIL("a word fold-in needs the NCE vectorspace model: the full-softmax variant (SERT_KIND_VECTORSPACE_SOFTMAX) is not supported");
    if (m->comm || m->host_ar || m->world > 1)
        SERT_FAIL("a word fold-in of a data-parallel model (a communicator is attached) is not supported");
    if (num_new_words < 1) SERT_FAIL("a word fold-in needs at least one new word (num_new_words >= 1)");
    if (!init_rows) SERT_FAIL("null argument");
    if (cfg->batch_size < 1 || cfg->num_negatives < 1) SERT_FAIL("a word fold-in needs batch_size >= 1 and num_negatives >= 1");
    if (!(cfg->lambda_ >= 0.f)) SERT_FAIL("regularization lambda must be >= 0");
    if (c.entity_dim > 512) SERT_FAIL("entity_dim > 512 is not supported");
    if ((int64_t)c.vocab_size + num_new_words > INT32_MAX) SERT_FAIL("more than 2^31 - 1 rows in the extended word table");
    if ((int64_t)cfg->batch_size * (cfg->num_negatives + 1) > ((int64_t)1 << 30)) SERT_FAIL("batch_size * (num_negatives + 1) > 2^30");
    if ((int64_t)cfg->batch_size * c.window_size > INT32_MAX) SERT_FAIL("batch_size * window_size > 2^31 - 1");
    SERT_HIP(hipSetDevice(c.device));
    f->device = c.device; f->cfg = *cfg;
    f->Vw = c.vocab_size; f->Ve = c.num_entities; f->Nw = num_new_words; f->dw = c.word_dim; f->de = c.entity_dim; f->n = c.window_size;
    const int B = cfg->batch_size, z = cfg->num_negatives, de = f->de, dw = f->dw, Nw = f->Nw;
    const size_t n_v = (size_t)Nw * dw;
    SERT_TRY(fold_settle_model(m, true));
    SERT_TRY(fold_snapshot_vs(f, m, 1));
    SERT_HIP(hipStreamCreate(&f->stream));
    hipStream_t s = f->stream;
    SERT_TRY(dmalloc(&f->Nv, round_up(n_v, 4)));
    SERT_TRY(dzalloc(&f->m1, round_up(n_v, 4), s));
    SERT_TRY(dzalloc(&f->m2, round_up(n_v, 4), s));
    SERT_TRY(dmalloc(&f->G, round_up(n_v, 4)));
    SERT_HIP(hipMemcpyAsync(f->Nv, init_rows, n_v * sizeof(float), hipMemcpyHostToDevice, s));
    const size_t total = (size_t)B * (z + 1);
    SERT_TRY(dmalloc(&f->P, (size_t)Nw * de));
    SERT_TRY(dmalloc(&f->S, (size_t)Nw * de));
    SERT_TRY(dmalloc(&f->T, (size_t)B * de));
    SERT_TRY(dmalloc(&f->DA, (size_t)B * de));
    SERT_TRY(dmalloc(&f->neg, (size_t)B * z));
    SERT_TRY(dmalloc(&f->neg_stage, (size_t)B * z));
    SERT_TRY(dmalloc(&f->coef, total));
    SERT_TRY(dmalloc(&f->cand, total));
    SERT_TRY(dmalloc(&f->rowloss, (size_t)B));
    SERT_TRY(dmalloc(&f->red_loss, (size_t)cdiv(B, 16)));
    SERT_TRY(dmalloc(&f->red_sq, (size_t)kOptBlocks));
    SERT_TRY(dmalloc(&f->d_loss, (size_t)3));
    return fold_created(f, m);      // (init_rows is borrowed for the call only)
}

int sert_wfold_create(sert_model* m, int32_t num_new_words, const float* init_rows, const sert_wfold_config* cfg, sert_wfold** out) {
    refresh_gemm_choice();
    return fold_create(m, cfg, out, "sert_wfold_config size mismatch (ABI)", sert_wfold_destroy,
                       [&](sert_wfold* f) { return wfold_create(f, m, num_new_words, init_rows, cfg); });
}

// launch_gemm, and the route it takes (gemm.h: GemmRoute) -- asked of the launcher's own predicates, for the plan
extern "C++" {
template <bool TA, bool TB, int EPI>
static int wfold_gemm(hipStream_t s, const float* A, const float* Bm, float* C, const float* bias, int M, int N, int K, int lda,
                      int ldb, int ldc) {
    const int route = gemm_route(TA, TB, EPI, false, false, A, Bm, M, N, K, lda, ldb, 1, K);
    launch_gemm<TA, TB, EPI>(s, A, Bm, C, bias, M, N, K, lda, ldb, ldc);
    return route;
}
}  // extern "C++"

int sert_wfold_upload(sert_wfold* f, const int32_t* x, const int32_t* y, const float* w, int64_t M) {
    refresh_gemm_choice();
    if (!f || M < 0 || (M > 0 && (!x || !y))) SERT_FAIL("bad argument");
    if (M > ((int64_t)1 << 31) - 1) SERT_FAIL("more than 2^31 - 1 fold-in instances");
    const int n = f->n, de = f->de, B = f->cfg.batch_size;
    // host-side validation: no kernel is launched on bad ids
    for (int64_t i = 0; i < M; ++i)
        if (y[i] < 0 || y[i] >= f->Ve) SERT_FAIL("fold-in label out of range [0, num_entities)");
    const int64_t ext = (int64_t)f->Vw + f->Nw;
    for (int64_t i = 0; i < M * n; ++i)
        if (x[i] < 0 || x[i] >= ext) SERT_FAIL("token id out of range [0, vocab_size + num_new_words)");
    SERT_HIP(hipSetDevice(f->device));
    hipStream_t s = f->stream;
    SERT_HIP(hipStreamSynchronize(s));
    wfold_free_upload(f);
    if (M == 0) return 0;
    // the inverted index of the complete batches (host; a function of the upload alone)
    const int64_t nbatches = M / B;
    WfoldIndex index;
    {
        std::vector<int32_t> tok((size_t)(nbatches * B) * n);
        for (size_t k = 0; k < tok.size(); ++k) tok[k] = x[k] < f->Vw ? -1 : x[k] - f->Vw;
        build_wfold_index(tok.data(), nbatches, B, n, f->Nw, index);
    }
    std::vector<float> ones;
    auto body = [&]() -> int {
        SERT_TRY(fold_upload_labels(f, y, w, M, ones));
        SERT_TRY(dmalloc(&f->A0, (size_t)M * de));
        SERT_TRY(dmalloc(&f->tok, (size_t)M * n));
        SERT_TRY(dmalloc(&f->idx_rows, std::max<size_t>(index.rows.size(), 1)));
        SERT_TRY(dmalloc(&f->idx_items, std::max<size_t>(index.items.size(), 1)));
        SERT_TRY(dmalloc(&f->part, std::max<size_t>((size_t)index.max_part_rows * de, 4)));
        if (!index.rows.empty())
            SERT_HIP(hipMemcpyAsync(f->idx_rows, index.rows.data(), index.rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (!index.items.empty())
            SERT_HIP(hipMemcpyAsync(f->idx_items, index.items.data(), index.items.size() * sizeof(SegItem), hipMemcpyHostToDevice, s));
        // A0 = hf W + b once: the new positions are pointed at the snapshot's appended zero row
        return fold_project_slabs<EPI_BIAS>(f, x, M, f->A0, [&](const int32_t* xs, uint32_t* dx, int64_t r0, int rows) {
            launch(wfold_split_ids, dim3(grid_for((int64_t)rows * n)), dim3(256), 0, s, xs, dx, f->tok + (size_t)r0 * n,
                   (int64_t)rows * n, f->Vw);
        });
    };
    const int rc = body();
    if (rc != 0) return fold_upload_failed(f, rc, wfold_free_upload);
    f->idx_batches.swap(index.batches);
    f->M = M;
    return 0;
}

int64_t sert_wfold_num_batches(sert_wfold* f) { return fold_num_batches(f); }

// the step's negatives into f->neg, over V_e
static int wfold_negatives(sert_wfold* f, const int64_t* negatives, uint64_t stream_pos) {
    return fold_negatives(f, negatives, stream_pos, (int64_t)f->Ve, "negative sample out of range [0, num_entities)");
}

// steps 1 to 3 on batch `batch`: P = Nv W, T = tanh(A0 + sum P / n), the model's loss kernel on T (train: weighted, DA
// written).  *parts / *n_parts: the loss partials it left.
static int wfold_forward_loss(sert_wfold* f, int64_t batch, bool train, const float** parts, int* n_parts) {
    const int B = f->cfg.batch_size, z = f->cfg.num_negatives, de = f->de, dw = f->dw, n = f->n;
    hipStream_t s = f->stream;
    const size_t row0 = (size_t)batch * B;
    for (int32_t& v : f->plan) v = 0;
    f->plan[12] = wfold_gemm<false, false, EPI_STORE>(s, f->Nv, f->W, f->P, nullptr, f->Nw, de, dw, dw, de, de);
    const bool vector = de % 4 == 0;
    if (vector)
        launch((wfold_project<4>), dim3(grid_for((int64_t)B * de / 4, 256, 1 << 20)), dim3(256), 0, s, (const float*)(f->A0 + row0 * de),
               (const int32_t*)(f->tok + row0 * n), (const float*)f->P, f->T, B, n, de);
    else
        launch((wfold_project<1>), dim3(grid_for((int64_t)B * de, 256, 1 << 20)), dim3(256), 0, s, (const float*)(f->A0 + row0 * de),
               (const int32_t*)(f->tok + row0 * n), (const float*)f->P, f->T, B, n, de);
    f->plan[0] = vector ? SERT_WFOLD_PROJECT_VECTOR : SERT_WFOLD_PROJECT_SCALAR;
    const int32_t* y = f->y + row0;
    const float* w = train ? f->w + row0 : (const float*)nullptr;
    const float inv_batch = 1.0f / (float)B;
    const int k = vector ? cdiv(de / 4, 16) : cdiv(de, 64);
    const dim3 grid(cdiv(B, vector ? 16 : 4)), block(256);
    const bool launched = dispatch_int<1, 8>(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (vector) {
            if (train) launch((vs_nce<K, true>), grid, block, 0, s, (const float*)f->T, (const float*)f->re, y, (const int32_t*)f->neg, w,
                              f->DA, f->coef, f->cand, f->rowloss, B, z, de, inv_batch, f->red_loss);
            else launch((vs_nce<K, false>), grid, block, 0, s, (const float*)f->T, (const float*)f->re, y, (const int32_t*)f->neg, w,
                        f->DA, f->coef, f->cand, f->rowloss, B, z, de, inv_batch, f->red_loss);
        } else {
            if (train) launch((vs_nce_scalar<K, true>), grid, block, 0, s, (const float*)f->T, (const float*)f->re, y,
                              (const int32_t*)f->neg, w, f->DA, f->coef, f->cand, f->rowloss, B, z, de, inv_batch);
            else launch((vs_nce_scalar<K, false>), grid, block, 0, s, (const float*)f->T, (const float*)f->re, y,
                        (const int32_t*)f->neg, w, f->DA, f->coef, f->cand, f->rowloss, B, z, de, inv_batch);
        }
    });
    if (!launched) SERT_FAIL("entity_dim > 512 is not supported");
    // (the scalar layout leaves no workgroup partials: the rows' losses themselves)
    *parts = vector ? f->red_loss : f->rowloss;
    *n_parts = vector ? cdiv(B, 16) : B;
    f->plan[1] = vector ? SERT_NCE_FORM_PER_CANDIDATE : SERT_NCE_FORM_SCALAR; f->plan[2] = k; f->plan[3] = train ? 1 : 0;
    return 0;
}

// step 4: S[v] = (sum of the DA rows of v's occurrences in the batch) / n over the batch's index, level after level -- the
// kernels of the word-gradient tree (kernels_seg.h) as word_grad_segsum launches them; rows of absent words stay zero
static int wfold_segsum(sert_wfold* f, int64_t batch) {
    const int de = f->de;
    hipStream_t s = f->stream;
    const WfoldBatch& bx = f->idx_batches[(size_t)batch];
    SERT_HIP(hipMemsetAsync(f->S, 0, (size_t)f->Nw * de * sizeof(float), s));
    const float divisor = (float)f->n;
    f->plan[4] = bx.nlevels;
    for (int l = 0; l < bx.nlevels; ++l) {
        const int nitems = bx.item_cnt[l];
        f->plan[5 + l] = nitems;
        if (nitems == 0) continue;
        const float* in = (l == 0) ? f->DA : f->part + (size_t)bx.part_off[l - 1] * de;
        const int32_t* rows = (l == 0) ? f->idx_rows + bx.rows_off : nullptr;
        const int4* items = f->idx_items + bx.item_off[l];
        float* pout = f->part + (size_t)bx.part_off[l] * de;
        if (de % 4 == 0) {
            const int ch = de / 4;
            const bool seg32y = ch > 64 && 64 * cdiv(ch, 64) > 32 * cdiv(ch, 32);
            if (ch <= 32 || seg32y) {
                launch((segsum_rows<32>), dim3(cdiv(nitems, 8), ch <= 32 ? 1 : cdiv(ch, 32)), dim3(256), 0, s, in, rows, items, nitems,
                       f->S, pout, de, divisor, (unsigned char*)nullptr, 1, nullptr, nullptr, DenseSlots(), XcdLists());
                f->plan[11] = SERT_WGRAD_FORM_ROWS32;
            } else {
                launch((segsum_rows<64>), dim3(cdiv(nitems, 4), cdiv(ch, 64)), dim3(256), 0, s, in, rows, items, nitems, f->S, pout, de,
                       divisor, (unsigned char*)nullptr, 1, nullptr, nullptr, DenseSlots(), XcdLists());
                f->plan[11] = SERT_WGRAD_FORM_ROWS64;
            }
        } else {
            launch((segsum_rows_scalar<false>), dim3(cdiv(nitems, 4), cdiv(de, 64)), dim3(256), 0, s, in, rows, items, nitems, f->S,
                   pout, de, divisor, (unsigned char*)nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
            f->plan[11] = SERT_WGRAD_FORM_SCALAR;
        }
    }
    return 0;
}

static int wfold_check_batch(sert_wfold* f, int64_t batch) {
    return fold_check_batch(f, &sert_wfold::A0, "sert_wfold_upload", batch);
}

// one step enqueued on the handle's stream; dst: 3 floats on the device (finalize_loss: loss, data term, regulariser)
static int wfold_step_async(sert_wfold* f, int64_t batch, const int64_t* negatives, float* dst) {
    SERT_TRY(wfold_negatives(f, negatives, (uint64_t)f->step * 2));
    const float* parts = nullptr;
    int n_parts = 0;
    SERT_TRY(wfold_forward_loss(f, batch, true, &parts, &n_parts));
    SERT_TRY(wfold_segsum(f, batch));
    // G = S W^T: the form of the step's dh GEMM
    f->plan[13] = wfold_gemm<false, true, EPI_STORE>(f->stream, f->S, f->W, f->G, nullptr, f->Nw, f->dw, f->de, f->de, f->de, f->dw);
    fold_adam_finalize(f, f->Nv, (size_t)f->Nw * f->dw, parts, n_parts, dst);
    return 0;
}

int sert_wfold_train_batch(sert_wfold* f, int64_t batch, const int64_t* negatives, float* loss_out) {
    refresh_gemm_choice();
    return fold_run_batch(f, batch, loss_out, wfold_check_batch,
                          [&](sert_wfold* h, int64_t b, float* dst) { return wfold_step_async(h, b, negatives, dst); });
}

int sert_wfold_train_batches(sert_wfold* f, const int64_t* batches, int64_t count, float* losses_out) {
    refresh_gemm_choice();
    return fold_train_batches(f, batches, count, losses_out, wfold_check_batch,
                              [](sert_wfold* h, int64_t b, float* dst) { return wfold_step_async(h, b, nullptr, dst); });
}

int sert_wfold_eval_batch(sert_wfold* f, int64_t batch, const int64_t* negatives, float* loss_out) {
    refresh_gemm_choice();
    return fold_run_batch(f, batch, loss_out, wfold_check_batch, [&](sert_wfold* h, int64_t b, float* dst) {
        SERT_TRY(wfold_negatives(h, negatives, (uint64_t)h->eval_draws * 2 + 1));
        if (!negatives) ++h->eval_draws;
        const float* parts = nullptr;
        int n_parts = 0;
        SERT_TRY(wfold_forward_loss(h, b, false, &parts, &n_parts));
        fold_eval_finalize(h, parts, n_parts, dst);
        return 0;
    });
}

int sert_wfold_negatives_of_step(sert_wfold* f, int64_t position, int evaluation, int64_t* out) {
    if (!f || !out || position < 0) SERT_FAIL("bad argument");
    return fold_negatives_of_step(f, position, evaluation, out, (int64_t)f->Ve);
}

static float* wfold_rows_ref(sert_wfold* f, int which, size_t* count) {
    *count = (size_t)f->Nw * f->dw;
    return which == SERT_WFOLD_ROWS ? f->Nv : which == SERT_WFOLD_M ? f->m1 : which == SERT_WFOLD_V ? f->m2 : nullptr;
}
static const char* const kWfoldWhich = "which must be SERT_WFOLD_ROWS, SERT_WFOLD_M or SERT_WFOLD_V";

int sert_wfold_get_rows(sert_wfold* f, int which, float* host, size_t count) {
    return fold_copy_tensor(f, which, host, count, true, wfold_rows_ref, kWfoldWhich);
}
int sert_wfold_set_rows(sert_wfold* f, int which, const float* host, size_t count) {
    return fold_copy_tensor(f, which, const_cast<float*>(host), count, false, wfold_rows_ref, kWfoldWhich);
}

int sert_wfold_set_step(sert_wfold* f, int64_t t) { return fold_set_counter(f, &FoldNce::step, t); }
int64_t sert_wfold_get_step(sert_wfold* f) { return fold_get_counter(f, &FoldNce::step); }
int sert_wfold_set_eval_draws(sert_wfold* f, int64_t n) { return fold_set_counter(f, &FoldNce::eval_draws, n); }
int64_t sert_wfold_get_eval_draws(sert_wfold* f) { return fold_get_counter(f, &FoldNce::eval_draws); }

int sert_debug_wfold_plan(sert_wfold* f, int32_t* out, int n) {
    if (!f || !out || n < 1 || n > 16) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = f->plan[i];
    return 0;
}

// Host only: the index build_wfold_index makes for batch `batch` of tok (num_batches, B, n) -- new word or -1 per position --
// as flat arrays: levels[0] = the levels, levels[1 + l] = the items of level l, levels[7 + l] = the first partial row of level
// l's output; rows_out (<= rows_cap) the entries; items_out (<= items_cap items of four ints) the items, level after level.
// *num_rows / *num_items: what the batch holds (also when the caps are too small: nothing is copied then, and 0 is returned).
int sert_debug_wfold_index(const int32_t* tok, int64_t num_batches, int B, int n, int num_words, int64_t batch, int32_t* levels,
                           int32_t* rows_out, int64_t rows_cap, int32_t* items_out, int64_t items_cap, int64_t* num_rows,
                           int64_t* num_items) {
    if (!tok || !levels || !num_rows || !num_items || num_batches < 1 || B < 1 || n < 1 || num_words < 1 || batch < 0 ||
        batch >= num_batches)
        SERT_FAIL("bad argument");
    for (int64_t k = 0; k < num_batches * B * n; ++k)
        if (tok[k] >= num_words) SERT_FAIL("new word out of range [0, num_words)");
    WfoldIndex index;
    build_wfold_index(tok, num_batches, B, n, num_words, index);
    const WfoldBatch& bx = index.batches[(size_t)batch];
    for (int i = 0; i < 13; ++i) levels[i] = 0;
    levels[0] = bx.nlevels;
    int64_t items = 0;
    for (int l = 0; l < bx.nlevels; ++l) { levels[1 + l] = bx.item_cnt[l]; levels[7 + l] = (int32_t)bx.part_off[l]; items += bx.item_cnt[l]; }
    *num_rows = bx.num_entries;
    *num_items = items;
    if (rows_out && rows_cap >= bx.num_entries && items_out && items_cap >= items) {
        std::copy(index.rows.begin() + bx.rows_off, index.rows.begin() + bx.rows_off + bx.num_entries, rows_out);
        if (items) memcpy(items_out, index.items.data() + bx.item_off[0], (size_t)items * sizeof(SegItem));
    }
    return 0;
}
