// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block, in front of api_foldin.inc): the
// runtime the four fold-in handles share (api_foldin.inc: sert_foldin; api_wfold.inc: sert_wfold -- the two NCE handles of a
// vectorspace model, on FoldNce; api_ll_foldin.inc: sert_ll_foldin; api_ll_wfold.inc: sert_ll_wfold -- the two Adadelta handles
// of a loglinear model, on FoldLl).  Every piece below is stated once; what a handle validates, its own buffers, its forward,
// its gradient and its plan stay in its file.  The launchers the handles share with the training step (gather_rows,
// gather_mean, logsoftmax_rows, gemm_long_k) are in lazy_segsum.inc, the CSR row validator (check_csr_rows) in
// api_data_train.inc.  Nothing here calls refresh_gemm_choice(): that is the public entry points' business.
extern "C++" {

// What every fold-in handle holds.  (cfg stays in the handle: the four config structs are distinct ABI structs.)
struct FoldBase {
    int device = -1;
    hipStream_t stream = nullptr;
    int64_t M = 0;                   // the uploaded instances
    float* d_loss = nullptr;         // [3]
    DevBuf<float> d_losses;          // multi-step loss ring: 3 floats per step
};

// ... and the two NCE handles of a vectorspace model on top of it.
struct FoldNce : FoldBase {
    int Vw = 0, Ve = 0, dw = 0, de = 0, n = 0;
    // the frozen snapshot
    float *rw = nullptr, *W = nullptr, *b = nullptr, *re = nullptr;
    // Adam's moments and the gradient of the trainable rows
    float *m1 = nullptr, *m2 = nullptr, *G = nullptr;
    // the uploaded labels and weights
    int32_t* y = nullptr;
    float* w = nullptr;
    // per-step scratch
    int32_t* neg = nullptr;          // (B, z)
    int64_t* neg_stage = nullptr;    // (B, z) host-supplied negatives
    float* coef = nullptr;           // (B, 1 + z)
    float* rowloss = nullptr;        // (B)
    float* red_loss = nullptr;       // per-workgroup loss partials of the loss kernel
    float* red_sq = nullptr;         // [kOptBlocks] sums of squares of the trainable rows
    int64_t step = 0, eval_draws = 0;
};

// ... and the two Adadelta handles of a loglinear model.  (Ve: the columns of the frozen W the handle's kernels see.)
struct FoldLl : FoldBase {
    int Vw = 0, Ve = 0, d = 0, n = 0;
    // the frozen snapshot
    float *rw = nullptr, *W = nullptr, *b = nullptr;
    // the uploaded labels: one per instance (*_upload), or label rows (*_upload_csr) -- (M + 1) offsets, the (nnz) columns,
    // strictly increasing per row, and their values -- with labfix, per entry Q_e dQ_e of the step (nnz); the weights (M)
    int32_t* y = nullptr;
    int64_t* indptr = nullptr;
    int32_t* indices = nullptr;
    float *data = nullptr, *labfix = nullptr, *w = nullptr;
    // per-step scratch
    float* rowloss = nullptr;        // (B)
    float* red_sq = nullptr;         // [kOptBlocks] sums of squares per parameter block (fold_adadelta)
};

// The labels of a loglinear upload, already validated: y (one per instance), or the CSR rows (indptr, indices, data).
struct FoldLabels {
    const int32_t* y;
    const int64_t* indptr;
    const int32_t* indices;
    const float* data;
};

// ---- create and destroy ----------------------------------------------------------------------------------------------
// The shell of every public creator: body(f) fills the new handle; a failure destroys it and keeps the body's error.
template <class F, class Cfg, class Body>
static int fold_create(sert_model* m, const Cfg* cfg, F** out, const char* abi_error, int (*destroy)(F*), Body body) {
    if (!m || !cfg || !out) SERT_FAIL("null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(Cfg)) SERT_FAIL(abi_error);
    F* f = new F();
    const int rc = body(f);
    if (rc != 0) {
        const std::string keep = g_last_error;
        destroy(f);
        g_last_error = keep;
        return rc;
    }
    *out = f;
    return 0;
}

// own: every device pointer of the handle outside its upload (free_upload) and outside FoldBase
template <class F, class FreeUpload>
static int fold_destroy(F* f, FreeUpload free_upload, std::initializer_list<void*> own) {
    if (f->device >= 0) {
        (void)hipSetDevice(f->device);
        if (f->stream) (void)hipStreamSynchronize(f->stream);
    }
    free_upload(f);
    for (void* p : own) (void)hipFree(p);
    (void)hipFree(f->d_loss);
    f->d_losses.release();
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
    return 0;
}

// The parameters as a reader must see them (sert_get_tensor, sert_reval_run): every lazily updated word-table row brought to
// the model's step, the side queues drained; entity_side (a vectorspace model): a deferred entity-table update landed.
static int fold_settle_model(sert_model* m, bool entity_side) {
    SERT_TRY(ensure_full_rw(m));
    SERT_TRY(ensure_rw_current(m, -1));
    if (m->comm_stream) SERT_HIP(hipStreamSynchronize(m->comm_stream));
    if (m->stream2) SERT_HIP(hipStreamSynchronize(m->stream2));
    if (entity_side) {
        SERT_TRY(settle_entity_update(m));
        flush_pending_tail(m);
    }
    return 0;
}

// *dst = `room` floats: the model's `count` at src, copied on the model's stream, and zeros behind them
static int fold_snapshot(sert_model* m, float** dst, const float* src, size_t count, size_t room) {
    SERT_TRY(dmalloc(dst, room));
    if (count) SERT_HIP(hipMemcpyAsync(*dst, src, count * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    if (room > count) SERT_HIP(hipMemsetAsync(*dst + count, 0, (room - count) * sizeof(float), m->stream));
    return 0;
}

// the snapshot of a vectorspace model behind fold_settle_model; zero_rows: rows of zeros appended to rw
static int fold_snapshot_vs(FoldNce* f, sert_model* m, int zero_rows) {
    SERT_TRY(fold_snapshot(m, &f->rw, m->rw, m->n_rw, zero_rows ? round_up(m->n_rw + (size_t)zero_rows * f->dw, 4) : m->n_rw));
    SERT_TRY(fold_snapshot(m, &f->W, m->W, m->n_w, m->n_w));
    SERT_TRY(fold_snapshot(m, &f->b, m->b, m->n_b, m->n_b));
    return fold_snapshot(m, &f->re, m->re, m->n_re, std::max<size_t>(m->n_re, 4));
}

// the end of a creator: the host arrays it borrowed are read, the snapshot is complete (the model may train or go away)
static int fold_created(FoldBase* f, sert_model* m) {
    SERT_HIP(hipStreamSynchronize(f->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    return 0;
}

// ---- the upload --------------------------------------------------------------------------------------------------------
// an upload that failed half-way: the partial upload is freed and the first error kept
template <class F, class FreeUpload>
static int fold_upload_failed(F* f, int rc, FreeUpload free_upload) {
    const std::string keep = g_last_error;
    (void)hipStreamSynchronize(f->stream);
    free_upload(f);
    g_last_error = keep;
    return rc;
}

// *dst = the weights of an upload of M > 0 instances; ones: the weights of an upload without w -- the caller's vector,
// because it must live until the upload's final synchronisation
static int fold_upload_weights(FoldBase* f, float** dst, const float* w, int64_t M, std::vector<float>& ones) {
    SERT_TRY(dmalloc(dst, (size_t)M));
    if (!w) ones.assign((size_t)M, 1.0f);
    SERT_HIP(hipMemcpyAsync(*dst, w ? w : ones.data(), (size_t)M * sizeof(float), hipMemcpyHostToDevice, f->stream));
    return 0;
}

// y and w of an upload of M > 0 instances into a vectorspace handle
static int fold_upload_labels(FoldNce* f, const int32_t* y, const float* w, int64_t M, std::vector<float>& ones) {
    SERT_TRY(dmalloc(&f->y, (size_t)M));
    SERT_HIP(hipMemcpyAsync(f->y, y, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    return fold_upload_weights(f, &f->w, w, M, ones);
}

// ... and the labels of either form and w into a loglinear handle
static int fold_upload_labels(FoldLl* f, const FoldLabels& lab, const float* w, int64_t M, std::vector<float>& ones) {
    hipStream_t s = f->stream;
    if (lab.y) {
        SERT_TRY(dmalloc(&f->y, (size_t)M));
        SERT_HIP(hipMemcpyAsync(f->y, lab.y, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, s));
    } else {
        const int64_t nnz = lab.indptr[M];
        SERT_TRY(dmalloc(&f->indptr, (size_t)M + 1));
        SERT_TRY(dmalloc(&f->indices, (size_t)std::max<int64_t>(1, nnz)));
        SERT_TRY(dmalloc(&f->data, (size_t)std::max<int64_t>(1, nnz)));
        SERT_TRY(dmalloc(&f->labfix, (size_t)std::max<int64_t>(1, nnz)));
        SERT_HIP(hipMemcpyAsync(f->indptr, lab.indptr, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (nnz) {
            SERT_HIP(hipMemcpyAsync(f->indices, lab.indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
            SERT_HIP(hipMemcpyAsync(f->data, lab.data, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    return fold_upload_weights(f, &f->w, w, M, ones);
}

static void fold_free_labels(FoldLl* f) {
    for (void* p : {(void*)f->y, (void*)f->indptr, (void*)f->indices, (void*)f->data, (void*)f->labfix, (void*)f->w}) (void)hipFree(p);
    f->y = nullptr; f->indptr = nullptr; f->indices = nullptr; f->data = nullptr; f->labfix = nullptr; f->w = nullptr;
}

// The distinct words of an upload that have a row in a device table of V_e columns (the logit cache, the frozen table):
// the ids below Vw among x's `count` tokens, ascending, and the row of each (-1: none); the table's bytes, refused above
// max_cache_bytes (0: no limit).  noun, unit: the handle's words for the table and for its rows.
struct FoldWordTable {
    std::vector<int32_t> row_of, words;
    unsigned long long need = 0;
    const char* noun = "";
};
static int fold_word_table(const int32_t* x, int64_t count, int Vw, int Ve, unsigned long long max_cache_bytes, const char* noun,
                           const char* unit, FoldWordTable* t) {
    t->noun = noun;
    t->row_of.assign((size_t)Vw, -1);
    for (int64_t i = 0; i < count; ++i)
        if (x[i] < Vw) t->row_of[(size_t)x[i]] = 0;
    for (int32_t v = 0; v < Vw; ++v)
        if (t->row_of[(size_t)v] == 0) { t->row_of[(size_t)v] = (int32_t)t->words.size(); t->words.push_back(v); }
    const unsigned long long D = t->words.size();
    t->need = D * (unsigned long long)Ve * sizeof(float);
    if (max_cache_bytes != 0 && t->need > max_cache_bytes)
        SERT_FAIL(std::string("the ") + noun + " of this upload needs " + std::to_string(t->need) + " bytes (" + std::to_string(D) + " " +
                  unit + " x " + std::to_string(Ve) + " entities), more than max_cache_bytes = " + std::to_string(max_cache_bytes));
    return 0;
}
// ... and its allocation (an empty table: *table stays null), refused with the bytes it needs
static int fold_alloc_table(const FoldWordTable& t, float** table) {
    *table = nullptr;
    if (t.need != 0 && hipMalloc((void**)table, (size_t)t.need) != hipSuccess) {
        (void)hipGetLastError();
        *table = nullptr;
        SERT_FAIL(std::string("the ") + t.noun + " of this upload needs " + std::to_string(t.need) + " bytes, which cannot be allocated");
    }
    return 0;
}

// out (M, d_e) = EPI(h W + b) by the model's forward (vs_project: vs_gather_mean on the snapshot, the projection GEMM), a slab
// of rows at a time; split (or nullptr): what turns a slab's token ids (staged) into the rows to gather, in front of the
// gather.  Ends with the upload's final synchronisation: the host arrays are borrowed for the call only.
template <int EPI, class Split>
static int fold_project_slabs(FoldNce* f, const int32_t* x, int64_t M, float* out, Split split) {
    constexpr bool has_split = !std::is_same<Split, std::nullptr_t>::value;
    const int n = f->n, dw = f->dw, de = f->de;
    hipStream_t s = f->stream;
    const int64_t slab = std::min<int64_t>(M, 65536);
    uint32_t* dx = nullptr;
    int32_t* xs = nullptr;
    float* H = nullptr;
    auto body = [&]() -> int {
        if constexpr (has_split) SERT_TRY(dmalloc(&xs, (size_t)slab * n));
        SERT_TRY(dmalloc(&dx, (size_t)slab * n));
        SERT_TRY(dmalloc(&H, (size_t)slab * dw));
        for (int64_t r0 = 0; r0 < M; r0 += slab) {
            const int rows = (int)std::min<int64_t>(slab, M - r0);
            SERT_HIP(hipMemcpyAsync(has_split ? (void*)xs : (void*)dx, x + (size_t)r0 * n, (size_t)rows * n * sizeof(int32_t),
                                    hipMemcpyHostToDevice, s));
            if constexpr (has_split) split((const int32_t*)xs, dx, r0, rows);
            gather_mean(s, (const uint32_t*)dx, f->rw, H, rows, n, dw);
            launch_gemm<false, false, EPI>(s, H, f->W, out + (size_t)r0 * de, f->b, rows, de, dw, dw, de, de);
        }
        SERT_HIP(hipGetLastError());
        SERT_HIP(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    (void)hipFree(dx); (void)hipFree(xs); (void)hipFree(H);
    return rc;
}

// ---- batches -----------------------------------------------------------------------------------------------------------
template <class F>
static int64_t fold_num_batches(F* f) { return f ? f->M / f->cfg.batch_size : -1; }

// uploaded: the member that an upload leaves non-null; upload_fn: the name the error sends the caller to
template <class F, class O>
static int fold_check_batch(F* f, float* O::*uploaded, const char* upload_fn, int64_t batch) {
    if (!f) SERT_FAIL("null argument");
    if (!(f->*uploaded)) SERT_FAIL(std::string("no fold-in instances uploaded (") + upload_fn + ")");
    if (batch < 0 || (batch + 1) * (int64_t)f->cfg.batch_size > f->M) SERT_FAIL("batch index out of range");
    return 0;
}

// the loss of what was just enqueued with f->d_loss as its destination (finalize_loss: loss, data term, regulariser)
static int fold_read_loss(FoldBase* f, float* loss_out) {
    float host[3] = {0.f, 0.f, 0.f};
    SERT_HIP(hipGetLastError());
    SERT_HIP(hipMemcpyAsync(host, f->d_loss, sizeof host, hipMemcpyDeviceToHost, f->stream));
    SERT_HIP(hipStreamSynchronize(f->stream));
    if (loss_out) *loss_out = host[0];
    return 0;
}

// *_train_batch and *_eval_batch: check(f, batch), then enqueue(f, batch, dst) with the handle's 3 floats, then the read-back
template <class F, class Check, class Enqueue>
static int fold_run_batch(F* f, int64_t batch, float* loss_out, Check check, Enqueue enqueue) {
    SERT_TRY(check(f, batch));
    SERT_HIP(hipSetDevice(f->device));
    SERT_TRY(enqueue(f, batch, f->d_loss));
    return fold_read_loss(f, loss_out);
}

// *_train_batches: every index checked before anything is enqueued, the steps' losses through the ring
template <class F, class Check, class Step>
static int fold_train_batches(F* f, const int64_t* batches, int64_t count, float* losses_out, Check check, Step step) {
    if (!f || count < 0 || (count > 0 && !batches)) SERT_FAIL("bad argument");
    for (int64_t i = 0; i < count; ++i) SERT_TRY(check(f, batches[i]));
    if (count == 0) return 0;
    SERT_HIP(hipSetDevice(f->device));
    if (3 * count > f->d_losses.cap) {
        SERT_HIP(hipStreamSynchronize(f->stream));      // (DevBuf::reserve frees the old ring without synchronising)
        SERT_TRY(f->d_losses.reserve(3 * count));
    }
    for (int64_t i = 0; i < count; ++i) SERT_TRY(step(f, batches[i], f->d_losses.p + 3 * i));
    SERT_HIP(hipGetLastError());
    std::vector<float> tmp((size_t)count * 3);
    SERT_HIP(hipMemcpyAsync(tmp.data(), f->d_losses.p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    SERT_HIP(hipStreamSynchronize(f->stream));
    if (losses_out)
        for (int64_t i = 0; i < count; ++i) losses_out[i] = tmp[(size_t)3 * i];
    return 0;
}

// ---- the vectorspace sampler -------------------------------------------------------------------------------------------
// `count` Philox draws from [0, range) at stream position stream_pos (even = training draws, odd = evaluation draws, as the
// model's sampler)
static void fold_sample(hipStream_t s, int32_t* dst, int64_t count, int64_t range, uint64_t seed, uint64_t stream_pos) {
    launch(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0, s, dst, count, (int64_t)0, (uint32_t)range, seed,
           stream_pos, (float4*)nullptr, (size_t)0, (uint4*)nullptr, (size_t)0);
}

// the step's negatives into f->neg: the caller's (validated before anything is launched: range_error) or the sampler's
template <class F>
static int fold_negatives(F* f, const int64_t* negatives, uint64_t stream_pos, int64_t range, const char* range_error) {
    const int64_t count = (int64_t)f->cfg.batch_size * f->cfg.num_negatives;
    if (negatives) {
        for (int64_t i = 0; i < count; ++i)
            if (negatives[i] < 0 || negatives[i] >= range) SERT_FAIL(range_error);
        SERT_HIP(hipMemcpyAsync(f->neg_stage, negatives, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
        launch(convert_i64_to_i32, dim3(grid_for(count)), dim3(256), 0, f->stream, (const int64_t*)f->neg_stage, f->neg, count);
    } else {
        fold_sample(f->stream, f->neg, count, range, f->cfg.seed, stream_pos);
    }
    return 0;
}

// *_negatives_of_step: a stream and a buffer of its own, nothing of the handle's state is touched
template <class F>
static int fold_negatives_of_step(F* f, int64_t position, int evaluation, int64_t* out, int64_t range) {
    SERT_HIP(hipSetDevice(f->device));
    const int64_t count = (int64_t)f->cfg.batch_size * f->cfg.num_negatives;
    int32_t* tmp = nullptr;
    SERT_HIP(hipMalloc((void**)&tmp, (size_t)count * sizeof(int32_t)));
    hipStream_t st = nullptr;
    if (hipStreamCreate(&st) != hipSuccess) { (void)hipFree(tmp); SERT_FAIL("hipStreamCreate failed"); }
    fold_sample(st, tmp, count, range, f->cfg.seed, (uint64_t)position * 2 + (evaluation ? 1 : 0));
    std::vector<int32_t> host((size_t)count);
    const hipError_t e = hipMemcpyAsync(host.data(), tmp, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    (void)hipFree(tmp);
    if (e != hipSuccess || e2 != hipSuccess) SERT_FAIL("reading the negatives back failed");
    for (int64_t i = 0; i < count; ++i) out[i] = host[(size_t)i];
    return 0;
}

// ---- the end of a step ---------------------------------------------------------------------------------------------------
// the workgroups of an optimiser launch over `count` floats: each leaves one partial sum of squares
static int fold_opt_blocks(size_t count) {
    return (int)std::min<int64_t>(kOptBlocks, std::max<int64_t>(1, cdiv(cdiv((int64_t)count, 4), 256)));
}

// the step's three losses at dst: the mean of the partials and, with an L2 term, the nb partial sums of squares at f->red_sq
template <class F>
static void fold_finalize(F* f, const float* parts, int n_parts, int nb, float* dst) {
    const auto& c = f->cfg;
    const float B = (float)c.batch_size;
    launch(finalize_loss, dim3(1), dim3(256), 0, f->stream, parts, n_parts, (const float*)f->red_sq, c.lambda_ > 0.f ? nb : 0, 1.0f / B,
           c.lambda_ > 0.f ? c.lambda_ / (2.0f * B) : 0.f, dst, (unsigned*)nullptr, 0u, (const float*)nullptr);
}

// Adam over the `count` trainable floats at P with the model's arithmetic (adam_l2: L2 folded into the gradient, sum of squares
// of the values BEFORE the update from the same pass); a_t on the host in fp32 (optimizer_args); then the step's three losses
template <class F>
static void fold_adam_finalize(F* f, float* P, size_t count, const float* parts, int n_parts, float* dst) {
    const auto& c = f->cfg;
    const float B = (float)c.batch_size;
    f->step += 1;
    const float tf = (float)f->step;
    AdamArgs aa{c.lambda_ > 0.f ? c.lambda_ / B : 0.f, c.lr * sqrtf(1.0f - powf(c.beta2, tf)) / (1.0f - powf(c.beta1, tf)), c.beta1,
                c.beta2, c.eps};
    const int nb = fold_opt_blocks(count);
    launch((adam_l2<false>), dim3(nb), dim3(256), 0, f->stream, P, f->G, f->m1, f->m2, count, aa, f->red_sq, (const uint32_t*)nullptr,
           1u, (int)kRowsAll, (float*)nullptr);
    fold_finalize(f, parts, n_parts, nb, dst);
}

// Adadelta over one parameter block of a loglinear handle, `count` floats at P, with the model's arithmetic (adadelta_l2: L2
// folded into the gradient where the block has an L2 term, the sum of squares of the values BEFORE the update from the same
// pass, into sq); -> the workgroups that wrote a partial sum to sq, for fold_finalize
template <class F>
static int fold_adadelta(F* f, float* P, float* G, float* accu, float* delta, size_t count, bool l2, float* sq) {
    const auto& c = f->cfg;
    const AdadeltaArgs a{l2 && c.lambda_ > 0.f ? c.lambda_ / (float)c.batch_size : 0.f, c.lr, c.rho, c.eps};
    const int nb = fold_opt_blocks(count);
    launch((adadelta_l2<false>), dim3(nb), dim3(256), 0, f->stream, P, G, accu, delta, count, a, sq, (const uint32_t*)nullptr, 1u,
           (int)kRowsAll);
    return nb;
}

// an evaluation's loss: the mean of the partials, unregularised
template <class F>
static void fold_eval_finalize(F* f, const float* parts, int n_parts, float* dst) {
    launch(finalize_loss, dim3(1), dim3(256), 0, f->stream, parts, n_parts, parts, 0, 1.0f / (float)f->cfg.batch_size, 0.0f, dst,
           (unsigned*)nullptr, 0u, (const float*)nullptr);
}

// ---- reading and writing the handle's tensors ------------------------------------------------------------------------------
// get_rows / set_rows / get_tensor / set_tensor: ref(f, which, &count) names the tensor or returns null (which_error)
template <class F, class Ref>
static int fold_copy_tensor(F* f, int which, float* host, size_t count, bool to_host, Ref ref, const char* which_error) {
    if (!f || !host) SERT_FAIL("null argument");
    size_t have = 0;
    float* p = ref(f, which, &have);
    if (!p) SERT_FAIL(which_error);
    if (count != have) SERT_FAIL("element count mismatch");
    SERT_HIP(hipSetDevice(f->device));
    if (to_host) SERT_HIP(hipMemcpyAsync(host, p, count * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    else SERT_HIP(hipMemcpyAsync(p, host, count * sizeof(float), hipMemcpyHostToDevice, f->stream));
    SERT_HIP(hipStreamSynchronize(f->stream));
    return 0;
}

// the step and evaluation-draw counters of the sampler
static int fold_set_counter(FoldNce* f, int64_t FoldNce::*counter, int64_t value) {
    if (!f || value < 0) SERT_FAIL("bad argument");
    f->*counter = value;
    return 0;
}
static int64_t fold_get_counter(FoldNce* f, int64_t FoldNce::*counter) { return f ? f->*counter : -1; }

}  // extern "C++"
