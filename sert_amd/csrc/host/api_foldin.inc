// Part of sert_hip.hip (one translation unit; included there, inside its extern "C" block): C ABI: folding unseen entities
// into a trained vectorspace model (include/sert_hip_foldin.h: sert_foldin_*; kernels_foldin.h).  The handle copies the
// model's parameters when it is created and runs on a stream of its own: it shares nothing with the model's step schedule.

struct sert_foldin : FoldNce {
    sert_foldin_config cfg;
    int N = 0;                       // the trainable rows E (sert_foldin_create: the new rows)
    // sert_foldin_create_refresh: E is num_refresh trained rows, then num_new new rows; slot_of (Ve + num_new): the slot of a
    // row of the extended table or -1 (frozen); refresh_ids (num_refresh): the trained row of a slot.  map: the loss kernels
    // that look a candidate up in slot_of (foldin_nce_map*); sert_foldin_create leaves it false and both arrays null.
    int num_new = 0, num_refresh = 0;
    bool map = false;
    int32_t *slot_of = nullptr, *refresh_ids = nullptr;
    float* E = nullptr;              // the trainable rows (FoldNce: Adam's moments m1, m2 and the gradient G)
    float* T = nullptr;              // (M, d_e) the projections of the uploaded instances
    // per-step scratch
    int32_t *key = nullptr, *key_sorted = nullptr, *pair_sorted = nullptr, *k_tmp = nullptr, *v_tmp = nullptr;
    int32_t *sort_hist = nullptr, *sort_bin_total = nullptr;
    int sort_bits = 1;
    int32_t* run_bounds = nullptr;   // run_start (round_up(N, 4)) then run_end (the same)
    float *ehead = nullptr, *etail = nullptr;   // (chunks, d_e) carries
    // what the last step launched, recorded where the launches are made: sert_debug_foldin_plan (sert_hip_debug.h)
    int32_t plan[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

static void foldin_free_upload(sert_foldin* f) {
    (void)hipFree(f->y); (void)hipFree(f->w); (void)hipFree(f->T);
    f->y = nullptr; f->w = nullptr; f->T = nullptr; f->M = 0;
}

int sert_foldin_destroy(sert_foldin* f) {
    if (!f) return 0;
    return fold_destroy(f, foldin_free_upload,
                        {f->rw, f->W, f->b, f->re, f->E, f->m1, f->m2, f->G, f->neg, f->neg_stage, f->coef, f->key, f->key_sorted,
                         f->pair_sorted, f->k_tmp, f->v_tmp, f->sort_hist, f->sort_bin_total, f->run_bounds, f->ehead, f->etail,
                         f->rowloss, f->red_loss, f->red_sq, f->slot_of, f->refresh_ids});
}

// map == false: sert_foldin_create (refresh_ids null, num_refresh 0).  map == true: sert_foldin_create_refresh.
static int foldin_create(sert_foldin* f, sert_model* m, bool map, const int32_t* refresh_ids, int32_t num_refresh, int32_t num_new,
                         const float* init_rows, const sert_foldin_config* cfg) {
    const auto& c = m->cfg;
    // ---- validation: everything the kernels index with is checked here ----
    if (c.kind == SERT_KIND_LOGLINEAR) SERT_FAIL("a fold-in needs a vectorspace model: a loglinear model has no entity rows to add");
    if (c.kind != SERT_KIND_VECTORSPACE)
        SERT_FAIL("a fold-in needs the NCE vectorspace model: the full-softmax variant (SERT_KIND_VECTORSPACE_SOFTMAX) is not supported");
    if (m->comm || m->host_ar || m->world > 1)
        SERT_FAIL("a fold-in of a data-parallel model (a communicator is attached) is not supported");
    if (!map) {
        if (num_new < 1) SERT_FAIL("a fold-in needs at least one new entity (num_new >= 1)");
        if (!init_rows) SERT_FAIL("null argument");
    } else {
        if (num_refresh < 0 || num_new < 0) SERT_FAIL("a refresh needs num_refresh >= 0 and num_new >= 0");
        if ((int64_t)num_refresh + num_new < 1) SERT_FAIL("a refresh needs at least one trainable row (num_refresh + num_new >= 1)");
        if (num_refresh > 0 && !refresh_ids) SERT_FAIL("null refresh_ids with num_refresh > 0");
        if (num_new > 0 && !init_rows) SERT_FAIL("null init_new_rows with num_new > 0");
    }
    if (cfg->batch_size < 1 || cfg->num_negatives < 1) SERT_FAIL("a fold-in needs batch_size >= 1 and num_negatives >= 1");
    if (!(cfg->lambda_ >= 0.f)) SERT_FAIL("regularization lambda must be >= 0");
    if (c.entity_dim > 512) SERT_FAIL("entity_dim > 512 is not supported");
    if ((int64_t)c.num_entities + num_new > INT32_MAX) SERT_FAIL("more than 2^31 - 1 rows in the extended entity table");
    if ((int64_t)cfg->batch_size * (cfg->num_negatives + 1) > ((int64_t)1 << 30)) SERT_FAIL("batch_size * (num_negatives + 1) > 2^30");
    // the slot of every row of the extended table (host; uploaded below): also what finds an id out of range or given twice
    std::vector<int32_t> slot_of;
    if (map) {
        slot_of.assign((size_t)c.num_entities + (size_t)num_new, -1);
        for (int32_t s = 0; s < num_refresh; ++s) {
            const int32_t e = refresh_ids[s];
            if (e < 0 || e >= c.num_entities) SERT_FAIL("refresh id out of range [0, num_entities)");
            if (slot_of[(size_t)e] >= 0) SERT_FAIL("duplicate refresh id");
            slot_of[(size_t)e] = s;
        }
        for (int32_t e = 0; e < num_new; ++e) slot_of[(size_t)c.num_entities + e] = num_refresh + e;
    }
    SERT_HIP(hipSetDevice(c.device));
    f->device = c.device; f->cfg = *cfg;
    f->map = map; f->num_new = num_new; f->num_refresh = num_refresh;
    f->Vw = c.vocab_size; f->Ve = c.num_entities; f->N = num_refresh + num_new; f->dw = c.word_dim; f->de = c.entity_dim; f->n = c.window_size;
    const int B = cfg->batch_size, z = cfg->num_negatives, de = f->de, N = f->N;
    const size_t n_e = (size_t)N * de;
    SERT_TRY(fold_settle_model(m, true));
    SERT_TRY(fold_snapshot_vs(f, m, 0));
    SERT_HIP(hipStreamCreate(&f->stream));
    hipStream_t s = f->stream;
    SERT_TRY(dmalloc(&f->E, n_e));
    SERT_TRY(dzalloc(&f->m1, n_e, s));
    SERT_TRY(dzalloc(&f->m2, n_e, s));
    SERT_TRY(dmalloc(&f->G, n_e));
    if (!map) {
        SERT_HIP(hipMemcpyAsync(f->E, init_rows, n_e * sizeof(float), hipMemcpyHostToDevice, s));
    } else {
        const size_t n_r = (size_t)num_refresh * de;
        if (num_new > 0)
            SERT_HIP(hipMemcpyAsync(f->E + n_r, init_rows, (n_e - n_r) * sizeof(float), hipMemcpyHostToDevice, s));
        SERT_TRY(dmalloc(&f->slot_of, slot_of.size()));
        SERT_HIP(hipMemcpyAsync(f->slot_of, slot_of.data(), slot_of.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (num_refresh > 0) {
            // the refreshed slots start from the model's rows as they are now: taken on the model's stream, behind the
            // preamble above (and from the model's table, not from the snapshot: the two hold the same bits)
            SERT_TRY(dmalloc(&f->refresh_ids, (size_t)num_refresh));
            SERT_HIP(hipMemcpyAsync(f->refresh_ids, refresh_ids, (size_t)num_refresh * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
            launch(foldin_take_rows, dim3(grid_for((int64_t)n_r, 256, 1 << 16)), dim3(256), 0, m->stream, (const float*)m->re,
                   (const int32_t*)f->refresh_ids, f->E, (int64_t)num_refresh, de);
            SERT_HIP(hipGetLastError());
        }
    }
    const size_t total = (size_t)B * (z + 1);
    SERT_TRY(dmalloc(&f->neg, (size_t)B * z));
    SERT_TRY(dmalloc(&f->neg_stage, (size_t)B * z));
    SERT_TRY(dmalloc(&f->coef, total));
    SERT_TRY(dmalloc(&f->key, total));
    SERT_TRY(dmalloc(&f->key_sorted, total));
    SERT_TRY(dmalloc(&f->pair_sorted, total));
    // keys lie in [0, N] (N: the sentinel of a pair on a frozen row)
    f->sort_bits = 1;
    while (((int64_t)1 << f->sort_bits) <= (int64_t)N) ++f->sort_bits;
    if (f->sort_bits > kSortMaxBits) {
        SERT_TRY(dmalloc(&f->k_tmp, total));
        SERT_TRY(dmalloc(&f->v_tmp, total));
    }
    SERT_TRY(dmalloc(&f->sort_hist, (size_t)kSortMaxBins * cdiv((int64_t)total, kSortTile)));
    SERT_TRY(dmalloc(&f->sort_bin_total, (size_t)kSortMaxBins));
    SERT_TRY(dzalloc(&f->run_bounds, 2 * round_up((size_t)N, 4), s));
    const size_t chunks = (size_t)cdiv((int64_t)total, kEChunk);
    SERT_TRY(dmalloc(&f->ehead, chunks * de));
    SERT_TRY(dmalloc(&f->etail, chunks * de));
    SERT_TRY(dmalloc(&f->rowloss, (size_t)B));
    SERT_TRY(dmalloc(&f->red_loss, (size_t)cdiv(B, 16)));
    SERT_TRY(dmalloc(&f->red_sq, (size_t)kOptBlocks));
    SERT_TRY(dmalloc(&f->d_loss, (size_t)3));
    return fold_created(f, m);      // (init_rows is borrowed for the call only)
}

int sert_foldin_create(sert_model* m, int32_t num_new, const float* init_rows, const sert_foldin_config* cfg, sert_foldin** out) {
    refresh_gemm_choice();
    return fold_create(m, cfg, out, "sert_foldin_config size mismatch (ABI)", sert_foldin_destroy,
                       [&](sert_foldin* f) { return foldin_create(f, m, false, nullptr, 0, num_new, init_rows, cfg); });
}

int sert_foldin_create_refresh(sert_model* m, const int32_t* refresh_ids, int32_t num_refresh, int32_t num_new,
                               const float* init_new_rows, const sert_foldin_config* cfg, sert_foldin** out) {
    refresh_gemm_choice();
    return fold_create(m, cfg, out, "sert_foldin_config size mismatch (ABI)", sert_foldin_destroy, [&](sert_foldin* f) {
        return foldin_create(f, m, true, refresh_ids, num_refresh, num_new, init_new_rows, cfg);
    });
}

int sert_foldin_upload(sert_foldin* f, const int32_t* x, const int32_t* y, const float* w, int64_t M) {
    refresh_gemm_choice();
    if (!f || M < 0 || (M > 0 && (!x || !y))) SERT_FAIL("bad argument");
    if (M > ((int64_t)1 << 31) - 1) SERT_FAIL("more than 2^31 - 1 fold-in instances");
    const int n = f->n;
    // host-side validation: no kernel is launched on bad ids
    for (int64_t i = 0; i < M; ++i)
        if (y[i] < 0 || y[i] >= f->N)
            SERT_FAIL(f->map ? "fold-in label out of range [0, num_refresh + num_new): y is a slot"
                             : "fold-in label out of range [0, num_new)");
    for (int64_t i = 0; i < M * n; ++i)
        if (x[i] < 0 || x[i] >= f->Vw) SERT_FAIL("token id out of range [0, vocab_size)");
    SERT_HIP(hipSetDevice(f->device));
    SERT_HIP(hipStreamSynchronize(f->stream));
    foldin_free_upload(f);
    if (M == 0) return 0;
    std::vector<float> ones;
    auto body = [&]() -> int {
        SERT_TRY(fold_upload_labels(f, y, w, M, ones));
        SERT_TRY(dmalloc(&f->T, (size_t)M * f->de));
        // T = tanh(h W + b) once
        return fold_project_slabs<EPI_BIAS_TANH>(f, x, M, f->T, nullptr);
    };
    const int rc = body();
    if (rc != 0) return fold_upload_failed(f, rc, foldin_free_upload);
    f->M = M;
    return 0;
}

int64_t sert_foldin_num_batches(sert_foldin* f) { return fold_num_batches(f); }

// the step's negatives into f->neg, over the extended table
static int foldin_negatives(sert_foldin* f, const int64_t* negatives, uint64_t stream_pos) {
    return fold_negatives(f, negatives, stream_pos, (int64_t)f->Ve + f->num_new,
                          "negative sample out of range [0, num_entities + num_new)");
}

// the loss kernel on batch `batch` (train: weighted, coef and keys written); *parts / *n_parts: the loss partials it left.
// A handle made by sert_foldin_create_refresh (f->map) launches the instance of foldin_nce_map / foldin_nce_map_scalar.
static int foldin_loss(sert_foldin* f, int64_t batch, bool train, const float** parts, int* n_parts) {
    const int B = f->cfg.batch_size, z = f->cfg.num_negatives, de = f->de;
    const size_t row0 = (size_t)batch * B;
    const float* T = f->T + row0 * de;
    const int32_t* y = f->y + row0;
    const float* w = train ? f->w + row0 : (const float*)nullptr;
    const float inv_batch = 1.0f / (float)B;
    const bool vector = de % 4 == 0;      // 16 lanes per instance and float4 columns; else one wave per instance
    const dim3 grid(cdiv(B, vector ? 16 : 4)), block(256);
    // one instance of the two-part table's kernel or of the slot map's; tail: the arguments behind inv_batch
    auto go = [&](auto two_part, auto map, auto... tail) {
        if (f->map)
            launch(map, grid, block, 0, f->stream, T, f->re, f->E, f->slot_of, y, f->neg, w, f->coef, f->key, f->rowloss, B, z, de,
                   f->N, inv_batch, tail...);
        else
            launch(two_part, grid, block, 0, f->stream, T, f->re, f->E, y, f->neg, w, f->coef, f->key, f->rowloss, B, z, de, f->Ve,
                   f->N, inv_batch, tail...);
    };
    const int k = vector ? cdiv(de / 4, 16) : cdiv(de, 64);
    const bool launched = vector ? dispatch_int<1, 8>(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (train) go(foldin_nce<K, true>, foldin_nce_map<K, true>, f->red_loss);
        else go(foldin_nce<K, false>, foldin_nce_map<K, false>, f->red_loss);
    }) : dispatch_int<1, 8>(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (train) go(foldin_nce_scalar<K, true>, foldin_nce_map_scalar<K, true>);
        else go(foldin_nce_scalar<K, false>, foldin_nce_map_scalar<K, false>);
    });
    if (!launched) SERT_FAIL("entity_dim > 512 is not supported");
    // (the scalar layout leaves no workgroup partials: the rows' losses themselves)
    *parts = vector ? f->red_loss : f->rowloss;
    *n_parts = vector ? cdiv(B, 16) : B;
    f->plan[0] = vector ? SERT_FOLDIN_LOSS_VECTOR : SERT_FOLDIN_LOSS_SCALAR; f->plan[1] = k; f->plan[2] = train ? 1 : 0;
    return 0;
}

// dE (data term) into f->G: stable sort of the (key, pair) entries, chunked reduce that stops at the sentinel N, carry fix-up
// over the N trainable rows -- the model's chain (lazy_segsum.inc: EntityChain) over this handle's buffers
static int foldin_grad(sert_foldin* f, int64_t batch) {
    const int B = f->cfg.batch_size, z = f->cfg.num_negatives, de = f->de, N = f->N;
    const int total = B * (z + 1);
    const int nbound = (int)round_up((size_t)N, 4);
    const EntityChain chain = {f->key_sorted, f->pair_sorted, f->k_tmp, f->v_tmp, f->sort_hist, f->sort_bin_total, f->run_bounds,
                               f->run_bounds + nbound, 2 * nbound, f->ehead, f->etail, f->sort_bits, N, de, z + 1, total};
    const ChainSorted sorted = entity_key_sort(chain, f->key, f->stream);
    f->plan[3] = sorted.bits; f->plan[4] = sorted.passes; f->plan[9] = (int32_t)cdiv((int64_t)total, kSortTile);
    const ChainReduced reduced = entity_chunk_reduce(chain, f->coef, f->T + (size_t)batch * B * de, f->G, f->stream, N);
    f->plan[5] = reduced.vec; f->plan[6] = reduced.nch; f->plan[7] = cdiv(de / reduced.vec, 16 * reduced.nch);
    f->plan[8] = entity_fixup(chain, f->G, f->stream);
    return 0;
}

static int foldin_check_batch(sert_foldin* f, int64_t batch) {
    return fold_check_batch(f, &sert_foldin::T, "sert_foldin_upload", batch);
}

// one step enqueued on the handle's stream; dst: 3 floats on the device (finalize_loss: loss, data term, regulariser)
static int foldin_step_async(sert_foldin* f, int64_t batch, const int64_t* negatives, float* dst) {
    SERT_TRY(foldin_negatives(f, negatives, (uint64_t)f->step * 2));
    const float* parts = nullptr;
    int n_parts = 0;
    SERT_TRY(foldin_loss(f, batch, true, &parts, &n_parts));
    SERT_TRY(foldin_grad(f, batch));
    fold_adam_finalize(f, f->E, (size_t)f->N * f->de, parts, n_parts, dst);
    return 0;
}

int sert_foldin_train_batch(sert_foldin* f, int64_t batch, const int64_t* negatives, float* loss_out) {
    return fold_run_batch(f, batch, loss_out, foldin_check_batch,
                          [&](sert_foldin* h, int64_t b, float* dst) { return foldin_step_async(h, b, negatives, dst); });
}

int sert_foldin_train_batches(sert_foldin* f, const int64_t* batches, int64_t count, float* losses_out) {
    return fold_train_batches(f, batches, count, losses_out, foldin_check_batch,
                              [](sert_foldin* h, int64_t b, float* dst) { return foldin_step_async(h, b, nullptr, dst); });
}

int sert_foldin_eval_batch(sert_foldin* f, int64_t batch, const int64_t* negatives, float* loss_out) {
    return fold_run_batch(f, batch, loss_out, foldin_check_batch, [&](sert_foldin* h, int64_t b, float* dst) {
        SERT_TRY(foldin_negatives(h, negatives, (uint64_t)h->eval_draws * 2 + 1));
        if (!negatives) ++h->eval_draws;
        const float* parts = nullptr;
        int n_parts = 0;
        SERT_TRY(foldin_loss(h, b, false, &parts, &n_parts));
        fold_eval_finalize(h, parts, n_parts, dst);
        return 0;
    });
}

int sert_foldin_negatives_of_step(sert_foldin* f, int64_t position, int evaluation, int64_t* out) {
    if (!f || !out || position < 0) SERT_FAIL("bad argument");
    return fold_negatives_of_step(f, position, evaluation, out, (int64_t)f->Ve + f->num_new);
}

static float* foldin_rows_ref(sert_foldin* f, int which, size_t* count) {
    *count = (size_t)f->N * f->de;
    return which == SERT_FOLDIN_ROWS ? f->E : which == SERT_FOLDIN_M ? f->m1 : which == SERT_FOLDIN_V ? f->m2 : nullptr;
}
static const char* const kFoldinWhich = "which must be SERT_FOLDIN_ROWS, SERT_FOLDIN_M or SERT_FOLDIN_V";

int sert_foldin_get_rows(sert_foldin* f, int which, float* host, size_t count) {
    return fold_copy_tensor(f, which, host, count, true, foldin_rows_ref, kFoldinWhich);
}
int sert_foldin_set_rows(sert_foldin* f, int which, const float* host, size_t count) {
    return fold_copy_tensor(f, which, const_cast<float*>(host), count, false, foldin_rows_ref, kFoldinWhich);
}

int sert_foldin_set_step(sert_foldin* f, int64_t t) { return fold_set_counter(f, &FoldNce::step, t); }
int64_t sert_foldin_get_step(sert_foldin* f) { return fold_get_counter(f, &FoldNce::step); }
int sert_foldin_set_eval_draws(sert_foldin* f, int64_t n) { return fold_set_counter(f, &FoldNce::eval_draws, n); }
int64_t sert_foldin_get_eval_draws(sert_foldin* f) { return fold_get_counter(f, &FoldNce::eval_draws); }

int sert_debug_foldin_plan(sert_foldin* f, int32_t* out, int n) {
    if (!f || !out || n < 1 || n > 10) SERT_FAIL("bad argument");
    for (int i = 0; i < n; ++i) out[i] = f->plan[i];
    return 0;
}

int sert_debug_foldin_table(sert_foldin* f, int32_t* out, int n) {
    if (!f || !out || n < 1 || n > 4) SERT_FAIL("bad argument");
    const int32_t v[4] = {f->map ? 1 : 0, f->num_refresh, f->num_new, f->N};
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return 0;
}
