// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): C ABI: errors, devices, sert_create / sert_destroy, tensors, step counters, negatives.

const char* sert_last_error(void) { return g_last_error.c_str(); }

int sert_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int sert_device_info(int device, char* buf, size_t buflen) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) {
        g_last_error = "hipGetDeviceProperties failed";
        return -1;
    }
    return snprintf(buf, buflen, "%s %s: %d CUs, %.0f MHz, %.1f GiB, LDS/block %zu KiB", p.name,
                    p.gcnArchName, p.multiProcessorCount, p.clockRate / 1000.0,
                    p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0), p.sharedMemPerBlock / 1024);
}

static int create_resources(sert_model* m);
static int layout_gradients(sert_model* m);

// Data parallel: give every big tensor its ZeRO-1 geometry for (world, ar_chunks): parameters and
// gradients are re-allocated with the padding that makes the slabs equal, the optimiser state
// shrinks to the owned pieces (whatever it held so far is kept).
static int shard_setup(sert_model* m) {
    if (m->cfg.inference_only) SERT_FAIL("model was created inference_only");
    for (int i = 0; i < 4; ++i)
        if (m->pt_sharded[i]) SERT_FAIL("this model already has a data-parallel communicator");
    hipStream_t s = m->stream;
    SERT_TRY(ensure_rw_current(m, -1));    // (data parallel runs the dense update: no row may be behind)
    SERT_HIP(hipStreamSynchronize(s));
    SERT_HIP(hipStreamSynchronize(m->stream2));
    if (m->stream3) SERT_HIP(hipStreamSynchronize(m->stream3));
    float** P[4] = {&m->rw, &m->re, &m->W, &m->b};
    float** S0[4] = {&m->s0_rw, &m->s0_re, &m->s0_w, &m->s0_b};
    float** S1[4] = {&m->s1_rw, &m->s1_re, &m->s1_w, &m->s1_b};
    const size_t n[4] = {m->n_rw, m->n_re, m->n_w, m->n_b};
    for (int i = 0; i < 4; ++i) {
        if (!m->pt_big[i]) continue;
        const size_t unit = (size_t)m->world * (size_t)m->ar_chunks;
        size_t sc = round_up((n[i] + unit - 1) / unit, 64);
        if (i == 0 && m->xr_mode) {
            // owned by rows: a piece is a whole number of rows (a multiple of 16, so that it stays a
            // multiple of 64 elements)
            m->xr_rows_per_rank = (int64_t)round_up(cdiv((int64_t)m->cfg.vocab_size, m->world), 16);
            sc = (size_t)m->xr_rows_per_rank * (size_t)m->cfg.word_dim;
        }
        const size_t pad = sc * unit;
        float *np = nullptr, *ns0 = nullptr, *ns1 = nullptr;
        SERT_TRY(dzalloc(&np, pad, s));
        SERT_HIP(hipMemcpyAsync(np, *P[i], n[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
        SERT_TRY(dzalloc(&ns0, sc * m->ar_chunks, s));
        SERT_TRY(dzalloc(&ns1, sc * m->ar_chunks, s));
        for (int c = 0; c < m->ar_chunks; ++c) {
            const size_t off = (size_t)c * sc * m->world + (size_t)m->rank * sc;
            if (off >= n[i]) continue;
            const size_t cnt = std::min(sc, n[i] - off);
            SERT_HIP(hipMemcpyAsync(ns0 + (size_t)c * sc, *S0[i] + off, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
            SERT_HIP(hipMemcpyAsync(ns1 + (size_t)c * sc, *S1[i] + off, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        SERT_HIP(hipStreamSynchronize(s));
        (void)hipFree(*P[i]); (void)hipFree(*S0[i]); (void)hipFree(*S1[i]);
        *P[i] = np; *S0[i] = ns0; *S1[i] = ns1;
        m->pt_pad[i] = pad;
        m->pt_sc[i] = sc;
        m->pt_sharded[i] = true;
    }
    return layout_gradients(m);
}

// Optimiser state of a sharded tensor <-> a full-size host array.  get is COLLECTIVE (every rank
// calls it, in the same order): the owned pieces are all-gathered into a scratch tensor.
static int sharded_state_io(sert_model* m, int i, int k, float* host_out, const float* host_in) {
    const ParamTensor t = param_tensor(m, i);
    float* st = k == 0 ? t.s0 : t.s1;
    const size_t sc = m->pt_sc[i], pad = m->pt_pad[i], n = t.n;
    hipStream_t s = m->stream;
    if (host_in) {
        for (int c = 0; c < m->ar_chunks; ++c) {
            const size_t off = piece_off(m, i, c);
            SERT_HIP(hipMemsetAsync(st + (size_t)c * sc, 0, sc * sizeof(float), s));
            if (off < n)
                SERT_HIP(hipMemcpyAsync(st + (size_t)c * sc, host_in + off, std::min(sc, n - off) * sizeof(float),
                                        hipMemcpyHostToDevice, s));
        }
        SERT_HIP(hipStreamSynchronize(s));
        return 0;
    }
    if (m->comm_dead) SERT_FAIL("the communicator of this data-parallel model was destroyed");
    float* full = nullptr;
    SERT_TRY(dzalloc(&full, pad, s));
    for (int c = 0; c < m->ar_chunks; ++c)
        SERT_HIP(hipMemcpyAsync(full + piece_off(m, i, c), st + (size_t)c * sc, sc * sizeof(float), hipMemcpyDeviceToDevice, s));
    int rc = 0;
    if (m->host_ar) {
        for (int c = 0; c < m->ar_chunks && rc == 0; ++c) rc = host_allgather(m, full + (size_t)c * slab_elems(m, i), sc, s);
    } else {
        for (int c = 0; c < m->ar_chunks && rc == 0; ++c)
            if (g_rccl.AllGather(full + piece_off(m, i, c), full + (size_t)c * slab_elems(m, i), sc, 7, m->comm, s) != 0)
                rc = fail(__FILE__, __LINE__, "ncclAllGather failed (optimiser state)");
    }
    if (rc == 0 && hipMemcpyAsync(host_out, full, n * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(__FILE__, __LINE__, "copy of the gathered optimiser state failed");
    (void)hipStreamSynchronize(s);
    (void)hipFree(full);
    return rc;
}

// The events that order this model's own streams against each other.  device_scope: without the SYSTEM-scope release
// (hipEventDisableSystemFence) -- right while every consumer is a kernel on this device.  A model with a communicator
// (sert_comm_init / sert_comm_init_host) re-creates them with HIP's default flags: there ev_join / ev_dense / ev_fork also
// stand in front of a D2H copy (host transport) or a collective whose readers are peers, and an agent-scope release does
// not make the gradients visible to those (advisor, round 5).
static int create_intra_events(sert_model* m, bool device_scope) {
    hipEvent_t* evs[] = {&m->ev_join3, &m->ev_step_done, &m->ev_neg, &m->ev_opt_fork,
                         &m->ev_dense, &m->ev_small, &m->ev_re, &m->ev_fork, &m->ev_join};
    const unsigned flags = hipEventDisableTiming | (device_scope ? (unsigned)hipEventDisableSystemFence : 0u);
    for (hipEvent_t* e : evs) {
        if (*e) { SERT_HIP(hipEventDestroy(*e)); *e = nullptr; }
        SERT_HIP(hipEventCreateWithFlags(e, flags));
    }
    m->events_device_scope = device_scope;
    return 0;
}

int sert_create(const sert_config* cfg, sert_model** out) {
    if (!cfg || !out) SERT_FAIL("null argument");
    if (cfg->struct_size != sizeof(sert_config)) SERT_FAIL("sert_config size mismatch (ABI)");
    if (cfg->kind != SERT_KIND_LOGLINEAR && cfg->kind != SERT_KIND_VECTORSPACE &&
        cfg->kind != SERT_KIND_VECTORSPACE_SOFTMAX)
        SERT_FAIL("bad kind");
    if (cfg->batch_size <= 0 || cfg->window_size <= 0 || cfg->vocab_size <= 0 ||
        cfg->num_entities <= 0 || cfg->word_dim <= 0)
        SERT_FAIL("sizes must be positive");
    if (cfg->global_batch_size < cfg->batch_size) SERT_FAIL("global_batch_size < batch_size");
    if (cfg->id_bytes != 1 && cfg->id_bytes != 2 && cfg->id_bytes != 4) SERT_FAIL("id_bytes must be 1, 2 or 4");
    if (cfg->kind != SERT_KIND_LOGLINEAR) {
        if (cfg->entity_dim <= 0 || cfg->entity_dim > 512) SERT_FAIL("entity_dim must be in [1, 512]");
        if (cfg->num_negatives < 0) SERT_FAIL("num_negatives must be >= 0");
    }
    SERT_HIP(hipSetDevice(cfg->device));
    sert_model* m = new sert_model();
    m->cfg = *cfg;
    // everything below may fail half-way (out of memory, ...): the partially built model is
    // torn down by sert_destroy, which tolerates null members
    const int rc = create_resources(m);
    if (rc != 0) {
        const std::string why = g_last_error;   // sert_destroy must not clobber the message
        sert_destroy(m);
        g_last_error = why;
        return rc;
    }
    *out = m;
    return 0;
}

// (Re)build the flat gradient buffer [g_rw | g_re | g_w | g_b | loss sum, owned sum of squares,
// pad | per-entity run bounds] for the current paddings pt_pad[] (every sub-tensor 16-byte aligned).
static int layout_gradients(sert_model* m) {
    const bool vs = is_vs(m);
    const size_t V = m->cfg.num_entities;
    // Order inside the buffer: the word table first (gflat[0, ar_split)), then the other SHARDED
    // tensors, then the replicated ones -- whatever their index: a loglinear model has no R_e and
    // may have a big W (d_w V_e > 4 M), a vectorspace model a small R_e beside a big W -- so that
    // the replicated remainder [rest_off, gflat_count) is one contiguous all-reduce.
    size_t off[5];
    size_t cur = 0;
    auto place = [&](int i) { off[i] = cur; cur += round_up(m->pt_pad[i], 4); };
    place(0);
    m->ar_split = cur;
    for (int i = 1; i < 4; ++i) if (m->pt_sharded[i]) place(i);
    m->rest_off = m->pt_sharded[0] ? cur : 0;
    for (int i = 1; i < 4; ++i) if (!m->pt_sharded[i]) place(i);
    off[4] = cur;
    m->gflat_count = off[4] + 4;
    // tail of the same allocation (zeroed with the gradients every step, not part of any
    // exchange): per-entity sorted-run bounds
    m->gflat_alloc = m->gflat_count + (vs ? 2 * round_up(V, 4) : 0);
    if (m->gflat) { SERT_HIP(hipStreamSynchronize(m->stream)); (void)hipFree(m->gflat); m->gflat = nullptr; }
    SERT_TRY(dzalloc(&m->gflat, m->gflat_alloc, m->stream));
    if (vs) {
        m->run_start = (int32_t*)(m->gflat + m->gflat_count);
        m->run_end = m->run_start + round_up(V, 4);
    }
    m->g_rw = m->gflat + off[0];
    m->g_re = m->n_re ? m->gflat + off[1] : nullptr;
    m->g_w = m->gflat + off[2];
    m->g_b = m->gflat + off[3];
    m->g_loss = m->gflat + off[4];
    m->g_sq = m->g_loss + 1;
    return 0;
}

static int create_resources(sert_model* m) {
    const auto& c = m->cfg;
    SERT_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    SERT_HIP(hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking));
    // The opt-in schedule that needs a third queue (SERT_STREAMS=3) creates it; by default it does not exist:
    // HIP maps streams onto FOUR hardware queues, and a fifth stream -- the communication stream of a
    // data-parallel model -- would share one with the main stream (its kernels then queue behind the
    // main stream's, and every cross-stream event costs 10-30 us instead of ~6)
    {
        const char* e3 = knob("SERT_STREAMS");
        if (e3 && atoi(e3) >= 3) SERT_HIP(hipStreamCreateWithFlags(&m->stream3, hipStreamNonBlocking));
    }
    // Events that only order this device's own streams against each other need no SYSTEM-scope release (the cache
    // write-back + invalidate that makes device memory visible to the host and to other devices): every kernel ends with
    // an agent-scope release already.  hipEventDisableSystemFence; SERT_EVENT_FENCE=system restores the default flags.
    // (ev_loss is waited on by the HOST and keeps them; so do the events of a communicator, whose consumers may be peers.)
    // (opt-in: measured SLOWER than the two launches at C2 -- 53 us against 25 + 25 -- and equal at 8192 rows; kernels_proj.h)
    m->proj_fused = variant_knob("SERT_PROJ_FUSED") && atoi(variant_knob("SERT_PROJ_FUSED")) != 0;
    m->lazy_skip = !(knob("SERT_LAZY_SKIP") && atoi(knob("SERT_LAZY_SKIP")) == 0);
    m->lazy_max = knob("SERT_LAZY_MAX") ? (float)atof(knob("SERT_LAZY_MAX")) : 0.5f;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->cfg.device) != hipSuccess || cus <= 0) cus = 256;
        m->num_cus = cus;
    }
    const char* fence_env = knob("SERT_EVENT_FENCE");
    SERT_TRY(create_intra_events(m, !(fence_env && !strcmp(fence_env, "system"))));
    SERT_HIP(hipEventCreateWithFlags(&m->ev_loss, hipEventDisableTiming));
    const size_t B = c.batch_size, n = c.window_size, dw = c.word_dim, V = c.num_entities;
    const bool vs = is_vs(m);
    const size_t de = vs ? c.entity_dim : 0;
    m->n_rw = (size_t)c.vocab_size * dw;
    m->n_re = vs ? V * de : 0;
    m->n_w = vs ? dw * de : dw * V;
    m->n_b = vs ? de : V;
    hipStream_t s = m->stream;
    {
        const size_t n[4] = {m->n_rw, m->n_re, m->n_w, m->n_b};
        for (int i = 0; i < 4; ++i) {
            m->pt_pad[i] = n[i];
            // the word table always has its own streaming launch; R_e / W beyond 4 M elements too
            m->pt_big[i] = n[i] > 0 && (i == 0 || (i < 3 && n[i] > ((size_t)1 << 22)));
            m->pt_sharded[i] = false;
        }
    }
    SERT_TRY(dzalloc(&m->rw, m->n_rw, s));  SERT_TRY(dzalloc(&m->re, m->n_re, s));
    SERT_TRY(dzalloc(&m->W, m->n_w, s));    SERT_TRY(dzalloc(&m->b, m->n_b, s));
    if (!c.inference_only) {
        SERT_TRY(dzalloc(&m->s0_rw, m->n_rw, s)); SERT_TRY(dzalloc(&m->s0_re, m->n_re, s));
        SERT_TRY(dzalloc(&m->s0_w, m->n_w, s));   SERT_TRY(dzalloc(&m->s0_b, m->n_b, s));
        SERT_TRY(dzalloc(&m->s1_rw, m->n_rw, s)); SERT_TRY(dzalloc(&m->s1_re, m->n_re, s));
        SERT_TRY(dzalloc(&m->s1_w, m->n_w, s));   SERT_TRY(dzalloc(&m->s1_b, m->n_b, s));
        // the lazy word-table update's per-row update counters (two: the kernel reads one and writes the other)
        static const bool no_lazy = variant_knob("SERT_NO_LAZY") != nullptr;   // cross-check knob (variants build)
        if (!no_lazy && c.word_dim % 4 == 0) {
            SERT_TRY(dzalloc(&m->rw_last[0], (size_t)c.vocab_size, s));
            SERT_TRY(dzalloc(&m->rw_last[1], (size_t)c.vocab_size, s));
            m->rw_pred_stride = (unsigned)round_up((size_t)c.vocab_size, 64);
            SERT_TRY(dzalloc(&m->rw_pred, (size_t)kLazyK * m->rw_pred_stride, s));
        }
        SERT_TRY(layout_gradients(m));
        SERT_TRY(dzalloc(&m->rowloss, B, s));
        size_t part = 0;
        if (vs) {
            SERT_TRY(dzalloc(&m->H, B * dw, s));  SERT_TRY(dzalloc(&m->T, B * de, s));
            if (c.kind == SERT_KIND_VECTORSPACE && !c.inference_only) SERT_TRY(dzalloc(&m->T_alt, B * de, s));
            SERT_TRY(dzalloc(&m->DA, B * de, s)); SERT_TRY(dzalloc(&m->DH, B * dw, s));
            SERT_TRY(dzalloc(&m->neg, std::max<size_t>(4, B * c.num_negatives), s));
            SERT_TRY(dzalloc(&m->neg_alt, std::max<size_t>(4, B * c.num_negatives), s));
            SERT_TRY(dzalloc(&m->neg_stage, std::max<size_t>(4, B * c.num_negatives), s));
            part = (size_t)1024 * (dw * de + de);
            if (c.kind == SERT_KIND_VECTORSPACE_SOFTMAX) {
                // The logit matrix is never larger than ~1.7 GB (SERT_FS_TILE_MB): beyond that the step walks
                // row tiles -- logits, softmax cross-entropy, dR_e += dZ^T.p and dp = dZ.R_e per tile -- so the
                // C4 configuration (65536 x 100 000 logits = 26 GB as one matrix) needs 1.6 GB of scratch.
                // SERT_FS_TILE_ROWS forces a tile height (tests).
                {
                    const char* em = variant_knob("SERT_FS_TILE_MB");
                    const size_t cap = (size_t)(em && atoi(em) > 0 ? atoi(em) : 1700) << 20;
                    size_t tile = B;
                    if (B * V * sizeof(float) > cap) tile = std::max<size_t>(256, (cap / (V * sizeof(float))) / 256 * 256);
                    const char* er = knob("SERT_FS_TILE_ROWS");
                    if (er && atoi(er) > 0) tile = (size_t)atoi(er);
                    m->fs_tile = (int)std::min<size_t>(B, tile);
                }
                SERT_TRY(dzalloc(&m->Z, (size_t)m->fs_tile * V, s));       // logits -> dL/dlogits, one row tile
                SERT_TRY(dzalloc(&m->DH2, B * de, s));    // p = clip(t)
                const size_t tiles = (size_t)cdiv(de, GN) * cdiv(V, GM);
                const size_t sp = std::max<size_t>(1, cdiv(1024, tiles)) + 1;
                part = std::max(part, sp * V * de);
            }
            const size_t total = B * (c.num_negatives + 1);
            {
                // sort-free entity gradient for small vocabularies (kernels_egrad.h); SERT_EGRAD_SORT=1
                // keeps the sorted path (cross-check knob)
                const bool force_sort = knob("SERT_EGRAD_SORT") && atoi(knob("SERT_EGRAD_SORT")) != 0;   // (read per model)
                m->egrad_force_sort = force_sort;
                m->egrad_ranges = variant_knob("SERT_EGRAD_RANGES") && atoi(variant_knob("SERT_EGRAD_RANGES")) != 0;
                const size_t c1 = c.num_negatives + 1;
                if (!force_sort && c.kind == SERT_KIND_VECTORSPACE && V <= 2048 && de % 4 == 0 && de <= 128 &&
                    total < ((size_t)1 << 27) && c1 <= (size_t)kElSubPairs) {
                    m->eg_er_shift = 4;                                      // 16 entities per range (egrad_acc)
                    m->eg_ranges = cdiv(V, 16);                              // <= 128 = kElMaxRanges
                    m->eg_sub_rows = (int)std::min<size_t>(256, kElSubPairs / c1);
                    // small batches: finer sub-groups and row groups, so that the accumulation still
                    // launches ~16 row groups x ranges workgroups with all four waves at work
                    // (batch 4096 was ONE row group: 63 workgroups, 31 us; now 16 x 63)
                    while (m->eg_sub_rows > 32 && (size_t)B < (size_t)64 * m->eg_sub_rows) m->eg_sub_rows /= 2;
                    m->eg_num_sub = cdiv(B, m->eg_sub_rows);
                    // row groups whose slice of T (rows x d_e floats) stays in one XCD's L2: <= 2 MB
                    m->eg_subs_per_group = (int)std::max<size_t>(1, (((size_t)2 << 20) / (de * sizeof(float))) / m->eg_sub_rows);
                    static const int want_groups = variant_knob("SERT_EG_GROUPS") ? std::max(1, atoi(variant_knob("SERT_EG_GROUPS"))) : 16;   // tuning knob
                    m->eg_subs_per_group = std::max(1, std::min(m->eg_subs_per_group, m->eg_num_sub / want_groups));
                    m->eg_groups = cdiv(m->eg_num_sub, m->eg_subs_per_group);
                }
                if (m->eg_groups > 0) {
                    SERT_TRY(dzalloc(&m->epart, (size_t)m->eg_groups * V * de, s));
                    SERT_TRY(dzalloc(&m->eg_entries, total, s));
                    SERT_TRY(dzalloc(&m->eg_offs, (size_t)m->eg_num_sub * (m->eg_ranges + 1), s));
                }
            }
            SERT_TRY(dzalloc(&m->cand, total, s));        SERT_TRY(dzalloc(&m->cand_sorted, total + 1, s));
            SERT_TRY(dzalloc(&m->cand_early, total, s));
            SERT_TRY(dzalloc(&m->pair_sorted, total, s));
            SERT_TRY(dzalloc(&m->coef, total, s));
            const size_t chunks = (total + kEChunk - 1) / kEChunk;
            SERT_TRY(dzalloc(&m->ehead, chunks * de, s)); SERT_TRY(dzalloc(&m->etail, chunks * de, s));
            m->sort_bits = 1;
            while ((1ll << m->sort_bits) < (long long)V) ++m->sort_bits;
            const size_t tiles = (total + kSortTile - 1) / kSortTile;
            SERT_TRY(dzalloc(&m->sort_hist, (size_t)kSortMaxBins * tiles, s));
            SERT_TRY(dzalloc(&m->sort_bin_total, (size_t)kSortMaxBins, s));
            if (m->sort_bits > kSortMaxBits) {
                SERT_TRY(dzalloc(&m->sort_k_tmp, total, s));
                SERT_TRY(dzalloc(&m->sort_v_tmp, total, s));
            }
        } else {
            // the fused loss kernel may ask for more than the default 64 KB of dynamic LDS
#define SERT_LL_ATTR(NT)                                                                                  \
    SERT_HIP(hipFuncSetAttribute((const void*)ll_fused_row<true, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024)); \
    SERT_HIP(hipFuncSetAttribute((const void*)ll_fused_row<false, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024))
            SERT_LL_ATTR(512);
            SERT_HIP(hipFuncSetAttribute((const void*)ll_row_from_table<512>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
#undef SERT_LL_ATTR
            SERT_TRY(dzalloc(&m->G, B * n * dw, s));  SERT_TRY(dzalloc(&m->Z, B * n * V, s));
            SERT_TRY(dzalloc(&m->J, B * V, s));       SERT_TRY(dzalloc(&m->DG, B * n * dw, s));
            const size_t nseg = cdiv(V, kLlSeg);
            SERT_TRY(dzalloc(&m->ll_tokstat, B * n * nseg, s)); SERT_TRY(dzalloc(&m->ll_lse, B * n, s));
            SERT_TRY(dzalloc(&m->ll_jstat, B * nseg, s));       SERT_TRY(dzalloc(&m->ll_rowinfo, B, s));
            SERT_TRY(dzalloc(&m->ll_rpart, B * n * nseg, s));   SERT_TRY(dzalloc(&m->ll_r, B * n, s));
            SERT_TRY(dzalloc(&m->ll_rsum, B * n, s));
            const size_t tiles = (size_t)cdiv(V, GN) * cdiv(dw, GM);
            const size_t splits = std::max<size_t>(1, cdiv(1024, tiles)) + 1;
            part = splits * (dw * V + V);
        }
        m->part_count = part;
        SERT_TRY(dzalloc(&m->part, part, s));
        SERT_TRY(dzalloc(&m->red_loss, std::max<size_t>((size_t)kOptBlocks, (B + 15) / 16), s));
        SERT_TRY(dzalloc(&m->red_sq, (size_t)8 * kOptBlocks, s));  // partials of up to 4 tensors (<= 2 kOptBlocks each)
        SERT_TRY(dzalloc(&m->re_sq, (size_t)4 * kOptBlocks, s));
        SERT_TRY(dzalloc(&m->sq_scratch, (size_t)8 * kOptBlocks, s));
        SERT_TRY(dzalloc(&m->d_loss, (size_t)4, s));
        if (vs) {
            SERT_TRY(dzalloc(&m->tail_blk, (size_t)4 * (cdiv((int64_t)(m->n_w + m->n_b), 64) + 1), s));
        }
    }
    // pinned, device-mapped: [loss, data, reg, -, seq]; the step's last kernel writes it directly
    SERT_HIP(hipHostMalloc((void**)&m->h_loss, 8 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
    memset(m->h_loss, 0, 8 * sizeof(float));
    SERT_HIP(hipHostGetDevicePointer((void**)&m->h_loss_dev, m->h_loss, 0));
    {
        const char* e = knob("SERT_STREAMS");   // tuning / cross-check knob
        const int v = e ? atoi(e) : 0;
        if (v >= 1 && v <= 3) m->nstreams = v;
    }
    for (int g = 0; g < TG_COUNT; ++g)
        for (int k = 0; k < 2; ++k) SERT_HIP(hipEventCreate(&m->timing.ev[g][k]));
    m->timing.created = true;
    SERT_HIP(hipStreamSynchronize(s));
    return 0;
}

static void free_split(DataSplit& d) {
    (void)hipFree(d.x); (void)hipFree(d.y); (void)hipFree(d.csr_indptr);
    (void)hipFree(d.csr_indices); (void)hipFree(d.csr_data); (void)hipFree(d.w); (void)hipFree(d.labfix);
    (void)hipFree(d.idx_rows); (void)hipFree(d.idx_items);
    (void)hipFree(d.idx_heavy); d.idx_heavy = nullptr;
    (void)hipFree(d.idx_bundles); d.idx_bundles = nullptr;
    (void)hipFree(d.idx_uwords); (void)hipFree(d.idx_slots); (void)hipFree(d.idx_rows_div);
    (void)hipFree(d.idx_touched_bits);
    (void)hipFree(d.idx_dense_counts); (void)hipFree(d.idx_dense_words); (void)hipFree(d.idx_tok_slot);
    d.idx_uwords = nullptr; d.idx_slots = nullptr; d.idx_rows_div = nullptr;
    d = DataSplit();
}

int sert_destroy(sert_model* m) {
    if (!m) return 0;
    (void)hipSetDevice(m->cfg.device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->stream2) (void)hipStreamSynchronize(m->stream2);   // (work that ran ahead of the host)
    if (m->stream3) (void)hipStreamSynchronize(m->stream3);
    if (m->comm_stream) (void)hipStreamSynchronize(m->comm_stream);
    if (m->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(m->comm);
    if (m->ev_rest_ready) (void)hipEventDestroy(m->ev_rest_ready);
    if (m->ev_ar_done) (void)hipEventDestroy(m->ev_ar_done);
    if (m->ev_ag_done) (void)hipEventDestroy(m->ev_ag_done);
    for (int i = 0; i < 4; ++i) {
        if (m->ev_grad_ready[i]) (void)hipEventDestroy(m->ev_grad_ready[i]);
        for (int c = 0; c < sert_model::kMaxArChunks; ++c) {
            if (m->ev_rs_done[i][c]) (void)hipEventDestroy(m->ev_rs_done[i][c]);
            if (m->ev_opt_done[i][c]) (void)hipEventDestroy(m->ev_opt_done[i][c]);
        }
    }
    (void)hipFree(m->sq_scratch);
    (void)hipFree(m->tail_blk);
    (void)hipFree(m->rw_last[0]); (void)hipFree(m->rw_last[1]); (void)hipFree(m->rw_pred);
    xr_free_lists(m);
    if (m->ev_params_ready) (void)hipEventDestroy(m->ev_params_ready);
    if (m->ev_word_updated) (void)hipEventDestroy(m->ev_word_updated);
    if (m->comm_stream) (void)hipStreamDestroy(m->comm_stream);
    float* bufs[] = {m->rw, m->re, m->W, m->b, m->s0_rw, m->s0_re, m->s0_w, m->s0_b, m->s1_rw,
                     m->s1_re, m->s1_w, m->s1_b, m->gflat, m->H, m->T, m->T_alt, m->DA, m->DH, m->rowloss,
                     m->G, m->Z, m->J, m->DG, m->DH2, m->part, m->skbuf.p, m->wpart, m->hpart, m->red_loss, m->red_sq, m->re_sq, m->d_loss,
                     m->d_losses};
    for (float* p : bufs) (void)hipFree(p);
    (void)hipFree(m->ll_tokstat); (void)hipFree(m->ll_lse); (void)hipFree(m->ll_jstat);
    (void)hipFree(m->ll_rowinfo); (void)hipFree(m->ll_rpart); (void)hipFree(m->ll_r); (void)hipFree(m->ll_rsum);
    (void)hipFree(m->Zu); (void)hipFree(m->dZu); (void)hipFree(m->zpart);
    (void)hipFree(m->neg); (void)hipFree(m->neg_alt); (void)hipFree(m->neg_stage);
    (void)hipFree(m->pred_a); (void)hipFree(m->pred_b); (void)hipFree(m->pred_ids);
    (void)hipFree(m->cand); (void)hipFree(m->cand_sorted); (void)hipFree(m->cand_early);
    (void)hipFree(m->pair_sorted); (void)hipFree(m->coef); (void)hipFree(m->ehead);
    (void)hipFree(m->etail); (void)hipFree(m->epart); (void)hipFree(m->eg_entries); (void)hipFree(m->eg_offs); (void)hipFree(m->sort_hist); (void)hipFree(m->sort_bin_total);
    (void)hipFree(m->sort_k_tmp); (void)hipFree(m->sort_v_tmp);
    if (m->h_loss) (void)hipHostFree(m->h_loss);
    if (m->host_send) (void)hipHostFree(m->host_send);
    if (m->host_recv) (void)hipHostFree(m->host_recv);
    free_split(m->split[0]); free_split(m->split[1]);
    if (m->timing.created)
        for (int g = 0; g < TG_COUNT; ++g)
            for (int k = 0; k < 2; ++k) (void)hipEventDestroy(m->timing.ev[g][k]);
    if (m->instep.created)
        for (int i = 0; i < InStep::kRing; ++i)
            for (int k = 0; k < 2; ++k) (void)hipEventDestroy(m->instep.ev[i][k]);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->stream2) (void)hipStreamDestroy(m->stream2);
    if (m->ev_join3) (void)hipEventDestroy(m->ev_join3);
    for (hipEvent_t e : {m->ev_step_done, m->ev_neg, m->ev_opt_fork, m->ev_small, m->ev_re, m->ev_dense, m->ev_loss})
        if (e) (void)hipEventDestroy(e);
    if (m->stream3) (void)hipStreamDestroy(m->stream3);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return 0;
}

size_t sert_tensor_size(sert_model* m, int which) {
    if (!m) return 0;
    return tensor_ref(m, which).count;
}

int sert_set_tensor(sert_model* m, int which, const float* host, size_t count) {
    if (m) invalidate_speculation(m);
    if (!m || !host) SERT_FAIL("null argument");
    SERT_HIP(hipSetDevice(m->cfg.device));
    TensorRef t = tensor_ref(m, which);
    if (!t.ptr || t.count == 0) SERT_FAIL("tensor not present for this model kind");
    if (t.count != count) SERT_FAIL("element count mismatch");
    if (which >= SERT_T_STATE0_RW && which <= SERT_T_STATE1_B && m->pt_sharded[(which - SERT_T_STATE0_RW) % 4])
        return sharded_state_io(m, (which - SERT_T_STATE0_RW) % 4, (which - SERT_T_STATE0_RW) / 4, nullptr, host);
    if (m->comm_stream) SERT_HIP(hipStreamSynchronize(m->comm_stream));
    SERT_TRY(settle_entity_update(m));
    m->re_sq_for[0] = m->re_sq_for[1] = -1;
    SERT_HIP(hipMemcpyAsync(t.ptr, host, count * sizeof(float), hipMemcpyHostToDevice, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    if (which == SERT_T_RW) { m->rw_full = true; m->xr_fetched_batch = -1; }   // (every rank sets the whole table)
    return 0;
}

int sert_get_tensor(sert_model* m, int which, float* host, size_t count) {
    if (!m || !host) SERT_FAIL("null argument");
    SERT_HIP(hipSetDevice(m->cfg.device));
    TensorRef t = tensor_ref(m, which);
    if (!t.ptr || t.count == 0) SERT_FAIL("tensor not present for this model kind");
    if (t.count != count) SERT_FAIL("element count mismatch");
    // Without keep_grads the gradient buffers are scratch: the word table is neither zeroed
    // nor fully written, the L2 term is never stored, and the activation buffers may already
    // hold the NEXT batch (sert_hint_next_batch).  Refuse instead of returning something stale.
    if (which >= SERT_T_GRAD_RW && which <= SERT_T_ACT_ROWLOSS && !m->cfg.keep_grads)
        SERT_FAIL("gradients and activations are only readable from a model created with keep_grads = 1");
    if (which >= SERT_T_STATE0_RW && which <= SERT_T_STATE1_B && m->pt_sharded[(which - SERT_T_STATE0_RW) % 4])
        return sharded_state_io(m, (which - SERT_T_STATE0_RW) % 4, (which - SERT_T_STATE0_RW) / 4, host, nullptr);
    if (which == SERT_T_RW) SERT_TRY(ensure_full_rw(m));   // (owned by rows: collective while stale)
    SERT_TRY(ensure_rw_current(m, -1));                     // (lazy word-table update: flush before anyone looks)
    if (m->comm_stream) SERT_HIP(hipStreamSynchronize(m->comm_stream));
    if (m->stream2) SERT_HIP(hipStreamSynchronize(m->stream2));
    SERT_HIP(hipMemcpyAsync(host, t.ptr, count * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    return 0;
}

int sert_set_step(sert_model* m, int64_t t) {
    if (!m || t < 0) SERT_FAIL("bad argument");
    invalidate_speculation(m);     // (first: a lazy word table is flushed at the OLD step count)
    m->step = t;
    return 0;
}
int64_t sert_get_step(sert_model* m) { return m ? m->step : -1; }

int sert_set_eval_draws(sert_model* m, int64_t n) {
    if (!m || n < 0) SERT_FAIL("bad argument");
    m->eval_draws = n;
    return 0;
}
int64_t sert_get_eval_draws(sert_model* m) { return m ? m->eval_draws : -1; }

int sert_negatives_of_step(sert_model* m, int64_t position, int evaluation, int64_t* out) {
    if (!m || !out || position < 0) SERT_FAIL("bad argument");
    if (!is_vs(m) || is_fs(m) || m->cfg.num_negatives <= 0) SERT_FAIL("this model draws no negatives");
    SERT_HIP(hipSetDevice(m->cfg.device));
    const int64_t count = (int64_t)m->cfg.batch_size * m->cfg.num_negatives;
    int32_t* tmp = nullptr;
    SERT_HIP(hipMalloc((void**)&tmp, (size_t)count * sizeof(int32_t)));
    // a stream of its own: nothing of the model's state or schedule is touched
    hipStream_t st = nullptr;
    if (hipStreamCreate(&st) != hipSuccess) { (void)hipFree(tmp); SERT_FAIL("hipStreamCreate failed"); }
    launch(vs_sample_negatives, dim3(grid_for((count + 3) / 4)), dim3(256), 0, st, tmp, count,
           (int64_t)m->rank * count, (uint32_t)m->cfg.num_entities, m->cfg.seed,
           (uint64_t)position * 2 + (evaluation ? 1 : 0), (float4*)nullptr, (size_t)0, (uint4*)nullptr, (size_t)0);
    std::vector<int32_t> host((size_t)count);
    const hipError_t e = hipMemcpyAsync(host.data(), tmp, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    (void)hipFree(tmp);
    if (e != hipSuccess || e2 != hipSuccess) SERT_FAIL("reading the negatives back failed");
    for (int64_t i = 0; i < count; ++i) out[i] = host[(size_t)i];
    return 0;
}
