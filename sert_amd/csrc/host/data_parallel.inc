// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): the data-parallel exchange: host transport, RCCL calls, the word table exchanged by rows, reduce-scatter / all-reduce of the rest.

// ---- data-parallel exchange (new: the reference is single-device, SURVEY 2.2 / 8-e) ---------
// ZeRO-1 over the big tensors (model.h): reduce-scatter of a gradient slab -> the optimiser on
// the owned piece (1/world of the launch, 1/world of the state) -> all-gather of the parameter
// slab; the small tensors' gradients, the loss sum and the owned pieces' sum of squares travel
// in ONE all-reduce and the small tensors are updated identically on every rank.  Every
// collective is issued on comm_stream, in the same order on every rank:
//   RS(R_w) as soon as the segmented reduction has produced dR_w (it overlaps the rest of the
//   backward), RS(other big tensors), AR(rest), then AG(R_w), AG(others) behind the optimiser.
static inline bool is_dp(const sert_model* m) { return m->comm != nullptr || m->host_ar != nullptr; }

struct ParamTensor {
    float *p, *g, *s0, *s1;
    size_t n;
    bool l2;
};
static ParamTensor param_tensor(sert_model* m, int i) {
    switch (i) {
        case 0: return {m->rw, m->g_rw, m->s0_rw, m->s1_rw, m->n_rw, true};
        case 1: return {m->re, m->g_re, m->s0_re, m->s1_re, m->n_re, true};
        case 2: return {m->W, m->g_w, m->s0_w, m->s1_w, m->n_w, true};
        default: return {m->b, m->g_b, m->s0_b, m->s1_b, m->n_b, false};   // bias: not regularised
    }
}
static inline size_t slab_elems(const sert_model* m, int i) { return m->pt_sc[i] * (size_t)m->world; }
static inline size_t piece_off(const sert_model* m, int i, int c) {
    return (size_t)c * slab_elems(m, i) + (size_t)m->rank * m->pt_sc[i];
}

// ---- host-mediated transport: every collective through ONE all-to-all callback ------------------
static int host_reserve(sert_model* m, size_t send_floats, size_t recv_floats) {
    if (m->host_send_cap < send_floats) {
        if (m->host_send) (void)hipHostFree(m->host_send);
        m->host_send = nullptr; m->host_send_cap = 0;
        SERT_HIP(hipHostMalloc((void**)&m->host_send, std::max<size_t>(send_floats, 64) * sizeof(float), hipHostMallocDefault));
        m->host_send_cap = std::max<size_t>(send_floats, 64);
    }
    if (m->host_recv_cap < recv_floats) {
        if (m->host_recv) (void)hipHostFree(m->host_recv);
        m->host_recv = nullptr; m->host_recv_cap = 0;
        SERT_HIP(hipHostMalloc((void**)&m->host_recv, std::max<size_t>(recv_floats, 64) * sizeof(float), hipHostMallocDefault));
        m->host_recv_cap = std::max<size_t>(recv_floats, 64);
    }
    return 0;
}
static int host_call(sert_model* m, const std::vector<int64_t>& soff, const std::vector<int64_t>& scnt,
                     const std::vector<int64_t>& roff, const std::vector<int64_t>& rcnt) {
    if (m->host_ar(m->host_ar_user, m->host_send, soff.data(), scnt.data(), m->host_recv, roff.data(), rcnt.data()) != 0)
        SERT_FAIL("host all-to-all callback failed");
    for (int q = 0; q < m->world; ++q)
        if (q != m->rank) m->comm_bytes_moved += 4.0 * (double)(scnt[(size_t)q] + rcnt[(size_t)q]);
    return 0;
}
// In-place SUM of dev[0, count) over the ranks (every rank sends the whole buffer to every rank and
// adds the copies in rank order: identical bits everywhere).  For the small replicated remainder.
static int host_allreduce(sert_model* m, float* dev, size_t count, hipStream_t st) {
    if (count == 0) return 0;
    const size_t W = (size_t)m->world;
    SERT_TRY(host_reserve(m, count, count * W));
    SERT_HIP(hipMemcpyAsync(m->host_send, dev, count * sizeof(float), hipMemcpyDeviceToHost, st));
    SERT_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> soff(W, 0), scnt(W, (int64_t)count), roff(W), rcnt(W, (int64_t)count);
    for (size_t q = 0; q < W; ++q) roff[q] = (int64_t)(q * count);
    SERT_TRY(host_call(m, soff, scnt, roff, rcnt));
    float* acc = m->host_send;
    for (size_t k = 0; k < count; ++k) acc[k] = m->host_recv[k];
    for (size_t q = 1; q < W; ++q) {
        const float* src = m->host_recv + q * count;
        for (size_t k = 0; k < count; ++k) acc[k] += src[k];
    }
    SERT_HIP(hipMemcpyAsync(dev, acc, count * sizeof(float), hipMemcpyHostToDevice, st));
    SERT_HIP(hipStreamSynchronize(st));
    return 0;
}
// Reduce-scatter of one slab (world pieces of sc floats at `slab`): piece q goes to rank q, this rank
// adds the world copies of ITS piece in rank order and stores the sum over its piece -- only there.
static int host_reduce_scatter(sert_model* m, float* slab, size_t sc, hipStream_t st) {
    const size_t W = (size_t)m->world;
    SERT_TRY(host_reserve(m, sc * W, sc * W));
    SERT_HIP(hipMemcpyAsync(m->host_send, slab, sc * W * sizeof(float), hipMemcpyDeviceToHost, st));
    SERT_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> soff(W), scnt(W, (int64_t)sc), roff(W), rcnt(W, (int64_t)sc);
    for (size_t q = 0; q < W; ++q) { soff[q] = (int64_t)(q * sc); roff[q] = (int64_t)(q * sc); }
    SERT_TRY(host_call(m, soff, scnt, roff, rcnt));
    float* acc = m->host_send;
    for (size_t k = 0; k < sc; ++k) acc[k] = m->host_recv[k];
    for (size_t q = 1; q < W; ++q) {
        const float* src = m->host_recv + q * sc;
        for (size_t k = 0; k < sc; ++k) acc[k] += src[k];
    }
    SERT_HIP(hipMemcpyAsync(slab + (size_t)m->rank * sc, acc, sc * sizeof(float), hipMemcpyHostToDevice, st));
    SERT_HIP(hipStreamSynchronize(st));
    return 0;
}
// All-gather of one slab: this rank's piece goes to everyone, piece q arrives from rank q.
static int host_allgather(sert_model* m, float* slab, size_t sc, hipStream_t st) {
    const size_t W = (size_t)m->world;
    SERT_TRY(host_reserve(m, sc, sc * W));
    SERT_HIP(hipMemcpyAsync(m->host_send, slab + (size_t)m->rank * sc, sc * sizeof(float), hipMemcpyDeviceToHost, st));
    SERT_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> soff(W, 0), scnt(W, (int64_t)sc), roff(W), rcnt(W, (int64_t)sc);
    for (size_t q = 0; q < W; ++q) roff[q] = (int64_t)(q * sc);
    SERT_TRY(host_call(m, soff, scnt, roff, rcnt));
    SERT_HIP(hipMemcpyAsync(slab, m->host_recv, sc * W * sizeof(float), hipMemcpyHostToDevice, st));
    SERT_HIP(hipStreamSynchronize(st));
    return 0;
}
// All-to-all of float segments between device buffers (offsets / counts in floats, peers only).
static int host_alltoallv(sert_model* m, const float* dsend, size_t stotal, const std::vector<int64_t>& soff,
                          const std::vector<int64_t>& scnt, float* drecv, size_t rtotal, const std::vector<int64_t>& roff,
                          const std::vector<int64_t>& rcnt, hipStream_t st) {
    SERT_TRY(host_reserve(m, stotal, rtotal));
    if (stotal) SERT_HIP(hipMemcpyAsync(m->host_send, dsend, stotal * sizeof(float), hipMemcpyDeviceToHost, st));
    SERT_HIP(hipStreamSynchronize(st));
    SERT_TRY(host_call(m, soff, scnt, roff, rcnt));
    if (rtotal) SERT_HIP(hipMemcpyAsync(drecv, m->host_recv, rtotal * sizeof(float), hipMemcpyHostToDevice, st));
    SERT_HIP(hipStreamSynchronize(st));
    return 0;
}
static int rccl_alltoallv(sert_model* m, const float* dsend, const std::vector<int64_t>& soff, const std::vector<int64_t>& scnt,
                          float* drecv, const std::vector<int64_t>& roff, const std::vector<int64_t>& rcnt, hipStream_t st) {
    SERT_NCCL(g_rccl.GroupStart());
    // a failing Send / Recv must not leave the group open (every later collective of this communicator would be
    // queued into the dangling group and hang): remember the first error, always close the group, then fail
    int first = 0;
    const char* what = "";
    for (int q = 0; q < m->world && first == 0; ++q) {
        if (q == m->rank) continue;
        if (scnt[(size_t)q]) {
            first = g_rccl.Send(dsend + soff[(size_t)q], (size_t)scnt[(size_t)q], /*ncclFloat32*/ 7, q, m->comm, st);
            if (first) { what = "ncclSend"; break; }
        }
        if (rcnt[(size_t)q]) {
            first = g_rccl.Recv(drecv + roff[(size_t)q], (size_t)rcnt[(size_t)q], 7, q, m->comm, st);
            if (first) { what = "ncclRecv"; break; }
        }
        m->comm_bytes_moved += 4.0 * (double)(scnt[(size_t)q] + rcnt[(size_t)q]);
    }
    const int end = g_rccl.GroupEnd();
    if (first != 0 || end != 0) {
        m->comm_dead = true;      // (peers may be blocked in a half-issued all-to-all: nothing sane can follow)
        SERT_FAIL(std::string(first ? what : "ncclGroupEnd") + " failed in the row all-to-all: " +
                  (g_rccl.GetErrorString ? g_rccl.GetErrorString(first ? first : end) : "rccl error"));
    }
    return 0;
}

// ---- the word table exchanged by rows (kernels_xchg.h) -------------------------------------------
static inline bool xr_async(const sert_model* m) { return m->comm && !m->timing.enabled; }

// One all-to-all of rows: `send_cnt[q]` rows to rank q out of xr_send (peer-major), `recv_cnt[q]` rows
// from rank q into xr_recv (peer-major), d_w floats each.
static int xr_alltoall(sert_model* m, const std::vector<int32_t>& send_cnt, const std::vector<int32_t>& recv_cnt, hipStream_t st) {
    const size_t W = (size_t)m->world;
    const int64_t d = m->cfg.word_dim;
    std::vector<int64_t> soff(W), scnt(W), roff(W), rcnt(W);
    int64_t so = 0, ro = 0;
    for (size_t q = 0; q < W; ++q) {
        soff[q] = so; scnt[q] = (int64_t)send_cnt[q] * d; so += scnt[q];
        roff[q] = ro; rcnt[q] = (int64_t)recv_cnt[q] * d; ro += rcnt[q];
    }
    if (m->host_ar) return host_alltoallv(m, m->xr_send, (size_t)so, soff, scnt, m->xr_recv, (size_t)ro, roff, rcnt, st);
    return rccl_alltoallv(m, m->xr_send, soff, scnt, m->xr_recv, roff, rcnt, st);
}

// PARAMETERS of the rows batch `b` touches: the owners pack and send them, this rank scatters what
// it receives into its copy of R_w.  Runs on the communication stream behind the word table's update.
static int xr_fetch_params(sert_model* m, int64_t b) {
    if (!m->xr_on || m->rw_full || m->xr_fetched_batch == b) return 0;
    if ((size_t)b >= m->xr->batches.size()) SERT_FAIL("batch has no row-exchange lists");
    const RowExchangeBatch& xb = m->xr->batches[(size_t)b];
    const int d4 = m->cfg.word_dim / 4;
    const bool async = xr_async(m);
    hipStream_t st = async ? m->comm_stream : m->stream;
    ScopedTimer tm(m, TG_ALLGATHER);
    if (async) SERT_HIP(hipStreamWaitEvent(st, m->ev_word_updated, 0));   // (the owners' rows are final)
    if (xb.serve_total)
        launch(xchg_pack_rows, dim3(grid_for((int64_t)xb.serve_total * d4)), dim3(256), 0, st, (const float*)m->rw,
               (const int32_t*)m->xr_serve + xb.serve_off, xb.serve_total, d4, reinterpret_cast<float4*>(m->xr_send));
    SERT_TRY(xr_alltoall(m, xb.serve_cnt, xb.fetch_cnt, st));
    if (xb.fetch_total)
        launch(xchg_unpack_rows, dim3(grid_for((int64_t)xb.fetch_total * d4)), dim3(256), 0, st, m->rw,
               (const int32_t*)m->xr_fetch + xb.fetch_off, xb.fetch_total, d4, reinterpret_cast<const float4*>(m->xr_recv));
    if (async) {
        SERT_HIP(hipEventRecord(m->ev_params_ready, st));
        SERT_HIP(hipStreamWaitEvent(m->stream, m->ev_params_ready, 0));
    }
    m->xr_fetched_batch = b;
    return 0;
}

// GRADIENT rows of batch `b`: packed from this rank's dR_w, sent to their owners; the rows received
// are added to this rank's own in rank order into dR_w[owned rows].
static int xr_return_grads(sert_model* m, int64_t b) {
    const RowExchangeBatch& xb = m->xr->batches[(size_t)b];
    const int d4 = m->cfg.word_dim / 4;
    const bool async = xr_async(m);
    hipStream_t st = async ? m->comm_stream : m->stream;
    ScopedTimer tm(m, TG_REDUCE_SCATTER);
    if (async) {
        SERT_HIP(hipEventRecord(m->ev_grad_ready[0], m->stream));
        SERT_HIP(hipStreamWaitEvent(st, m->ev_grad_ready[0], 0));
    }
    if (xb.fetch_total)
        launch(xchg_pack_rows, dim3(grid_for((int64_t)xb.fetch_total * d4)), dim3(256), 0, st, (const float*)m->g_rw,
               (const int32_t*)m->xr_fetch + xb.fetch_off, xb.fetch_total, d4, reinterpret_cast<float4*>(m->xr_send));
    SERT_TRY(xr_alltoall(m, xb.fetch_cnt, xb.serve_cnt, st));
    if (xb.nunion)
        launch(xchg_reduce_rows, dim3(grid_for((int64_t)xb.nunion * d4)), dim3(256), 0, st,
               reinterpret_cast<const float4*>(m->xr_recv), (const int32_t*)m->xr_ptr + xb.ptr_off,
               (const int32_t*)m->xr_ent + xb.ent_off, (const int32_t*)m->xr_union + xb.union_off, xb.nunion, d4, m->g_rw);
    if (async) {
        SERT_HIP(hipEventRecord(m->ev_rs_done[0][0], st));
        m->rs_issued[0] = true;
    }
    return 0;
}

static void xr_free_lists(sert_model* m) {
    m->xr_on = false;
    (void)hipFree(m->xr_serve); (void)hipFree(m->xr_fetch); (void)hipFree(m->xr_union); (void)hipFree(m->xr_ent);
    (void)hipFree(m->xr_ptr); (void)hipFree(m->xr_ubits); (void)hipFree(m->xr_send); (void)hipFree(m->xr_recv);
    m->xr_serve = m->xr_fetch = m->xr_union = m->xr_ent = m->xr_ptr = nullptr;
    m->xr_ubits = nullptr; m->xr_send = m->xr_recv = nullptr;
    delete m->xr;
    m->xr = nullptr;
}

// The exchange lists of a freshly uploaded training split: every rank's per-batch touched bitmaps are
// all-gathered (in groups of batches: at most 64 MB of bitmaps at a time), the lists derived from
// them on the host (kernels_xchg.h) and uploaded.  COLLECTIVE: every rank uploads its split.
static int xr_build_lists(sert_model* m, const std::vector<uint32_t>& bits, int64_t nb, int64_t bit_words) {
    xr_free_lists(m);
    if (!m->xr_mode || !m->pt_sharded[0]) return 0;      // (rank-invariant: every rank leaves here or none does)
    const size_t W = (size_t)m->world;
    hipStream_t s = m->stream;
    {
        // This function is collective, `nb` is a per-rank quantity: agree on it BEFORE anything can return early
        // (a rank whose shard held no complete batch used to skip the bitmap all-gather its peers blocked in).
        // Three exact small integers per rank as floats: nb (< 2^48 split in two) and the bitmap width.
        std::vector<float> mine = {(float)(nb & 0xffffff), (float)(nb >> 24), (float)bit_words}, all3(3 * W, 0.f);
        if (m->host_ar) {
            SERT_TRY(host_reserve(m, 3, 3 * W));
            memcpy(m->host_send, mine.data(), 3 * sizeof(float));
            std::vector<int64_t> soff(W, 0), scnt(W, 3), roff(W), rcnt(W, 3);
            for (size_t q = 0; q < W; ++q) roff[q] = (int64_t)(3 * q);
            const double moved = m->comm_bytes_moved;
            SERT_TRY(host_call(m, soff, scnt, roff, rcnt));
            m->comm_bytes_moved = moved;
            memcpy(all3.data(), m->host_recv, 3 * W * sizeof(float));
        } else {
            float *src = nullptr, *dst = nullptr;
            SERT_TRY(dmalloc(&src, 3));
            if (dmalloc(&dst, 3 * W) != 0) { (void)hipFree(src); return -1; }
            hipError_t he = hipMemcpyAsync(src, mine.data(), 3 * sizeof(float), hipMemcpyHostToDevice, s);
            const int rc = he == hipSuccess ? g_rccl.AllGather(src, dst, 3, /*ncclFloat32*/ 7, m->comm, s) : 0;
            if (he == hipSuccess) he = hipMemcpyAsync(all3.data(), dst, 3 * W * sizeof(float), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipStreamSynchronize(s);
            (void)hipFree(src); (void)hipFree(dst);
            if (rc != 0) SERT_FAIL("ncclAllGather of the batch counts failed");
            SERT_HIP(he);
        }
        for (size_t q = 0; q < W; ++q) {
            const int64_t nbq = (int64_t)all3[3 * q] + ((int64_t)all3[3 * q + 1] << 24);
            if (nbq != nb || (nb > 0 && (int64_t)all3[3 * q + 2] != bit_words))
                SERT_FAIL("data parallel: rank " + std::to_string(q) + " uploaded " + std::to_string(nbq) + " complete batches, rank " +
                          std::to_string(m->rank) + " " + std::to_string(nb) + " -- every rank must upload the same number of rows "
                          "(sert_amd.distributed.shard_rows)");      // (raised on EVERY rank: they all see the same table)
        }
    }
    if (nb == 0) return 0;
    m->xr = new RowExchangeLists();
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(nb, ((int64_t)64 << 20) / (bit_words * 4 * (int64_t)W)));
    std::vector<uint32_t> all;
    for (int64_t b0 = 0; b0 < nb; b0 += group) {
        const int64_t gb = std::min(group, nb - b0);
        const size_t cnt = (size_t)(gb * bit_words);
        all.resize(W * cnt);
        const uint32_t* mine = bits.data() + (size_t)(b0 * bit_words);
        if (m->host_ar) {
            SERT_TRY(host_reserve(m, cnt, cnt * W));
            memcpy(m->host_send, mine, cnt * 4);
            std::vector<int64_t> soff(W, 0), scnt(W, (int64_t)cnt), roff(W), rcnt(W, (int64_t)cnt);
            for (size_t q = 0; q < W; ++q) roff[q] = (int64_t)(q * cnt);
            const double moved = m->comm_bytes_moved;
            SERT_TRY(host_call(m, soff, scnt, roff, rcnt));
            m->comm_bytes_moved = moved;   // (set-up traffic is not part of a step)
            memcpy(all.data(), m->host_recv, W * cnt * 4);
        } else {
            float *src = nullptr, *dst = nullptr;
            SERT_TRY(dmalloc(&src, cnt));
            if (dmalloc(&dst, cnt * W) != 0) { (void)hipFree(src); return -1; }
            hipError_t he = hipMemcpyAsync(src, mine, cnt * 4, hipMemcpyHostToDevice, s);
            const int rc = he == hipSuccess ? g_rccl.AllGather(src, dst, cnt, /*ncclFloat32: bits only*/ 7, m->comm, s) : 0;
            if (he == hipSuccess) he = hipMemcpyAsync(all.data(), dst, W * cnt * 4, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipStreamSynchronize(s);
            (void)hipFree(src); (void)hipFree(dst);
            if (rc != 0) SERT_FAIL("ncclAllGather of the touched-row bitmaps failed");
            SERT_HIP(he);
        }
        build_row_exchange(all.data(), m->world, m->rank, gb, bit_words, m->xr_rows_per_rank, m->cfg.vocab_size, *m->xr);
    }
    const RowExchangeLists& L = *m->xr;
    auto up = [&](int32_t** d, const std::vector<int32_t>& h) -> int {
        SERT_TRY(dmalloc(d, std::max<size_t>(1, h.size())));
        if (!h.empty()) SERT_HIP(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        return 0;
    };
    SERT_TRY(up(&m->xr_serve, L.serve_rows)); SERT_TRY(up(&m->xr_fetch, L.fetch_rows));
    SERT_TRY(up(&m->xr_union, L.union_rows)); SERT_TRY(up(&m->xr_ent, L.ent)); SERT_TRY(up(&m->xr_ptr, L.ptr));
    SERT_TRY(dmalloc(&m->xr_ubits, std::max<size_t>(1, L.union_bits.size())));
    if (!L.union_bits.empty())
        SERT_HIP(hipMemcpyAsync(m->xr_ubits, L.union_bits.data(), L.union_bits.size() * 4, hipMemcpyHostToDevice, s));
    const size_t buf = (size_t)std::max<int32_t>(1, L.max_xfer_rows) * (size_t)m->cfg.word_dim;
    SERT_TRY(dmalloc(&m->xr_send, buf));
    SERT_TRY(dmalloc(&m->xr_recv, buf));
    SERT_HIP(hipStreamSynchronize(s));
    m->xr_on = true;
    return 0;
}

// Make every row of R_w on this rank current (all-gather of the owned slabs).  COLLECTIVE.
static int ensure_full_rw(sert_model* m) {
    if (m->rw_full || !m->pt_sharded[0] || !is_dp(m)) { m->rw_full = true; return 0; }
    if (m->comm_dead) SERT_FAIL("the communicator of this data-parallel model was destroyed");
    const size_t sc = m->pt_sc[0], slab = sc * (size_t)m->world;
    if (m->comm_stream) SERT_HIP(hipStreamSynchronize(m->comm_stream));
    SERT_HIP(hipStreamSynchronize(m->stream));
    for (int c = 0; c < m->ar_chunks; ++c) {
        if (m->host_ar) SERT_TRY(host_allgather(m, m->rw + (size_t)c * slab, sc, m->stream));
        else SERT_NCCL(g_rccl.AllGather(m->rw + (size_t)c * slab + (size_t)m->rank * sc, m->rw + (size_t)c * slab, sc, 7, m->comm, m->stream));
    }
    SERT_HIP(hipStreamSynchronize(m->stream));
    m->rw_full = true;
    m->xr_fetched_batch = -1;
    return 0;
}

// Reduce-scatter of big tensor i's gradient (complete on the main stream at this point).
static int exchange_grad(sert_model* m, int i) {
    if (!is_dp(m) || !m->pt_sharded[i]) return 0;
    if (m->comm_dead) SERT_FAIL("the communicator of this data-parallel model was destroyed");
    const ParamTensor t = param_tensor(m, i);
    const size_t sc = m->pt_sc[i];
    m->rs_issued[i] = false;
    if (i == 0 && m->xr_on) return xr_return_grads(m, m->xr_batch);
    // verification transport: slab by slab, this rank receives and sums ITS piece only
    if (m->host_ar) {
        ScopedTimer tm(m, TG_REDUCE_SCATTER);
        for (int c = 0; c < m->ar_chunks; ++c) SERT_TRY(host_reduce_scatter(m, t.g + (size_t)c * slab_elems(m, i), sc, m->stream));
        return 0;
    }
    if (m->timing.enabled) {   // timing mode: serial, on the main stream
        ScopedTimer tm(m, TG_REDUCE_SCATTER);
        for (int c = 0; c < m->ar_chunks; ++c)
            SERT_NCCL(g_rccl.ReduceScatter(t.g + (size_t)c * slab_elems(m, i), t.g + piece_off(m, i, c), sc,
                                           /*ncclFloat32*/ 7, /*ncclSum*/ 0, m->comm, m->stream));
        return 0;
    }
    SERT_HIP(hipEventRecord(m->ev_grad_ready[i], m->stream));
    SERT_HIP(hipStreamWaitEvent(m->comm_stream, m->ev_grad_ready[i], 0));
    m->comm_bytes_moved += 8.0 * (double)sc * (double)(m->world - 1) * m->ar_chunks;   // (N-1) pieces out, (N-1) in per slab
    for (int c = 0; c < m->ar_chunks; ++c) {
        SERT_NCCL(g_rccl.ReduceScatter(t.g + (size_t)c * slab_elems(m, i), t.g + piece_off(m, i, c), sc, 7, 0,
                                       m->comm, m->comm_stream));
        SERT_HIP(hipEventRecord(m->ev_rs_done[i][c], m->comm_stream));
    }
    m->rs_issued[i] = true;
    return 0;
}
static int allreduce_word_grad(sert_model* m) { return exchange_grad(m, 0); }

// The other big tensors' reduce-scatters, then the all-reduce of the replicated remainder
// [small tensors' gradients | loss sum | owned sum of squares].
static int allreduce_rest(sert_model* m) {
    if (!is_dp(m)) return 0;
    if (m->plan.dp_late_join) {
        // (every gradient of the side stream -- a sharded entity table's as well as the replicated remainder -- is
        //  complete before the communication stream touches it; the main stream meets them again behind the collectives)
        SERT_HIP(hipEventRecord(m->ev_join, m->stream2));
        SERT_HIP(hipStreamWaitEvent(m->comm_stream, m->ev_join, 0));
    }
    for (int i = 1; i < 4; ++i) SERT_TRY(exchange_grad(m, i));
    float* rest = m->gflat + m->rest_off;
    const size_t count = m->gflat_count - m->rest_off;
    if (m->host_ar) { ScopedTimer t(m, TG_ALLREDUCE); return host_allreduce(m, rest, count, m->stream); }
    m->comm_bytes_moved += 16.0 * (double)count * (double)(m->world - 1) / (double)m->world;   // ring all-reduce: 2 (N-1)/N out + in
    if (m->timing.enabled) {
        ScopedTimer t(m, TG_ALLREDUCE);
        SERT_NCCL(g_rccl.AllReduce(rest, rest, count, 7, 0, m->comm, m->stream));
        return 0;
    }
    SERT_HIP(hipEventRecord(m->ev_rest_ready, m->stream));
    SERT_HIP(hipStreamWaitEvent(m->comm_stream, m->ev_rest_ready, 0));
    SERT_NCCL(g_rccl.AllReduce(rest, rest, count, 7, 0, m->comm, m->comm_stream));
    SERT_HIP(hipEventRecord(m->ev_ar_done, m->comm_stream));
    // the main stream waits for it in optimizer_and_loss, behind the big tensors' updates
    return 0;
}

// Sum of squares of the pieces this rank owns (pre-update values: the L2 term of the loss the
// step returns, sert/models.py:773-791) into the scalar slot that rides in the all-reduce.
// Launched behind the zeroing of the gradient buffer, on the stream that did it.
static int owned_sum_of_squares(sert_model* m, hipStream_t st) {
    if (!is_dp(m)) return 0;
    int nparts = 0;
    for (int i = 0; i < 4; ++i) {
        if (!m->pt_sharded[i]) continue;
        const ParamTensor t = param_tensor(m, i);
        const size_t owned = m->pt_sc[i] * (size_t)m->ar_chunks;
        const int nb = (int)std::min<size_t>(kOptBlocks / 2, std::max<size_t>(1, owned / 1024));
        launch(sumsq_pieces, dim3(nb), dim3(256), 0, st, (const float*)t.p + (size_t)m->rank * m->pt_sc[i],
               m->pt_sc[i], slab_elems(m, i), m->ar_chunks, m->sq_scratch + 4 * kOptBlocks + nparts);
        nparts += nb;
    }
    if (nparts) launch(partials_to_scalar, dim3(1), dim3(256), 0, st, m->sq_scratch + 4 * kOptBlocks, nparts, m->g_sq);
    return 0;
}
