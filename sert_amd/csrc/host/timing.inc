// Part of sert_hip.hip (one translation unit; included there, inside its namespace / extern "C" block): the timing groups of a step, their roctx ranges, and the in-step event ring behind launch() (launch.h).

static const char* kTimingNames[TG_COUNT] = {
    "gather",        "gemm_fwd", "loss",      "entity_sort",          "entity_grad_reduce",
    "entity_grad_fixup", "gemm_dW", "splitk_combine", "gemm_dX",      "word_grad_segsum",
    "allreduce",     "reduce_scatter", "all_gather", "optimizer_word_table",  "optimizer_other",      "finalize"};

// ---- roctx ranges (SURVEY 5, 8-b: sert_profile_range_push / pop) ------------------------------------
// Loaded lazily from the ROCm tools library; SERT_ROCTX=1 additionally wraps every kernel group of a step
// (the timing groups below) in a range, so that a rocprofv3 --marker-trace shows the step's structure on
// the host timeline.  Without the library the calls are no-ops.
struct Roctx {
    bool tried = false;
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
static Roctx g_roctx;
static void roctx_load() {
    if (g_roctx.tried) return;
    g_roctx.tried = true;
    for (const char* n : {"libroctx64.so.4", "libroctx64.so", "librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/libroctx64.so"}) {
        void* lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) continue;
        g_roctx.push = (decltype(g_roctx.push))dlsym(lib, "roctxRangePushA");
        g_roctx.pop = (decltype(g_roctx.pop))dlsym(lib, "roctxRangePop");
        if (g_roctx.push && g_roctx.pop) return;
        g_roctx.push = nullptr; g_roctx.pop = nullptr;
    }
}
static bool roctx_groups() {
    static const bool on = [] {
        const bool want = knob("SERT_ROCTX") && atoi(knob("SERT_ROCTX")) != 0;
        if (want) roctx_load();
        return want && g_roctx.push != nullptr;
    }();
    return on;
}

// ---- in-step mode (sert_timing_enable(m, 2)) -----------------------------------------------------------------------
// The NORMAL schedule (all streams, run-ahead), with every plain launch inside a timing group bound to a (start, stop)
// event pair of its own: what a kernel takes IN THE STEP, beside whatever the other queue runs (mode 1 times every group
// alone on one queue).  launch() asks the hook below for the pair; the pairs in flight sit in a ring (model.h: InStep)
// that is harvested when it is full.  Launches that carry a completion event of the schedule keep it and are not timed.
static void instep_harvest(sert_model* m, bool all) {
    InStep& t = m->instep;
    while (t.head < t.tail && (all || t.tail - t.head >= InStep::kRing)) {
        const int i = (int)(t.head % InStep::kRing);
        float ms = 0.f;
        if (hipEventSynchronize(t.ev[i][1]) == hipSuccess && hipEventElapsedTime(&ms, t.ev[i][0], t.ev[i][1]) == hipSuccess) {
            t.total_us[t.group[i]] += 1000.0 * ms;
            t.launches[t.group[i]] += 1;
        }
        ++t.head;
    }
}
static bool instep_take(void* ctx, hipEvent_t* a, hipEvent_t* b) {
    sert_model* m = (sert_model*)ctx;
    InStep& t = m->instep;
    if (!t.on || t.cur_group < 0) return false;
    instep_harvest(m, false);
    const int i = (int)(t.tail % InStep::kRing);
    t.group[i] = t.cur_group;
    *a = t.ev[i][0];
    *b = t.ev[i][1];
    ++t.tail;
    return true;
}
// (the launch of the pair taken last failed: the slot's events are those of its previous lap, not a sample)
static void instep_give_back(void* ctx) { --((sert_model*)ctx)->instep.tail; }

struct ScopedTimer {
    sert_model* m;
    int g;
    hipStream_t s;
    int instep_prev = -1;
    InStepHook hook_prev = {nullptr, nullptr, nullptr};
    ScopedTimer(sert_model* m_, int g_, hipStream_t s_ = nullptr) : m(m_), g(g_), s(s_ ? s_ : m_->stream) {
        if (m->instep.on) {
            instep_prev = m->instep.cur_group;
            hook_prev = instep_hook();
            m->instep.cur_group = g;
            instep_hook() = InStepHook{instep_take, instep_give_back, m};
        }
        if (roctx_groups()) (void)g_roctx.push(kTimingNames[g]);
        // a group bracketed several times in one step spans first start .. last end
        if (m->timing.enabled && !m->timing.used[g]) {
            (void)hipEventRecord(m->timing.ev[g][0], s);
        }
    }
    ~ScopedTimer() {
        if (m->timing.enabled) {
            (void)hipEventRecord(m->timing.ev[g][1], s);
            m->timing.used[g] = true;
        }
        if (roctx_groups()) (void)g_roctx.pop();
        if (m->instep.on) {
            m->instep.cur_group = instep_prev;
            instep_hook() = hook_prev;
        }
    }
};

static void timing_collect(sert_model* m) {
    if (!m->timing.enabled) return;
    for (int g = 0; g < TG_COUNT; ++g) {
        if (!m->timing.used[g]) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->timing.ev[g][0], m->timing.ev[g][1]) == hipSuccess) {
            m->timing.total_us[g] += 1000.0 * ms;
            m->timing.samples[g] += 1;
        }
        m->timing.used[g] = false;
    }
}
