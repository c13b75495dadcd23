// s3d_runtime.hip — error state, device buffers and the generic C-ABI entry points.
#include "s3d_common.h"
#include <atomic>

namespace s3d {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    S3D_HIP(hipMalloc(&p, bytes));
    cap = bytes;
    return 0;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}
int workspace_overrun(const char* what, size_t run_peak, size_t measured) {
    if (run_peak <= measured) return 0;
    set_error("%s: the run pass took %zu bytes of workspace, the measuring pass found %zu (internal error: the workspace key "
              "misses something the allocations depend on)", what, run_peak, measured);
    return S3D_ERR_INTERNAL;
}
int upload(DevBuf& dst, const void* host, size_t bytes) {
    S3D_TRY(dst.reserve(bytes));
    S3D_HIP(hipMemcpy(dst.p, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

// ---- options
static std::atomic<int> g_opt[OPT_COUNT];
static std::atomic<int> g_opt_state[OPT_COUNT];          // 0: not looked at yet, 1: resolved (environment or unset), 2: set through the ABI
static std::atomic<long long> g_opt_gen{0};
long long opt_generation() { return g_opt_gen.load(std::memory_order_acquire); }
// The value a string selects, or kOptUnset when the option does not take it: CONV_IMPL "naive" -> 1, any other string -> 0;
// WINO 0 / 4 / 24; every other option 0 / 1.
static int parse_opt(int o, const char* v) {
    if (o == OPT_CONV_IMPL) return strcmp(v, "naive") == 0 ? 1 : 0;
    char* end = nullptr;
    const long n = strtol(v, &end, 10);
    if (end == v || *end) return kOptUnset;
    return (o == OPT_WINO ? n == 0 || n == 4 || n == 24 : n == 0 || n == 1) ? int(n) : kOptUnset;
}
static const char* opt_values(int o) { return o == OPT_WINO ? "0, 4 or 24" : "0 or 1"; }     // (for messages)
int opt(Opt o) {
    if (g_opt_state[o].load(std::memory_order_acquire) == 0) {
        const std::string env = std::string("S3D_") + kOptNames[o];
        const char* e = getenv(env.c_str());
        int expect = 0;
        const int v = e ? parse_opt(o, e) : kOptUnset;      // (a value the option does not take: unset)
        // (a concurrent s3d_set_option wins: its state is 2)
        if (g_opt_state[o].compare_exchange_strong(expect, -1, std::memory_order_acq_rel)) {
            g_opt[o].store(v, std::memory_order_relaxed);
            g_opt_state[o].store(1, std::memory_order_release);
        } else while (g_opt_state[o].load(std::memory_order_acquire) < 0) {}
    }
    return g_opt[o].load(std::memory_order_relaxed);
}
static int find_opt(const char* name) {
    if (!name) return -1;
    if (strncmp(name, "S3D_", 4) == 0) name += 4;
    for (int o = 0; o < OPT_COUNT; ++o) if (strcmp(name, kOptNames[o]) == 0) return o;
    return -1;
}
// the rider switch: -1 not looked at yet (the environment decides at the first query), 0 off, 1 on
static std::atomic<int> g_riders{-1};
bool riders_enabled() {
    int v = g_riders.load(std::memory_order_acquire);
    if (v < 0) {
        const char* e = getenv("S3D_RIDERS");
        int expect = -1;
        g_riders.compare_exchange_strong(expect, e && strcmp(e, "0") == 0 ? 0 : 1, std::memory_order_acq_rel);   // (a concurrent s3d_set_riders wins)
        v = g_riders.load(std::memory_order_acquire);
    }
    return v != 0;
}
int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int n = cache[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    n = 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// The argument rules of the seven step entry points.  What a known region and the multistep update bring along holds for every
// entry that takes one; what differs between entries beyond that is in StepEntry.  Everything here comes before any launch.
int check_step(const StepEntry& e, const StepReq& r) {
    const s3d_sampler_args* a = r.step;
    const char* who = e.who;
    S3D_CHECK((r.carry_flags & ~(S3D_CARRY_OUT | S3D_CARRY_IN)) == 0, S3D_ERR_INVALID, "%s: unknown flag bits %d", who, r.carry_flags);
    S3D_CHECK((r.model || a->model_out) && a->x && a->t && a->tables && a->pred_xstart, S3D_ERR_INVALID,
              "%s: %sx, t, tables and pred_xstart are required", who, r.model ? "" : "model_out, ");
    if (r.ms) S3D_CHECK(a->mode == S3D_STEP_DDIM, S3D_ERR_INVALID, "%s: the step's mode must be S3D_STEP_DDIM, not %d", who, a->mode);
    else if (r.known) S3D_CHECK(a->mode == S3D_STEP_DDPM || a->mode == S3D_STEP_DDIM, S3D_ERR_INVALID, "%s: a DDPM or DDIM step, not mode %d", who, a->mode);
    else if (!e.lax) S3D_CHECK(a->mode == S3D_STEP_DDPM || a->mode == S3D_STEP_DDIM || a->mode == S3D_STEP_MEAN_ONLY, S3D_ERR_INVALID, "%s: bad mode %d", who, a->mode);
    S3D_CHECK(a->mode == S3D_STEP_MEAN_ONLY || a->sample, S3D_ERR_INVALID, "%s: sample output required", who);
    S3D_CHECK(a->mode != S3D_STEP_DDPM || a->noise, S3D_ERR_INVALID, "%s: DDPM step needs noise", who);
    if (!r.ms && !e.lax) S3D_CHECK(a->mode != S3D_STEP_DDIM || a->eta == 0.f || a->noise, S3D_ERR_INVALID, "%s: eta>0 needs noise", who);
    if (r.known || r.ms) S3D_CHECK(!a->y0 && !a->mask, S3D_ERR_INVALID, "%s: the step's own y0 / mask (x0 replacement) cannot be combined with a known region or the multistep update", who);
    else if (!e.lax) S3D_CHECK((a->y0 == nullptr) == (a->mask == nullptr), S3D_ERR_INVALID, "%s: y0 and mask go together", who);
    if (r.ms) S3D_CHECK(!a->mean, S3D_ERR_INVALID, "%s: mean must be NULL (the multistep update has no posterior mean)", who);
    else if (r.known) S3D_CHECK(!a->mean || !r.model || r.model_out, S3D_ERR_INVALID, "%s: the posterior mean is only written by a step that also stores the model output (model_out != NULL)", who);
    if (r.known) S3D_CHECK(r.known->y0 && r.known->mask && r.known->noise && r.known->tables, S3D_ERR_INVALID, "%s: y0, mask, noise and tables of the known region are required", who);
    if (r.ms) {
        S3D_CHECK(r.ms->tables, S3D_ERR_INVALID, "%s: the coefficient tables are required", who);
        S3D_CHECK(r.ms->order == 1 || r.ms->order == 2, S3D_ERR_INVALID, "%s: order must be 1 or 2, not %d", who, r.ms->order);
        S3D_CHECK(r.ms->order == 1 || r.ms->x0_prev, S3D_ERR_INVALID, "%s: order 2 needs x0_prev", who);
        S3D_CHECK(r.ms->order == 1 || r.ms->x0_prev != a->pred_xstart, S3D_ERR_INVALID, "%s: x0_prev may not alias pred_xstart", who);
    }
    if (e.sizes) S3D_CHECK(a->T > 0 && a->batch >= 0 && a->per_sample >= 0, S3D_ERR_INVALID, "%s: bad sizes", who);
    return 0;
}

// the stand-alone entries: the update on a stored model output
static int sampler_entry(const char* who, const s3d_sampler_args* a, const s3d_multistep* ms, const s3d_known_region* known, void* stream) {
    S3D_TRY(check_step(StepEntry{who, false, true}, StepReq{a, known, ms}));
    return launch_sampler(*a, ms, known, static_cast<hipStream_t>(stream));
}

}  // namespace s3d

extern "C" {

int s3d_set_option(const char* name, const char* value) {
    using namespace s3d;
    const int o = find_opt(name);
    S3D_CHECK(o >= 0, S3D_ERR_INVALID, "set_option: unknown option '%s'", name ? name : "(null)");
    const bool given = value && *value;
    const int v = given ? parse_opt(o, value) : kOptUnset;
    S3D_CHECK(!given || v != kOptUnset, S3D_ERR_INVALID, "set_option: %s takes %s, not '%s'", kOptNames[o], opt_values(o), value);
    g_opt[o].store(v, std::memory_order_relaxed);
    g_opt_state[o].store(2, std::memory_order_release);
    g_opt_gen.fetch_add(1, std::memory_order_acq_rel);
    return 0;
}

int s3d_get_option(const char* name, int* value) {
    using namespace s3d;
    const int o = find_opt(name);
    S3D_CHECK(o >= 0 && value, S3D_ERR_INVALID, "get_option: unknown option '%s'", name ? name : "(null)");
    *value = opt(Opt(o));
    return 0;
}

int s3d_set_riders(int on) {
    s3d::g_riders.store(on ? 1 : 0, std::memory_order_release);
    return 0;
}

int s3d_abi_version(void) { return S3D_ABI_VERSION; }
const char* s3d_last_error(void) { return s3d::get_error(); }

int s3d_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        s3d::set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return S3D_ERR_HIP;
    }
    return n;
}

int s3d_sampler_step(const s3d_sampler_args* a, void* stream) {
    S3D_CHECK(a != nullptr, S3D_ERR_INVALID, "sampler_step: null args");
    return s3d::sampler_entry("sampler_step", a, nullptr, nullptr, stream);
}

int s3d_sampler_step_known(const s3d_sampler_args* a, const s3d_known_region* known, void* stream) {
    S3D_CHECK(a != nullptr && known != nullptr, S3D_ERR_INVALID, "sampler_step_known: null args");
    return s3d::sampler_entry("sampler_step_known", a, nullptr, known, stream);
}

int s3d_sampler_step_multistep(const s3d_sampler_args* a, const s3d_multistep* ms, const s3d_known_region* known, void* stream) {
    S3D_CHECK(a != nullptr && ms != nullptr, S3D_ERR_INVALID, "sampler_step_multistep: null args");
    return s3d::sampler_entry("sampler_step_multistep", a, ms, known, stream);
}

int s3d_sampler_renoise(const float* x_prev, const float* noise, const float* known_tables, const int64_t* t, int32_t T, int64_t batch,
                        int64_t per_sample, float* x_t, void* stream) {
    using namespace s3d;
    S3D_CHECK(x_prev && noise && known_tables && t && x_t, S3D_ERR_INVALID, "sampler_renoise: null argument");
    S3D_CHECK(T > 0 && batch >= 0 && per_sample >= 0, S3D_ERR_INVALID, "sampler_renoise: bad sizes");
    return launch_renoise(x_prev, noise, known_tables, t, T, batch, per_sample, x_t, static_cast<hipStream_t>(stream));
}

}  // extern "C"
