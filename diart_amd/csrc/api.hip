// What every part of libdiart_amd.so (include/diart_amd.h) shares: errors, the context, the per-kernel profiler, the
// run-time options; and the entry points that belong to no handle (wave statistics, small ops).  The launch
// sequences of the networks are in *_api.hip, the kernel-level entry points in kernel_api.hip.  Host code.
#include "dz_sincnet.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <new>

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void dz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* dz_last_error(void) { return g_err; }
extern "C" int dz_version(void) { return DZ_VERSION; }
extern "C" int dz_abi_struct_sizes(int out[5]) {
    if (!out) return 2;
    out[0] = (int)sizeof(dz_sincnet_weights);
    out[1] = (int)sizeof(dz_seg_weights);
    out[2] = (int)sizeof(dz_emb_weights);
    out[3] = (int)sizeof(dz_ecapa_weights);
    out[4] = (int)sizeof(dz_convgemm_desc);
    return 0;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" int dz_ctx_create(int hip_device, dz_ctx** out) {
    DZ_REQUIRE(out != nullptr, "dz_ctx_create: out is NULL");
    int n = 0;
    DZ_HIP(hipGetDeviceCount(&n));
    DZ_REQUIRE(hip_device >= 0 && hip_device < n, "dz_ctx_create: device %d of %d", hip_device, n);
    hipDeviceProp_t prop;
    DZ_HIP(hipGetDeviceProperties(&prop, hip_device));
    DZ_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
               "dz_ctx_create: device %d is %s, this library is built for gfx950 only", hip_device,
               prop.gcnArchName);
    dz_ctx* c = new (std::nothrow) dz_ctx;
    DZ_REQUIRE(c != nullptr, "dz_ctx_create: out of memory");
    c->device = hip_device;
    c->oflag_host = c->oflag_dev = nullptr;
    c->conv0_frag = c->convp_frag = nullptr;
    c->conv0_src = c->convp_src = nullptr;
    c->conv0_user = c->convp_user = nullptr;
    c->conv0_used = c->convp_used = false;
    c->convp_cin = c->convp_kpad = 0;
    c->rr_flags = c->rr_host = c->rr_dev = nullptr;
    c->rr_cap = 0;
    c->rr_user = nullptr;
    c->rr_dirty = false;
    DZ_HIP(hipSetDevice(hip_device));
    DZ_HIP(hipHostMalloc((void**)&c->oflag_host, sizeof(int), hipHostMallocMapped));
    *c->oflag_host = 0;
    DZ_HIP(hipHostGetDevicePointer((void**)&c->oflag_dev, c->oflag_host, 0));
    DZ_HIP(hipHostMalloc((void**)&c->rr_host, sizeof(int), hipHostMallocMapped));
    *c->rr_host = 0;
    DZ_HIP(hipHostGetDevicePointer((void**)&c->rr_dev, c->rr_host, 0));
    *out = c;
    return 0;
}
extern "C" int dz_ctx_destroy(dz_ctx* ctx) {
    if (ctx && ctx->oflag_host) (void)hipHostFree(ctx->oflag_host);
    if (ctx && ctx->conv0_frag) (void)hipFree(ctx->conv0_frag);
    if (ctx && ctx->convp_frag) (void)hipFree(ctx->convp_frag);
    if (ctx && ctx->rr_host) (void)hipHostFree(ctx->rr_host);
    if (ctx && ctx->rr_flags) (void)hipFree(ctx->rr_flags);
    delete ctx;
    return 0;
}
extern "C" int dz_range_check(dz_ctx* ctx, int reset) {
    DZ_REQUIRE(ctx != nullptr, "dz_range_check: NULL context");
    const int seen = *(volatile int*)ctx->oflag_host;
    if (reset) *(volatile int*)ctx->oflag_host = 0;
    if (seen) {
        dz_set_error("an operand of a split-f16 (\"f16x3\") kernel was outside +-65504 and has been clamped: "
                     "the result differs from an f32 reference; use precision=\"f32\" for such inputs");
        return 6;
    }
#ifdef DZ_EXPERIMENTS
    DZ_HIP(hipSetDevice(ctx->device));
    if (dz_g3_error(reset)) {
        dz_set_error("k_gemm_g3.hip: a workgroup gave up waiting for the partial sums of a neighbour (the results of "
                     "that launch are wrong); DZ_GEMM_GEN=1 selects the non-persistent kernel");
        return 7;
    }
#endif
    return 0;
}

// ---------------------------------------------------------------------------
// per-kernel timing (bench.py's roofline leg).  Off by default; when on, every launch issued by
// the forward passes carries a (start, stop) event pair from a fixed pool that the runtime fills
// with the dispatch's own timestamps (DZ_LAUNCH / hipExtLaunchKernelGGL): kernel execution time on
// whatever stream it ran, no marker packets between kernels.  dz_prof_collect() synchronises and
// accumulates.
// ---------------------------------------------------------------------------
enum { PROF_POOL = 8192, PROF_TAGS = DZ_T_COUNT };
// indexed by DzProfTag (dz_common.h)
static const char* const kProfNames[] = {
    "wave_stats", "sinc_conv0", "finalize_norm", "conv1_pool", "conv2_pool", "lstm_proj",
    "lstm_rec", "seg_mlp", "seg_classifier", "tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5",
    "stats_pool", "emb_linear", "l2norm", "osp", "powerset", "cdist", "lstm_proj0",
    // config 3 (ecapa_api.hip)
    "ecapa_fbank", "ecapa_block0", "ecapa_wide1x1", "ecapa_res2net", "ecapa_se", "ecapa_asp", "ecapa_fc",
    "sinc_conv0_pair", "norm_split"};
static_assert(sizeof(kProfNames) / sizeof(kProfNames[0]) == DZ_T_COUNT, "one name per DzProfTag, in its order");
thread_local DzLaunchProf* dz_launch_prof = nullptr;
thread_local int* dz_cur_oflag = nullptr;
struct Prof {
    bool on = false;
    int used = 0;
    DzLaunchProf ev[PROF_POOL];
    int tag[PROF_POOL];
    int units[PROF_POOL];        // chunks the bracketed launch works on
    bool made = false;
    double ms[PROF_TAGS];
    long long n[PROF_TAGS];
    long long chunks[PROF_TAGS];
};
// One profiler per process, shared by every handle and host thread: slots are handed out under a
// lock (the forward passes of different handles may be driven from different threads); the
// "consumed by the next DZ_LAUNCH" hand-off itself is thread local.
static Prof g_prof;
static std::mutex g_prof_mu;
// `chunks`: how many 5 s chunks (ECAPA: embedding rows) this launch processes — the unit bench.py's roofline counts in
DzProfScope::DzProfScope(int tag, int chunks) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof.on && g_prof.used < PROF_POOL && tag >= 0 && tag < PROF_TAGS) {
        const int slot = g_prof.used++;
        g_prof.tag[slot] = tag;
        g_prof.units[slot] = chunks;
        dz_launch_prof = &g_prof.ev[slot];   // consumed by the next DZ_LAUNCH
    }
}
DzProfScope::~DzProfScope() { dz_launch_prof = nullptr; }
extern "C" int dz_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (on && !g_prof.made) {
        for (int i = 0; i < PROF_POOL; ++i) {
            DZ_HIP(hipEventCreate(&g_prof.ev[i].start));
            DZ_HIP(hipEventCreate(&g_prof.ev[i].stop));
        }
        g_prof.made = true;
    }
    g_prof.on = on != 0;
    g_prof.used = 0;
    for (int t = 0; t < PROF_TAGS; ++t) { g_prof.ms[t] = 0.0; g_prof.n[t] = 0; g_prof.chunks[t] = 0; }
    return 0;
}
// suspend / resume the bracketing without touching what has been accumulated: bench.py instruments
// every k-th step of its timed region only (a dispatch that carries profiling events costs the
// runtime ~15 % of throughput when every launch has one)
extern "C" int dz_prof_pause(int paused) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof.made) g_prof.on = !paused;
    return 0;
}
// drains the event pool (device must be idle or will be synchronised); returns #tags
extern "C" int dz_prof_collect(void) {
    DZ_HIP(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_prof_mu);
    // DZ_PROF_TIMELINE=<file>: additionally append "tag chunks start_us duration_us" of every bracketed launch
    // (start relative to the first one of this drain; the dispatches' own timestamps, whatever stream they
    // ran on) — the step's schedule without a tracer slowing the host down (tools/timeline.py)
    const char* tl_path = getenv("DZ_PROF_TIMELINE");
    FILE* tl = tl_path && tl_path[0] && g_prof.used > 0 ? fopen(tl_path, "a") : nullptr;
    if (tl) fprintf(tl, "# drain of %d launches\n", g_prof.used);
    for (int i = 0; i < g_prof.used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof.ev[i].start, g_prof.ev[i].stop) == hipSuccess) {
            g_prof.ms[g_prof.tag[i]] += ms;
            g_prof.n[g_prof.tag[i]] += 1;
            g_prof.chunks[g_prof.tag[i]] += g_prof.units[i];
            float t0 = 0.f;
            if (tl && hipEventElapsedTime(&t0, g_prof.ev[0].start, g_prof.ev[i].start) == hipSuccess)
                fprintf(tl, "%s %d %.1f %.1f\n", kProfNames[g_prof.tag[i]], g_prof.units[i], t0 * 1e3, ms * 1e3);
        }
    }
    if (tl) fclose(tl);
    g_prof.used = 0;
    // an event pair whose bracket never launched (a ProfScope around a path that returned early) fails
    // in hipEventElapsedTime: it is skipped above, and the runtime's sticky "last error" must not be left
    // for the next caller's error check (torch raises on it)
    (void)hipGetLastError();
    return PROF_TAGS;
}
extern "C" int dz_prof_get(int tag, const char** name, double* total_ms, long long* launches,
                           long long* chunks) {
    if (tag < 0 || tag >= PROF_TAGS) return 2;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (name) *name = kProfNames[tag];
    if (total_ms) *total_ms = g_prof.ms[tag];
    if (launches) *launches = g_prof.n[tag];
    if (chunks) *chunks = g_prof.chunks[tag];
    return 0;
}

// ---- run-time options (dz_common.h) ----------------------------------------------------------------
static int g_options[DZ_OPT_COUNT] = {1, 1, 0};
static const char* const kOptionNames[DZ_OPT_COUNT] = {"f32_gemm", "pool_fuse", "pack_cache"};
int dz_option(int id) { return id >= 0 && id < DZ_OPT_COUNT ? __atomic_load_n(&g_options[id], __ATOMIC_RELAXED) : 0; }
static int option_index(const char* name) {
    for (int i = 0; name && i < DZ_OPT_COUNT; ++i)
        if (strcmp(name, kOptionNames[i]) == 0) return i;
    return -1;
}
extern "C" int dz_set_option(const char* name, int value) {
    const int i = option_index(name);
    DZ_REQUIRE(i >= 0, "dz_set_option: unknown option '%s' (f32_gemm, pool_fuse, pack_cache)", name ? name : "(null)");
    __atomic_store_n(&g_options[i], value, __ATOMIC_RELAXED);
    return 0;
}
extern "C" int dz_get_option(const char* name, int* value) {
    const int i = option_index(name);
    DZ_REQUIRE(i >= 0 && value, "dz_get_option: unknown option '%s' (f32_gemm, pool_fuse, pack_cache)", name ? name : "(null)");
    *value = dz_option(i);
    return 0;
}
extern "C" int dz_has_experiments(void) {
#ifdef DZ_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

// ---------------------------------------------------------------------------
// InstanceNorm1d(1) statistics of the windows, shared by both networks
// ---------------------------------------------------------------------------
extern "C" int dz_wave_stats_floats(void) { return 2 * DZ_WS_G; }
extern "C" int dz_wave_stats(dz_ctx* ctx, const float* d_wave, long long wave_stride, int batch,
                             int num_samples, float* d_moments, void* stream) {
    DZ_REQUIRE(ctx && d_moments, "dz_wave_stats: NULL argument");
    DZ_REQUIRE(batch >= 1 && num_samples >= 1, "dz_wave_stats: empty input");
    int rc;
    if ((rc = check_wave("dz_wave_stats", d_wave, wave_stride, num_samples))) return rc;
    DZ_HIP(hipSetDevice(ctx->device));
    DzProfScope ps(DZ_T_WAVE, batch);
    return dz_launch_wave_stats(d_wave, wave_stride, batch, num_samples, d_moments, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// small ops
// ---------------------------------------------------------------------------
extern "C" int dz_osp(dz_ctx* ctx, const float* d_seg, int batch, int frames, int speakers,
                      float gamma, float beta, int normalize, int speaker_major, float* d_out,
                      void* stream) {
    DZ_REQUIRE(ctx && d_seg && d_out, "dz_osp: NULL argument");
    DZ_REQUIRE(batch >= 1 && frames >= 1, "dz_osp: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    DzProfScope ps(DZ_T_OSP, batch);
    return dz_launch_osp(d_seg, batch, frames, speakers, gamma, beta, normalize, speaker_major,
                         d_out, (hipStream_t)stream);
}

extern "C" int dz_l2_normalize(dz_ctx* ctx, float* d_emb, int rows, int dim, float norm,
                               void* stream) {
    DZ_REQUIRE(ctx && d_emb, "dz_l2_normalize: NULL argument");
    DZ_REQUIRE(rows >= 1 && dim >= 1, "dz_l2_normalize: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_l2norm(d_emb, rows, dim, norm, (hipStream_t)stream);
}

extern "C" int dz_cdist_cosine(dz_ctx* ctx, const float* d_emb, const double* d_centers,
                               int n_streams, int k_local, int g_global, int dim, double* d_out,
                               void* stream) {
    DZ_REQUIRE(ctx && d_emb && d_centers && d_out, "dz_cdist_cosine: NULL argument");
    DZ_REQUIRE(n_streams >= 1 && k_local >= 1 && g_global >= 1 && dim >= 1,
               "dz_cdist_cosine: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_cdist(d_emb, d_centers, n_streams, k_local, g_global, dim, d_out,
                           (hipStream_t)stream);
}

extern "C" int dz_rows_repeat(dz_ctx* ctx, const float* d_wave, long long wave_stride, int n_rows, int num_samples,
                              void* stream, int* repeat_out) {
    DZ_REQUIRE(ctx && d_wave && repeat_out, "dz_rows_repeat: NULL argument");
    DZ_REQUIRE(((uintptr_t)d_wave & 3) == 0, "dz_rows_repeat: d_wave %p is not a float address", (const void*)d_wave);
    DZ_REQUIRE(n_rows >= 1 && num_samples >= 1, "dz_rows_repeat: %d rows of %d samples", n_rows, num_samples);
    DZ_REQUIRE(n_rows == 1 || wave_stride >= 0, "dz_rows_repeat: negative stride %lld", wave_stride);
    if (n_rows == 1) {
        *repeat_out = 1;
        return 0;
    }
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    DZ_HIP(hipStreamIsCapturing(st, &capturing));
    DZ_REQUIRE(capturing == hipStreamCaptureStatusNone,
               "dz_rows_repeat: the stream is being captured; this call waits for its answer and cannot be part of a graph");
    std::lock_guard<std::mutex> lock(ctx->rr_mu);
    if (ctx->rr_dirty) {                          // the previous call's wait failed: its kernels may still own the flags
        DZ_HIP(hipStreamSynchronize(ctx->rr_user));
        if (ctx->rr_flags) DZ_HIP(hipMemsetAsync(ctx->rr_flags, 0, (size_t)ctx->rr_cap * sizeof(int), st));
        ctx->rr_dirty = false;
    }
    if (n_rows > ctx->rr_cap) {                   // (no kernel of an earlier call is running: every call ends in a wait)
        if (ctx->rr_flags) DZ_HIP(hipFree(ctx->rr_flags));
        ctx->rr_flags = nullptr;
        ctx->rr_cap = 0;
        const int cap = n_rows < 1024 ? 1024 : n_rows;
        DZ_HIP(hipMalloc((void**)&ctx->rr_flags, (size_t)cap * sizeof(int)));
        ctx->rr_cap = cap;
        DZ_HIP(hipMemsetAsync(ctx->rr_flags, 0, (size_t)cap * sizeof(int), st));
    }
    ctx->rr_user = st;
    ctx->rr_dirty = true;
    int rc;
    if ((rc = dz_launch_rows_repeat(d_wave, wave_stride, n_rows, num_samples, ctx->rr_flags, ctx->rr_dev, st))) return rc;
    DZ_HIP(hipStreamSynchronize(st));             // the one wait: four bytes of verdict
    ctx->rr_dirty = false;
    const int r = *(volatile int*)ctx->rr_host;
    DZ_REQUIRE(r >= 1 && n_rows % r == 0, "dz_rows_repeat: the device answered %d for %d rows", r, n_rows);
    *repeat_out = r;
    return 0;
}
