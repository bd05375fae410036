// dz_resample_*: geometry, filter table and device handle of the band-limited resampler (include/diart_amd.h;
// kernels: k_resample.hip; definition: DESIGN.md "Resampling").  Host code.
#include "dz_common.h"

#include <math.h>
#include <string.h>
#include <new>
#include <vector>

namespace {

constexpr int LOWPASS_WIDTH = 6;
constexpr double ROLLOFF = 0.99;
constexpr long long MAX_TABLE_BYTES = 16ll << 20;   // refuse ratios whose (padded) table exceeds 16 MiB

struct Geometry {
    int o, n, width, T, n_pad;
    bool tap_major;
};

long long gcd_ll(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int geometry(int orig, int target, Geometry* g, const char* who) {
    DZ_REQUIRE(orig > 0 && target > 0, "%s: sample rates must be positive (got %d -> %d)", who, orig, target);
    const long long d = gcd_ll(orig, target);
    g->o = (int)(orig / d);
    g->n = (int)(target / d);
    const double base = (double)(g->o < g->n ? g->o : g->n) * ROLLOFF;
    const double w = ceil((double)LOWPASS_WIDTH * g->o / base);
    DZ_REQUIRE(w < 1e8, "%s: %d -> %d Hz needs a filter of %.0f taps", who, orig, target, 2 * w);
    g->width = (int)w;
    const long long T = 2ll * g->width + g->o;
    g->tap_major = g->n >= 64;
    g->n_pad = g->tap_major ? (g->n + 63) / 64 * 64 : g->n;
    const long long bytes = (long long)g->n_pad * T * 4;
    DZ_REQUIRE(T < (1ll << 30) && bytes <= MAX_TABLE_BYTES,
               "%s: %d -> %d Hz (%d phases x %lld taps) needs a %lld-byte filter table, more than the %lld bytes "
               "this resampler accepts", who, orig, target, g->n, T, bytes, MAX_TABLE_BYTES);
    g->T = (int)T;
    return 0;
}

// torchaudio's _get_sinc_resample_kernel (sinc_interp_hann) in float64, rounded to float32: phase-major [n][T]
void fill_table(const Geometry& g, float* h) {
    const double base = (double)(g.o < g.n ? g.o : g.n) * ROLLOFF;
    for (int i = 0; i < g.n; ++i) {
        for (int k = 0; k < g.T; ++k) {
            double t = ((double)-i / g.n + (double)(k - g.width) / g.o) * base;
            t = t < -LOWPASS_WIDTH ? -LOWPASS_WIDTH : (t > LOWPASS_WIDTH ? LOWPASS_WIDTH : t);
            const double c = cos(t * M_PI / LOWPASS_WIDTH / 2);
            const double win = c * c;
            const double pt = t * M_PI;
            const double s = pt == 0.0 ? 1.0 : sin(pt) / pt;
            h[(size_t)i * g.T + k] = (float)(s * (win * (base / g.o)));
        }
    }
}

}  // namespace

struct dz_resample {
    int device;
    int orig, target;
    Geometry g;
    float* table;       // device: tap-major [T][n_pad] (n >= 64) or phase-major [n][T]; NULL at equal rates
};

extern "C" int dz_resample_geometry(int orig_freq, int new_freq, int* phases, int* taps, int* width, int* in_step) {
    Geometry g;
    const int rc = geometry(orig_freq, new_freq, &g, "dz_resample_geometry");
    if (rc) return rc;
    if (phases) *phases = g.n;
    if (taps) *taps = g.T;
    if (width) *width = g.width;
    if (in_step) *in_step = g.o;
    return 0;
}

extern "C" long long dz_resample_out_len(int orig_freq, int new_freq, long long in_len) {
    if (orig_freq <= 0 || new_freq <= 0 || in_len < 0) return -1;
    if (orig_freq == new_freq) return in_len;
    const long long d = gcd_ll(orig_freq, new_freq), o = orig_freq / d, n = new_freq / d;
    if (in_len > 0 && n > (1ll << 62) / in_len) return -1;
    return (n * in_len + o - 1) / o;
}

extern "C" int dz_resample_table(int orig_freq, int new_freq, float* out) {
    DZ_REQUIRE(out, "dz_resample_table: NULL output");
    Geometry g;
    const int rc = geometry(orig_freq, new_freq, &g, "dz_resample_table");
    if (rc) return rc;
    fill_table(g, out);
    return 0;
}

extern "C" int dz_resample_create(dz_ctx* ctx, int orig_freq, int new_freq, dz_resample** out) {
    DZ_REQUIRE(ctx && out, "dz_resample_create: NULL argument");
    Geometry g;
    const int rc = geometry(orig_freq, new_freq, &g, "dz_resample_create");
    if (rc) return rc;
    DZ_HIP(hipSetDevice(ctx->device));
    dz_resample* m = new (std::nothrow) dz_resample;
    DZ_REQUIRE(m != nullptr, "dz_resample_create: out of memory");
    m->device = ctx->device;
    m->orig = orig_freq;
    m->target = new_freq;
    m->g = g;
    m->table = nullptr;
    if (orig_freq != new_freq) {
        std::vector<float> ph((size_t)g.n * g.T), dev((size_t)g.n_pad * g.T, 0.f);
        fill_table(g, ph.data());
        if (g.tap_major) {
            for (int i = 0; i < g.n; ++i)
                for (int k = 0; k < g.T; ++k) dev[(size_t)k * g.n_pad + i] = ph[(size_t)i * g.T + k];
        } else {
            dev.swap(ph);
        }
        const size_t bytes = dev.size() * sizeof(float);
        hipError_t err = hipMalloc((void**)&m->table, bytes);
        if (err == hipSuccess) err = hipMemcpy(m->table, dev.data(), bytes, hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            dz_set_error("dz_resample_create: table upload (%zu bytes) failed: %s", bytes, hipGetErrorString(err));
            if (m->table) (void)hipFree(m->table);
            delete m;
            return 1;
        }
    }
    *out = m;
    return 0;
}

extern "C" int dz_resample_forward(dz_resample* m, const float* d_in, long long in_stride, long long in_len, int rows,
                                   float* d_out, long long out_stride, void* stream) {
    DZ_REQUIRE(m && d_in && d_out, "dz_resample_forward: NULL argument");
    DZ_REQUIRE(rows >= 0 && in_len >= 0, "dz_resample_forward: %d rows of %lld samples", rows, in_len);
    const long long out_len = dz_resample_out_len(m->orig, m->target, in_len);
    DZ_REQUIRE(out_len >= 0, "dz_resample_forward: %lld samples overflow the output length", in_len);
    // input rows may overlap (a rolling window batch is a view at the hop); output rows may not
    DZ_REQUIRE(rows <= 1 || (in_stride >= 0 && out_stride >= out_len),
               "dz_resample_forward: strides %lld in / %lld out for rows of %lld -> %lld samples", in_stride,
               out_stride, in_len, out_len);
    if (rows == 0 || out_len == 0) return 0;
    DZ_HIP(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    if (m->table == nullptr) {   // equal rates: the input as it is (a copy, no kernel)
        for (int r = 0; r < rows; ++r)
            DZ_HIP(hipMemcpyAsync(d_out + (long long)r * out_stride, d_in + (long long)r * in_stride,
                                  (size_t)in_len * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    const Geometry& g = m->g;
    return dz_launch_resample(d_in, in_stride, in_len, rows, m->table, g.tap_major ? 1 : 0, g.n, g.n_pad, g.o,
                              g.width, g.T, d_out, out_stride, out_len, st);
}

extern "C" int dz_resample_destroy(dz_resample* m) {
    if (m) {
        if (m->table) {
            (void)hipSetDevice(m->device);
            (void)hipFree(m->table);
        }
        delete m;
    }
    return 0;
}
