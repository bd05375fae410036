// dz_wsp_*: launch sequence of the WeSpeaker ResNet34 embedding (include/diart_amd.h).  Host code.
#include "dz_embed.h"

namespace {

enum { WIN = 400, HOP = 160, NMEL = 80, EMB = 256, POOLED = 5120, MAXK = 8, FC_SPLIT = 16 };
constexpr int kBlocks[4] = {3, 4, 6, 3};

int frames_for(int S, int stage) {
    if (stage < 0 || stage > 4) return -1;
    int T = S >= WIN ? 1 + (S - WIN) / HOP : 0;
    for (int l = 2; l <= stage && T > 0; ++l) T = (T - 1) / 2 + 1;    // layers 2 - 4 have stride 2
    return T;
}

}  // namespace

struct dz_wsp {
    dz_ctx* ctx;
    dz_wsp_weights w;
    int Nm, S, T[5];
    char* arena;
    float *raw, *feats, *c1, *s0, *s1, *mid, *sc, *L[4], *pooled, *parts;
    int *bad, *rflag;
    int lastN, lastRows;
};

static void wsp_carve(dz_wsp* m, Arena& a) {
    const size_t N = m->Nm, T = m->T[0];
    const size_t big = (size_t)NMEL * T * 32;                       // the largest activation: layer 1, per row
    m->raw = a.take<float>(N * NMEL * T);
    m->feats = a.take<float>(N * NMEL * T);
    m->c1 = a.take<float>(N * big);
    m->s0 = a.take<float>(N * big);
    m->s1 = a.take<float>(N * big);
    m->mid = a.take<float>(N * big);
    m->sc = a.take<float>(N * 40 * m->T[2] * 64);                   // shortcut outputs: layer 2's is the largest
    for (int l = 0; l < 4; ++l) m->L[l] = a.take<float>(N * (size_t)(NMEL >> l) * m->T[l + 1] * (32 << l));
    m->pooled = a.take<float>(N * MAXK * POOLED);
    m->parts = a.take<float>((size_t)FC_SPLIT * N * MAXK * EMB);
    m->bad = a.take<int>(N);
    m->rflag = a.take<int>(N * MAXK);
}

extern "C" int dz_wsp_abi_size(void) { return (int)sizeof(dz_wsp_weights); }

extern "C" int dz_wsp_frames_for(int num_samples, int stage) { return frames_for(num_samples, stage); }

extern "C" int dz_wsp_create(dz_ctx* ctx, const dz_wsp_weights* w, int max_rows, int num_samples, dz_wsp** out) {
    DZ_REQUIRE(ctx && w && out, "dz_wsp_create: NULL argument");
    DZ_REQUIRE(max_rows >= 1 && frames_for(num_samples, 4) >= 2, "dz_wsp_create: max_rows %d, %d samples",
               max_rows, num_samples);
    DZ_REQUIRE(w->mel && w->conv1.w && w->conv1.b && w->seg_w && w->seg_b, "dz_wsp_create: missing weights");
    for (int i = 0; i < 16; ++i)
        DZ_REQUIRE(w->block[i][0].w && w->block[i][0].b && w->block[i][1].w && w->block[i][1].b,
                   "dz_wsp_create: block %d has no weights", i);
    DZ_HIP(hipSetDevice(ctx->device));
    dz_wsp* m = new (std::nothrow) dz_wsp;
    DZ_REQUIRE(m != nullptr, "dz_wsp_create: out of memory");
    memset(m, 0, sizeof(*m));
    m->ctx = ctx; m->w = *w; m->Nm = max_rows; m->S = num_samples;
    for (int s = 0; s < 5; ++s) m->T[s] = frames_for(num_samples, s);
    if (int rc = dz_arena_alloc("dz_wsp_create", m, wsp_carve)) {
        dz_wsp_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

extern "C" int dz_wsp_destroy(dz_wsp* m) { return dz_handle_destroy(m); }

static int conv(const dz_wsp_conv& c, const float* X, int N, int Fi, int Ti, int Cin, int Cout, int taps, int stride,
                const float* R, int relu, float* Y, hipStream_t st) {
    return dz_launch_conv2d(dz_conv2d(c.w, c.wsplit, c.b, X, N, Fi, Ti, Cin, Cout, taps, stride, R, relu, nullptr, Y),
                            st);
}

// fbank -> trunk -> layer 4 output in m->L[3] for N rows
static int wsp_trunk(dz_wsp* m, const float* d_wave, long long wave_stride, int N, hipStream_t st) {
    int rc;
    const dz_wsp_weights& w = m->w;
    const int T = m->T[0];
    DZ_HIP(hipMemsetAsync(m->bad, 0, sizeof(int) * N, st));
    if ((rc = dz_launch_wsp_fbank(d_wave, wave_stride, N, T, w.mel, m->raw, m->bad, st))) return rc;
    if ((rc = dz_launch_wsp_cmn(m->raw, N, T, m->bad, m->feats, st))) return rc;
    if ((rc = dz_launch_wsp_conv1(m->feats, N, T, w.conv1.w, w.conv1.b, m->c1, st))) return rc;
    const float* x = m->c1;
    int F = NMEL, Tt = T, Cin = 32, bi = 0;
    for (int l = 0; l < 4; ++l) {
        const int C = 32 << l, stride = l ? 2 : 1;
        for (int j = 0; j < kBlocks[l]; ++j, ++bi) {
            const int s = j ? 1 : stride;
            const int Fo = (F - 1) / s + 1, To = (Tt - 1) / s + 1;
            float* y = j == kBlocks[l] - 1 ? m->L[l] : (j & 1 ? m->s1 : m->s0);
            if ((rc = conv(w.block[bi][0], x, N, F, Tt, Cin, C, 9, s, nullptr, 1, m->mid, st))) return rc;
            const float* R = x;
            if (w.block[bi][2].w) {
                if ((rc = conv(w.block[bi][2], x, N, F, Tt, Cin, C, 1, s, nullptr, 0, m->sc, st))) return rc;
                R = m->sc;
            } else {
                DZ_REQUIRE(s == 1 && Cin == C, "dz_wsp: block %d needs a shortcut convolution", bi);
            }
            if ((rc = conv(w.block[bi][1], m->mid, N, Fo, To, C, C, 9, 1, R, 1, y, st))) return rc;
            x = y;
            F = Fo; Tt = To; Cin = C;
        }
    }
    return 0;
}

// pooling + seg_1 of `rows` = N K pool rows -> d_out (rows, 256)
static int wsp_head(dz_wsp* m, int N, int K, const float* d_weights, int Fw, int normalize, float* d_out, hipStream_t st) {
    int rc;
    const int rows = N * K;
    if ((rc = dz_launch_wsp_pool(m->L[3], N, m->T[4], d_weights, Fw, K, m->bad, m->pooled, m->rflag, st))) return rc;
    // seg_1: rows x 5120 -> 256, split-K with a fixed-order reduce (k_pool.hip) on the exact-f32 GEMM
    const dz_layer seg = {m->w.seg_w, m->w.seg_b, nullptr, nullptr, nullptr};
    if ((rc = dz_splitk_linear(seg, m->pooled, rows, POOLED, POOLED, EMB, FC_SPLIT, m->parts, normalize ? 1 : 0, d_out, st)))
        return rc;
    m->lastRows = rows;
    return dz_launch_nan_rows(d_out, rows, EMB, m->rflag, st);
}

extern "C" int dz_wsp_forward(dz_wsp* m, const float* d_wave, long long wave_stride, const float* d_weights, int n_rows,
                              int weight_frames, float* d_out, void* stream) {
    int rc = dz_check_rows_forward("dz_wsp_forward", m, m ? m->Nm : 0, d_wave, wave_stride, d_weights, n_rows,
                                   weight_frames, d_out, "weight_frames");
    if (rc) return rc;
    DZ_HIP(hipSetDevice(m->ctx->device));
    DzRangeScope range_scope(m->ctx->oflag_dev);
    hipStream_t st = (hipStream_t)stream;
    m->lastN = n_rows;
    if ((rc = wsp_trunk(m, d_wave, wave_stride, n_rows, st))) return rc;
    return wsp_head(m, n_rows, 1, d_weights, weight_frames, 0, d_out, st);
}

extern "C" int dz_wsp_trunk(dz_wsp* m, const float* d_wave, long long wave_stride, int batch, void* stream) {
    DZ_REQUIRE(m && d_wave, "dz_wsp_trunk: NULL argument");
    DZ_REQUIRE(batch >= 1 && batch <= m->Nm, "dz_wsp_trunk: batch %d outside [1, %d]", batch, m->Nm);
    DZ_REQUIRE(wave_stride >= 0, "dz_wsp_trunk: negative stride");
    DZ_HIP(hipSetDevice(m->ctx->device));
    DzRangeScope range_scope(m->ctx->oflag_dev);
    m->lastN = batch;
    return wsp_trunk(m, d_wave, wave_stride, batch, (hipStream_t)stream);
}

extern "C" int dz_wsp_pool(dz_wsp* m, const float* d_weights, int batch, int num_speakers, int weight_frames,
                           int normalize, float* d_out, void* stream) {
    DZ_REQUIRE(m && d_weights && d_out, "dz_wsp_pool: NULL argument");
    DZ_REQUIRE(batch >= 1 && batch == m->lastN, "dz_wsp_pool: batch %d, the handle's last trunk ran %d", batch,
               m->lastN);
    DZ_REQUIRE(num_speakers >= 1 && num_speakers <= MAXK, "dz_wsp_pool: %d speakers outside [1, %d]", num_speakers,
               (int)MAXK);
    DZ_REQUIRE(weight_frames >= 1, "dz_wsp_pool: weight_frames %d", weight_frames);
    DZ_HIP(hipSetDevice(m->ctx->device));
    DzRangeScope range_scope(m->ctx->oflag_dev);
    return wsp_head(m, batch, num_speakers, d_weights, weight_frames, normalize, d_out, (hipStream_t)stream);
}

// the two halves on one stream; every argument is checked before the first launch
extern "C" int dz_wsp_forward_multi(dz_wsp* m, const float* d_wave, long long wave_stride, const float* d_weights,
                                    int batch, int num_speakers, int weight_frames, int normalize, float* d_out,
                                    void* stream) {
    DZ_REQUIRE(m && d_wave && d_weights && d_out, "dz_wsp_forward_multi: NULL argument");
    DZ_REQUIRE(batch >= 1 && batch <= m->Nm, "dz_wsp_forward_multi: batch %d outside [1, %d]", batch, m->Nm);
    DZ_REQUIRE(num_speakers >= 1 && num_speakers <= MAXK, "dz_wsp_forward_multi: %d speakers outside [1, %d]",
               num_speakers, (int)MAXK);
    DZ_REQUIRE(weight_frames >= 1, "dz_wsp_forward_multi: weight_frames %d", weight_frames);
    DZ_REQUIRE(wave_stride >= 0, "dz_wsp_forward_multi: negative stride");
    if (int rc = dz_wsp_trunk(m, d_wave, wave_stride, batch, stream)) return rc;
    return dz_wsp_pool(m, d_weights, batch, num_speakers, weight_frames, normalize, d_out, stream);
}

// kernel-level entry points of k_conv2d.hip (parity tests): the launcher checks the operands
static int k_conv2d(dz_ctx* ctx, const float* d_x, const float* d_w, const void* d_wsplit, const float* d_bias,
                    const float* d_r, const int* d_ext, float* d_y, int batch, int fi, int ti, int cin, int cout,
                    int taps, int stride, int relu, void* stream) {
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_conv2d(
        dz_conv2d(d_w, d_wsplit, d_bias, d_x, batch, fi, ti, cin, cout, taps, stride, d_r, relu, d_ext, d_y),
        (hipStream_t)stream);
}

extern "C" int dz_k_conv2d(dz_ctx* ctx, const float* d_x, const float* d_w, const void* d_wsplit, const float* d_bias,
                           const float* d_r, float* d_y, int batch, int fi, int ti, int cin, int cout, int taps,
                           int stride, int relu, void* stream) {
    DZ_REQUIRE(ctx != nullptr, "dz_k_conv2d: NULL context");
    return k_conv2d(ctx, d_x, d_w, d_wsplit, d_bias, d_r, nullptr, d_y, batch, fi, ti, cin, cout, taps, stride, relu,
                    stream);
}

// the same with a row's live steps of the f axis (the masked instances; sbr_api.hip runs the trunk on them)
extern "C" int dz_k_conv2d_masked(dz_ctx* ctx, const float* d_x, const float* d_w, const void* d_wsplit,
                                  const float* d_bias, const float* d_r, const int* d_ext, float* d_y, int batch, int fi,
                                  int ti, int cin, int cout, int taps, int stride, int relu, void* stream) {
    DZ_REQUIRE(ctx != nullptr && d_ext != nullptr, "dz_k_conv2d_masked: NULL context or extents");
    return k_conv2d(ctx, d_x, d_w, d_wsplit, d_bias, d_r, d_ext, d_y, batch, fi, ti, cin, cout, taps, stride, relu,
                    stream);
}

extern "C" int dz_wsp_peek(dz_wsp* m, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(m && d_ptr && count, "dz_wsp_peek: NULL argument");
    const long long N = m->lastN;
    int T = 0;
    switch (which) {
        case 0: *d_ptr = m->feats; T = m->T[0]; *count = N * NMEL * T; break;
        case 1: *d_ptr = m->c1; T = m->T[0]; *count = N * NMEL * T * 32; break;
        case 2: case 3: case 4: case 5: {
            const int l = which - 2;
            *d_ptr = m->L[l]; T = m->T[l + 1];
            *count = N * (NMEL >> l) * T * (32 << l);
            break;
        }
        case 6: *d_ptr = m->pooled; T = m->T[4]; *count = (long long)m->lastRows * POOLED; break;
        case 7: *d_ptr = m->raw; T = m->T[0]; *count = N * NMEL * T; break;
        default:
            dz_set_error("dz_wsp_peek: unknown buffer %d", which);
            return 2;
    }
    if (frames) *frames = T;
    return 0;
}
