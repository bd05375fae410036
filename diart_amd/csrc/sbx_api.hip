// dz_sbx_*: launch sequence of the speechbrain x-vector embedding (include/diart_amd.h).  Host code.
// Fbank, the batch geometry and the NaN rules are ECAPA's (k_ecapa.hip, ecapa_api.hip) with 24 mel bins and a
// shorter minimum; the TDNN layers run on the implicit-GEMM convolution (k_convgemm.hip / k_gemm_split.hip) with
// the bias -> LeakyReLU -> BatchNorm epilogue, reflect-padded at each row's own frame count; the statistics pooling
// is sb_stats_pool_kernel; Linear(3000, 512) is split-K with the fixed-order finish.
#include "dz_common.h"

#include <string.h>
#include <new>

namespace {

// MIN_NUM_SAMPLES: the shortest signal whose reflect pads fit (largest pad 3, tdnn3: k3 dilation 3) — T = 1 + n / 160
// >= 4 frames, n >= 480 (pyannote's PretrainedSpeakerEmbedding.min_num_samples bisects for it)
enum { MIN_NUM_SAMPLES = 480, HOP = 160, NFFT = 400, NMEL = 24, C5 = 1500, C5PAD = 1536, EMB = 512, POOLED = 3000,
       POOLED_KPAD = 3008, FC_SPLIT = 16 };
// speechbrain StatisticsPooling adds noise in [1e-5, 9e-5] to the mean (_get_gauss_noise); this path adds the band's
// midpoint (DESIGN.md "speechbrain x-vector"), and eps = 1e-5 to the std
constexpr float MEAN_NOISE = 5e-5f, STD_EPS = 1e-5f;
constexpr int kTaps[5] = {5, 3, 3, 1, 1}, kDil[5] = {1, 2, 3, 1, 1}, kCin[5] = {NMEL, 512, 512, 512, 512},
              kNpad[5] = {512, 512, 512, 512, C5PAD}, kKpad[5] = {128, 1536, 1536, 512, 512};

}  // namespace

struct dz_sbx {
    dz_ctx* ctx;
    dz_sbx_weights w;
    int Nm;
    DzRowGeometry geo;
    char* arena;
    float *spec, *pw, *melp, *feats, *x[5], *pooled, *parts;
    int lastN;
};

static void sbx_carve(dz_sbx* m, Arena& a) {
    const size_t N = m->Nm, NT = N * m->geo.Tc;
    m->spec = a.take<float>(NT * 404);
    m->pw = a.take<float>(NT * 204);
    m->melp = a.take<float>(NT * NMEL);
    m->feats = a.take<float>(NT * NMEL);
    for (int l = 0; l < 4; ++l) m->x[l] = a.take<float>(NT * 512);
    m->x[4] = a.take<float>(NT * C5);
    m->pooled = a.take<float>(N * POOLED);
    m->parts = a.take<float>((size_t)FC_SPLIT * N * EMB);
    m->geo.carve(a, N);
}

extern "C" int dz_sbx_abi_size(void) { return (int)sizeof(dz_sbx_weights); }

extern "C" int dz_sbx_create(dz_ctx* ctx, const dz_sbx_weights* w, int max_rows, int num_samples, dz_sbx** out) {
    DZ_REQUIRE(ctx && w && out, "dz_sbx_create: NULL argument");
    DZ_REQUIRE(max_rows >= 1 && num_samples >= MIN_NUM_SAMPLES, "dz_sbx_create: max_rows %d, %d samples", max_rows,
               num_samples);
    DZ_HIP(hipSetDevice(ctx->device));
    dz_sbx* m = new (std::nothrow) dz_sbx;
    DZ_REQUIRE(m != nullptr, "dz_sbx_create: out of memory");
    memset(m, 0, sizeof(*m));
    m->ctx = ctx; m->w = *w; m->Nm = max_rows;
    m->geo.init(num_samples, MIN_NUM_SAMPLES);
    if (int rc = dz_arena_alloc("dz_sbx_create", m, sbx_carve)) {
        dz_sbx_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

extern "C" int dz_sbx_destroy(dz_sbx* m) {
    if (m) {
        if (m->arena) (void)hipFree(m->arena);
        delete m;
    }
    return 0;
}

// one convolution / linear launch: split-f16 when the layer has planes (and is not split-K), exact f32 otherwise
static int sbx_gemm(hipStream_t st, const float* X, int ldx, long long xbs, int B, int T, int Cin, int taps, int dil,
                    int pad, const dz_layer& L, int Kpad, int Npad, int Nstore, float* Y, int ldy, long long ybs, int epi,
                    const int* Tdev = nullptr, int ksplit = 0, long long ysplit = 0) {
    DzConvGemm p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.W = L.w; p.bias = L.b; p.e0 = L.s; p.e1 = L.h; p.Y = Y;
    p.B = B; p.Tin = T; p.Tout = pad ? T : T - (taps - 1) * dil; p.Tstore = p.Tout;
    p.Cin = Cin; p.taps = taps; p.dil = dil; p.pad = pad; p.K = taps * Cin; p.Kpad = Kpad;
    p.Npad = Npad; p.Nstore = Nstore; p.ldx = ldx; p.ldy = ldy; p.xbs = xbs; p.ybs = ybs;
    p.epi = epi; p.ksplit = ksplit; p.ysplit = ysplit; p.Tdev = Tdev;
    if (L.wsplit && ksplit <= 1) {
        p.Wsplit = L.wsplit;
        p.Npad = (Npad + 127) / 128 * 128;       // (the DFT's planes are packed with 512 rows)
        return dz_launch_gemm_split(p, st);
    }
    return dz_launch_convgemm(p, st);
}

// The forward of n_groups groups of K rows, each group with its own batch geometry, every row laid out with the
// handle's Tc frames (ecapa_api.hip's groups forward, whose geometry kernel this shares).  Row g K + k reads
// waveform row (g K + k) / rows_per_wave and mask row g K + k (or every sample when d_masks is NULL).
static int sbx_run(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks, int G, int K,
                   int rows_per_wave, int mask_frames, int normalize, float* d_out, hipStream_t st) {
    const dz_sbx_weights& w = m->w;
    DzRowGeometry& geo = m->geo;
    const int N = G * K, T = geo.Tc;
    const long long NT = (long long)N * T;
    int rc;
    if ((rc = geo.prologue(d_wave, wave_stride, d_masks, mask_frames, G, K, rows_per_wave, st))) return rc;
    m->lastN = N;
    // ---- Fbank(n_mels = 24): STFT as one GEMM over the overlapping rows, |.|^2, mel GEMM, dB / top-dB / sentence mean
    const dz_layer dft = {w.dft, w.zeros, nullptr, nullptr, w.dft_split};
    if ((rc = sbx_gemm(st, geo.sig, HOP, geo.lstride, N, T, NFFT, 1, 1, 0, dft, 416, 448, 402, m->spec, 404,
                       (long long)T * 404, DZ_EPI_BIAS)))
        return rc;
    if ((rc = dz_launch_power(m->spec, 404, NT, m->pw, st))) return rc;
    const dz_layer mel = {w.mel, w.zeros, nullptr, nullptr, nullptr};
    if ((rc = sbx_gemm(st, m->pw, 204, 0, 1, (int)NT, 204, 1, 1, 0, mel, 224, 64, NMEL, m->melp, NMEL, 0, DZ_EPI_BIAS)))
        return rc;
    if ((rc = dz_launch_fbank_post_mels(m->melp, NMEL, T, N, geo.nvalid, m->feats, st, geo.tdev))) return rc;
    // ---- TDNN 1 - 5: Conv1d (reflect "same" at the row's own frame count) -> LeakyReLU -> BatchNorm ------------
    const float* xin = m->feats;
    int ldin = NMEL;
    for (int l = 0; l < 5; ++l) {
        const int pad = kDil[l] * (kTaps[l] - 1) / 2, cout = l == 4 ? C5 : 512;
        if (pad)
            rc = sbx_gemm(st, xin, ldin, (long long)T * ldin, N, T, kCin[l], kTaps[l], kDil[l], pad, w.tdnn[l], kKpad[l],
                          kNpad[l], cout, m->x[l], cout, (long long)T * cout, DZ_EPI_TDNN, geo.tdev);
        else        // (1 x 1: every frame of every row is one GEMM row)
            rc = sbx_gemm(st, xin, ldin, 0, 1, (int)NT, kCin[l], 1, 1, 0, w.tdnn[l], kKpad[l], kNpad[l], cout, m->x[l],
                          cout, 0, DZ_EPI_TDNN);
        if (rc) return rc;
        xin = m->x[l];
        ldin = cout;
    }
    // ---- StatisticsPooling over round(rel T) frames, Linear(3000 -> 512) split-K + fixed-order finish --------------
    if ((rc = dz_launch_sb_stats_pool(m->x[4], T, C5, C5, N, geo.nvalid, MEAN_NOISE, STD_EPS, m->pooled, st))) return rc;
    const dz_layer lin = {w.lin_w, w.lin_b, nullptr, nullptr, nullptr};
    const long long ysplit = (long long)N * EMB;
    if ((rc = sbx_gemm(st, m->pooled, POOLED, 0, 1, N, POOLED, 1, 1, 0, lin, POOLED_KPAD, EMB, EMB, m->parts, EMB, 0,
                       DZ_EPI_BIAS, nullptr, FC_SPLIT, ysplit)))
        return rc;
    if ((rc = dz_launch_splitk_finish(m->parts, FC_SPLIT, ysplit, N, EMB, 0, d_out, st))) return rc;
    if ((rc = dz_launch_nan_rows(d_out, N, EMB, geo.tooshort, st))) return rc;
    return normalize ? dz_launch_l2norm(d_out, N, EMB, 1.0f, st) : 0;
}

extern "C" int dz_sbx_forward(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks, int N,
                              int mask_frames, float* d_out, void* stream) {
    if (int rc = dz_check_rows_forward("dz_sbx_forward", m, m ? m->Nm : 0, d_wave, wave_stride, d_masks, N, mask_frames,
                                       d_out))
        return rc;
    DZ_HIP(hipSetDevice(m->ctx->device));
    DzRangeScope range_scope(m->ctx->oflag_dev);
    return sbx_run(m, d_wave, wave_stride, d_masks, 1, N, 1, mask_frames, 0, d_out, (hipStream_t)stream);
}

extern "C" int dz_sbx_forward_groups(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks,
                                     int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                                     void* stream) {
    if (int rc = dz_check_groups_forward("dz_sbx_forward_groups", m, m ? m->Nm : 0, d_wave, wave_stride, d_masks,
                                         n_groups, rows_per_group, mask_frames, d_out))
        return rc;
    DZ_HIP(hipSetDevice(m->ctx->device));
    DzRangeScope range_scope(m->ctx->oflag_dev);
    return sbx_run(m, d_wave, wave_stride, d_masks, n_groups, rows_per_group, rows_per_group, mask_frames, normalize,
                   d_out, (hipStream_t)stream);
}

extern "C" int dz_sbx_peek(dz_sbx* m, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(m && d_ptr && count, "dz_sbx_peek: NULL argument");
    const long long N = m->lastN, NT = N * m->geo.Tc;
    if (frames) *frames = m->geo.Tc;
    switch (which) {
        case 0: *d_ptr = m->feats; *count = NT * NMEL; return 0;
        case 1: case 2: case 3: case 4: *d_ptr = m->x[which - 1]; *count = NT * 512; return 0;
        case 5: *d_ptr = m->x[4]; *count = NT * C5; return 0;
        case 6: *d_ptr = m->pooled; *count = N * POOLED; return 0;
        case 7: *d_ptr = m->geo.lens; *count = N; return 0;
        case 8: *d_ptr = m->geo.rep_nvalid; *count = N; return 0;
        case 9: *d_ptr = m->geo.rep_T; *count = N; return 0;
    }
    dz_set_error("dz_sbx_peek: unknown buffer %d", which);
    return 2;
}
