// dz_sbx_*: launch sequence of the speechbrain x-vector embedding (include/diart_amd.h).  Host code.
// Fbank, the batch geometry and the NaN rules are ECAPA's (k_ecapa.hip, ecapa_api.hip) with 24 mel bins and a
// shorter minimum; the TDNN layers run on the implicit-GEMM convolution (k_convgemm.hip / k_gemm_split.hip) with
// the bias -> LeakyReLU -> BatchNorm epilogue, reflect-padded at each row's own frame count; the statistics pooling
// is sb_stats_pool_kernel; Linear(3000, 512) is split-K with the fixed-order finish.
#include "dz_embed.h"

namespace {

// MIN_NUM_SAMPLES: the shortest signal whose reflect pads fit (largest pad 3, tdnn3: k3 dilation 3) — T = 1 + n / 160
// >= 4 frames, n >= 480 (pyannote's PretrainedSpeakerEmbedding.min_num_samples bisects for it)
enum { MIN_NUM_SAMPLES = 480, NMEL = 24, C5 = 1500, C5PAD = 1536, EMB = 512, POOLED = 3000,
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
    return dz_handle_create("dz_sbx_create", ctx, w, max_rows, num_samples, MIN_NUM_SAMPLES, sbx_carve, out);
}

extern "C" int dz_sbx_destroy(dz_sbx* m) { return dz_handle_destroy(m); }

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
    // ---- Fbank(n_mels = 24): STFT, |.|^2, mel GEMM (dz_fbank_front), dB / top-dB / sentence mean -----------------
    const dz_layer dft = {w.dft, w.zeros, nullptr, nullptr, w.dft_split};
    const dz_layer mel = {w.mel, w.zeros, nullptr, nullptr, nullptr};
    if ((rc = dz_fbank_front(dft, mel, geo.sig, geo.lstride, N, T, m->spec, m->pw, NMEL, 64, m->melp, st))) return rc;
    if ((rc = dz_launch_fbank_post(m->melp, NMEL, T, N, geo.nvalid, m->feats, st, geo.tdev))) return rc;
    // ---- TDNN 1 - 5: Conv1d (reflect "same" at the row's own frame count) -> LeakyReLU -> BatchNorm ------------
    const float* xin = m->feats;
    int ldin = NMEL;
    for (int l = 0; l < 5; ++l) {
        const int pad = kDil[l] * (kTaps[l] - 1) / 2, cout = l == 4 ? C5 : 512;
        // (a 1 x 1 layer is dense: every frame of every row is one GEMM row)
        DzGemm g = pad ? DzGemm::conv1d(w.tdnn[l], xin, ldin, N, T, kCin[l], m->x[l], cout, cout, DZ_EPI_TDNN)
                             .taps(kTaps[l], kDil[l], pad).tdev(geo.tdev)
                       : DzGemm::dense(w.tdnn[l], xin, ldin, NT, kCin[l], m->x[l], cout, cout, DZ_EPI_TDNN);
        if ((rc = g.padded(kKpad[l], kNpad[l]).run(st))) return rc;
        xin = m->x[l];
        ldin = cout;
    }
    // ---- StatisticsPooling over round(rel T) frames, Linear(3000 -> 512) split-K + fixed-order finish --------------
    if ((rc = dz_launch_sb_stats_pool(m->x[4], T, C5, C5, N, geo.nvalid, MEAN_NOISE, STD_EPS, m->pooled, st))) return rc;
    const dz_layer lin = {w.lin_w, w.lin_b, nullptr, nullptr, nullptr};
    if ((rc = dz_splitk_linear(lin, m->pooled, N, POOLED, POOLED_KPAD, EMB, FC_SPLIT, m->parts, 0, d_out, st))) return rc;
    if ((rc = dz_launch_nan_rows(d_out, N, EMB, geo.tooshort, st))) return rc;
    return normalize ? dz_launch_l2norm(d_out, N, EMB, 1.0f, st) : 0;
}

extern "C" int dz_sbx_forward(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks, int N,
                              int mask_frames, float* d_out, void* stream) {
    return dz_handle_forward("dz_sbx_forward", m, d_wave, wave_stride, d_masks, N, mask_frames, d_out, stream, sbx_run);
}

extern "C" int dz_sbx_forward_groups(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks,
                                     int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                                     void* stream) {
    return dz_handle_forward_groups("dz_sbx_forward_groups", m, d_wave, wave_stride, d_masks, n_groups, rows_per_group,
                                    mask_frames, normalize, d_out, stream, sbx_run);
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
