// dz_ttn_*: launch sequence of the NeMo TitaNet-L embedding (include/diart_amd.h).  Host code.
// The mask compaction, the NaN rows, the attentive statistics pooling and the split-K tail are ECAPA's (k_ecapa.hip,
// ecapa_api.hip) at C = 3072; the front end, the depthwise convolutions and the squeeze-excitation are k_titanet.hip;
// the pointwise convolutions (BatchNorm folded) are descriptor instances of the wide GEMMs: k_gemm_pre.hip over the
// depthwise kernel's f16 planes ("f16x3"), k_gemm_f32.hip over its f32 rows ("f32").  A pointwise layer's ReLU is
// applied by the depthwise kernel that reads it.
#include "dz_embed.h"

int dz_launch_ttn_geometry(const int* lens, int G, int K, int Tc, int S, int min_samples, int fpad, int fnfft,
                           int* tooshort, int* elen, int* plen, int* frames, hipStream_t st);
int dz_launch_ttn_prep(const float* sig, long long stride, int rows, const int* elen, const int* plen, int reflect,
                       float* out, hipStream_t st);
int dz_launch_ttn_norm(const float* melp, int T, int rows, const int* frames, float* feats, hipStream_t st);
int dz_launch_ttn_depthwise(const float* x, int ldx, int Cin, const float* taps, int ktaps, const int* frames, int rows,
                            int T, int C, int relu, float* y, void* planes, long long plane, hipStream_t st);
int dz_launch_ttn_se_fc(const float* s, const float* w1, const float* w2t, int rows, int C, float* gate, hipStream_t st);
int dz_launch_ttn_apply(const float* y, const float* gate, const float* resid, float* out, void* planes,
                        long long plane, int rows, int T, int C, hipStream_t st);

namespace {

enum { HOP = 160, NWIN = 400, NBIN = 257, SPEC_LD = 516, PW_LD = 260, NMEL = 80, C0PAD = 96, C1 = 1024, C3 = 3072,
       EMB = 192, FC_SPLIT = 16, PLANE_SLACK = 16384, NBLOCK = 5 };
constexpr int kRepeats[NBLOCK] = {1, 3, 3, 3, 1}, kTaps[NBLOCK] = {3, 7, 11, 15, 1};

}  // namespace

struct dz_ttn {
    dz_ctx* ctx;
    dz_ttn_weights w;
    int Nm;
    DzRowGeometry geo;          // sig, lens, tooshort; init / carve only (the geometry itself is ttn_geometry's)
    char* arena;
    float* sig2;                // pre-emphasised, padded signal, laid out like geo.sig
    int *elen, *plen, *frames;
    float *spec, *pw, *melp, *feats, *dwf, *y[2], *resy, *blk[NBLOCK], *a1, *smean, *gate, *gstat, *rb, *pooled, *parts;
    unsigned short *dws, *blks;  // "f16x3": planes of the depthwise output and of the block output
    int lastN;
};

static void ttn_carve(dz_ttn* m, Arena& a) {
    const size_t N = m->Nm, NT = N * m->geo.Tc;
    m->sig2 = a.take<float>(N * m->geo.lstride);
    m->spec = a.take<float>(NT * SPEC_LD);
    m->pw = a.take<float>(NT * PW_LD);
    m->melp = a.take<float>(NT * NMEL);
    m->feats = a.take<float>(NT * NMEL);
    m->y[0] = a.take<float>(NT * C3);          // pointwise outputs, ping-pong; y[0] also block 4's and the logits
    m->y[1] = a.take<float>(NT * C1);
    m->resy = a.take<float>(NT * C1);
    for (int i = 0; i < NBLOCK; ++i) m->blk[i] = a.take<float>(NT * (i == 4 ? C3 : C1));
    m->a1 = a.take<float>(NT * 128);
    m->smean = a.take<float>(N * C3);
    m->gate = a.take<float>(N * C3);
    m->gstat = a.take<float>(N * 2 * C3);
    m->rb = a.take<float>(N * 128);
    m->pooled = a.take<float>(N * 2 * C3);
    m->parts = a.take<float>((size_t)FC_SPLIT * N * EMB);
    m->dwf = nullptr;
    m->dws = m->blks = nullptr;
    if (m->w.block[1].rep[0].pw.wsplit) {
        m->dws = a.take<unsigned short>(2 * NT * C1 + PLANE_SLACK);
        m->blks = a.take<unsigned short>(2 * NT * C1 + PLANE_SLACK);
    } else {
        m->dwf = a.take<float>(NT * C1);
    }
    m->elen = a.take<int>(N);
    m->plen = a.take<int>(N);
    m->frames = a.take<int>(N);
    m->geo.carve(a, N);
}

extern "C" int dz_ttn_abi_size(void) { return (int)sizeof(dz_ttn_weights); }
extern "C" int dz_ttn_frames_for(int num_samples) { return num_samples > 0 ? 1 + num_samples / HOP : 0; }

extern "C" int dz_ttn_create(dz_ctx* ctx, const dz_ttn_weights* w, int max_rows, int num_samples, dz_ttn** out) {
    DZ_REQUIRE(ctx && w && out, "dz_ttn_create: NULL argument");
    DZ_REQUIRE(w->min_num_samples > 200 && w->frame_pad >= 0 && w->frame_nfft >= 0,
               "dz_ttn_create: min_num_samples %d (> 200: the reflect padding reads 200 samples back), frame_pad %d, "
               "frame_nfft %d", w->min_num_samples, w->frame_pad, w->frame_nfft);
    DZ_REQUIRE((long long)max_rows * (1 + num_samples / HOP) * C3 * 2 < (1ll << 31),
               "dz_ttn_create: %d rows x %d frames exceed the GEMM operands' 2 GiB offset range", max_rows,
               1 + num_samples / HOP);
    return dz_handle_create("dz_ttn_create", ctx, w, max_rows, num_samples, w->min_num_samples, ttn_carve, out);
}

extern "C" int dz_ttn_destroy(dz_ttn* m) { return dz_handle_destroy(m); }

// a pointwise convolution with its BatchNorm folded: rows x Cin -> rows x Cout, + bias.  "f16x3": both operands as
// kb-major planes (k_gemm_pre.hip); "f32": f32 rows (k_gemm_f32.hip through dz_launch_convgemm)
static int ttn_pointwise(hipStream_t st, const float* Xf, const void* Xs, long long rows, int Cin, const dz_layer& L,
                         int Cout, float* Y) {
    return DzGemm::dense(L, Xf, Cin, rows, Cin, Y, Cout, Cout, DZ_EPI_BIAS).xplanes(Xs, rows * Cin).run(st);
}

// The forward of G groups of K rows, every row laid out with the handle's Tc frames.  Row g K + k reads waveform row
// (g K + k) / rows_per_wave and mask row g K + k (or every sample when d_masks is NULL).
static int ttn_run(dz_ttn* m, const float* d_wave, long long wave_stride, const float* d_masks, int G, int K,
                   int rows_per_wave, int mask_frames, int normalize, float* d_out, hipStream_t st) {
    const dz_ttn_weights& w = m->w;
    DzRowGeometry& geo = m->geo;
    const int N = G * K, T = geo.Tc;
    const long long NT = (long long)N * T;
    const bool pre = m->dws != nullptr;
    int rc;
    m->lastN = N;
    // ---- wrapper: mask -> kept samples; geometry; pre-emphasis + centre padding ------------------------------------
    DZ_HIP(hipMemsetAsync(geo.sig, 0, sizeof(float) * (size_t)N * geo.lstride, st));
    if ((rc = dz_launch_mask_compact(d_wave, wave_stride, geo.S, d_masks, mask_frames, N, geo.sig, geo.lstride, geo.lens,
                                     st, rows_per_wave)))
        return rc;
    if ((rc = dz_launch_ttn_geometry(geo.lens, G, K, T, geo.S, w.min_num_samples, w.frame_pad, w.frame_nfft, geo.tooshort,
                                     m->elen, m->plen, m->frames, st)))
        return rc;
    if ((rc = dz_launch_ttn_prep(geo.sig, geo.lstride, N, m->elen, m->plen, w.pad_reflect, m->sig2, st))) return rc;
    // ---- front end: STFT as one GEMM over the overlapping rows, |.|^2, mel GEMM, log + normalisation ---------------
    const dz_layer dft = {w.dft, w.zeros, nullptr, nullptr, w.dft_split};
    if ((rc = DzGemm::conv1d(dft, m->sig2, HOP, N, T, NWIN, m->spec, SPEC_LD, 2 * NBIN, DZ_EPI_BIAS)
                  .xstride(geo.lstride, (long long)T * SPEC_LD).padded(416, 640).run(st)))
        return rc;
    if ((rc = dz_launch_power(m->spec, SPEC_LD, 257, NT, m->pw, st))) return rc;
    const dz_layer mel = {w.mel, w.zeros, nullptr, nullptr, nullptr};
    if ((rc = DzGemm::dense(mel, m->pw, PW_LD, NT, PW_LD, m->melp, NMEL, NMEL, DZ_EPI_BIAS).padded(288, 128).run(st)))
        return rc;
    if ((rc = dz_launch_ttn_norm(m->melp, T, N, m->frames, m->feats, st))) return rc;
    // ---- encoder: five separable blocks -------------------------------------------------------------------------
    const float* xin = m->feats;
    int cin = NMEL, ldin = NMEL;
    for (int i = 0; i < NBLOCK; ++i) {
        const dz_ttn_block& b = w.block[i];
        const int R = kRepeats[i], cpad = i == 0 ? C0PAD : C1, cout = i == 4 ? C3 : C1;
        const float* src = xin;
        int csrc = cin, ldsrc = ldin;
        float* yl = nullptr;
        for (int j = 0; j < R; ++j) {
            if ((rc = dz_launch_ttn_depthwise(src, ldsrc, csrc, b.rep[j].dw, kTaps[i], m->frames, N, T, cpad, j > 0, m->dwf,
                                              m->dws, NT * cpad, st)))
                return rc;
            yl = m->y[j & 1];
            if ((rc = ttn_pointwise(st, m->dwf, m->dws, NT, cpad, b.rep[j].pw, cout, yl))) return rc;
            src = yl; csrc = ldsrc = cout;
        }
        // masked squeeze-excitation, residual, ReLU
        if ((rc = dz_launch_se_mean(yl, T, cout, cout, N, m->frames, m->smean, st))) return rc;
        if ((rc = dz_launch_ttn_se_fc(m->smean, b.se1, b.se2t, N, cout, m->gate, st))) return rc;
        const bool res = b.res.w != nullptr;
        if (res && (rc = ttn_pointwise(st, xin, pre ? m->blks : nullptr, NT, C1, b.res, C1, m->resy))) return rc;
        // (blocks 0 .. 2 feed a residual GEMM: their output also goes out as planes)
        if ((rc = dz_launch_ttn_apply(yl, m->gate, res ? m->resy : nullptr, m->blk[i], pre && i < 3 ? m->blks : nullptr,
                                      NT * C1, N, T, cout, st)))
            return rc;
        xin = m->blk[i];
        cin = ldin = cout;
    }
    // ---- decoder: attentive statistics pooling (ECAPA's form), BatchNorm + Conv1d(6144, 192) ------------------------
    // (the logits go where block 4's pointwise output is dead behind its apply pass)
    const dz_layer fc = {w.fc.w, w.fc.b, nullptr, nullptr, nullptr};
    const DzAspTail tail = {w.asp_wms, w.zeros, &w.asp_tdnn, &w.asp_conv, &fc, m->gstat, m->rb, m->a1, m->y[0], m->pooled,
                            m->parts, FC_SPLIT, -1, -1};
    if ((rc = dz_asp_tail(tail, m->blk[4], N, T, C3, EMB, m->frames, d_out, st))) return rc;
    if ((rc = dz_launch_nan_rows(d_out, N, EMB, geo.tooshort, st))) return rc;
    return normalize ? dz_launch_l2norm(d_out, N, EMB, 1.0f, st) : 0;
}

extern "C" int dz_ttn_forward(dz_ttn* m, const float* d_wave, long long wave_stride, const float* d_masks, int N,
                              int mask_frames, float* d_out, void* stream) {
    return dz_handle_forward("dz_ttn_forward", m, d_wave, wave_stride, d_masks, N, mask_frames, d_out, stream, ttn_run);
}

extern "C" int dz_ttn_forward_groups(dz_ttn* m, const float* d_wave, long long wave_stride, const float* d_masks,
                                     int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                                     void* stream) {
    return dz_handle_forward_groups("dz_ttn_forward_groups", m, d_wave, wave_stride, d_masks, n_groups, rows_per_group,
                                    mask_frames, normalize, d_out, stream, ttn_run);
}

extern "C" int dz_ttn_peek(dz_ttn* m, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(m && d_ptr && count, "dz_ttn_peek: NULL argument");
    const long long N = m->lastN, NT = N * m->geo.Tc;
    if (frames) *frames = m->geo.Tc;
    switch (which) {
        case 0: *d_ptr = m->feats; *count = NT * NMEL; return 0;
        case 1: case 2: case 3: case 4: *d_ptr = m->blk[which - 1]; *count = NT * C1; return 0;
        case 5: *d_ptr = m->blk[4]; *count = NT * C3; return 0;
        case 6: *d_ptr = m->pooled; *count = N * 2 * C3; return 0;
        case 7: *d_ptr = m->geo.lens; *count = N; return 0;
        case 8: *d_ptr = m->plen; *count = N; return 0;
        case 9: *d_ptr = m->frames; *count = N; return 0;
    }
    dz_set_error("dz_ttn_peek: unknown buffer %d", which);
    return 2;
}

extern "C" int dz_k_ttn_depthwise(dz_ctx* ctx, const float* d_x, int ldx, const float* d_taps, int taps,
                                  const int* d_frames, int rows, int T, int C, int relu, float* d_y, void* d_planes,
                                  void* stream) {
    DZ_REQUIRE(ctx != nullptr, "dz_k_ttn_depthwise: NULL context");
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_ttn_depthwise(d_x, ldx, C, d_taps, taps, d_frames, rows, T, C, relu, d_y, d_planes,
                                   (long long)rows * T * C, (hipStream_t)stream);
}
