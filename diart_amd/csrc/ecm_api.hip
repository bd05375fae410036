// dz_ecm_*: launch sequence of the mel-spectrogram ECAPA-TDNN embedding (include/diart_amd.h).  Host
// code.  The mask compaction, the batch geometry and the NaN rules are ECAPA's (k_ecapa.hip) at hop 256; the front end
// is k_ecapa_mel.hip around two GEMM instances (the Hann-windowed DFT of 1024 taps at stride 256, the slaney mel
// bank); everything behind the features is DzEcapaTrunk::run (ecapa_api.hip), the function dz_ecapa runs.
#include "dz_embed.h"

namespace {

enum { HOP = 256, NFFT = 1024, LDS_SPEC = 1028, NSPEC = 1026, DFT_NPAD = 1152, LDM = 544, NMEL = 80, MEL_NPAD = 128,
       EMB = 192 };

}  // namespace

struct dz_ecm {
    dz_ctx* ctx;
    dz_ecm_weights w;
    int Nm;
    DzRowGeometry geo;      // sig: the compacted rows; lstride also strides csig
    char* arena;
    float *csig, *spec, *mag, *melp;
    int* lmax;
    DzEcapaTrunk tr;
    int lastN;
};

static void ecm_carve(dz_ecm* m, Arena& a) {
    const size_t N = m->Nm, NT = N * m->geo.Tc;
    m->csig = a.take<float>(N * m->geo.lstride);
    m->spec = a.take<float>(NT * LDS_SPEC);
    m->mag = a.take<float>(NT * LDM);
    m->melp = a.take<float>(NT * NMEL);
    m->lmax = a.take<int>(N);
    m->tr.carve(a, N, m->geo.Tc, m->w.net.mfa.wsplit != nullptr);
    m->geo.carve(a, N);
}

extern "C" int dz_ecm_abi_size(void) { return (int)sizeof(dz_ecm_weights); }

extern "C" int dz_ecm_frames_for(int num_samples) { return num_samples > 0 ? 1 + num_samples / HOP : 0; }

extern "C" int dz_ecm_create(dz_ctx* ctx, const dz_ecm_weights* w, int max_rows, int num_samples, dz_ecm** out) {
    DZ_REQUIRE(w, "dz_ecm_create: NULL argument");
    DZ_REQUIRE(w->min_num_samples > NFFT / 2, "dz_ecm_create: min_num_samples %d (the STFT's reflect padding needs > %d)",
               w->min_num_samples, NFFT / 2);
    return dz_handle_create("dz_ecm_create", ctx, w, max_rows, num_samples, w->min_num_samples, ecm_carve, out, HOP,
                            NFFT);
}

extern "C" int dz_ecm_destroy(dz_ecm* m) { return dz_handle_destroy(m); }

// The forward of G groups of K rows, each group with its own batch geometry, every row laid out with the handle's Tc
// frames.  Row g K + k reads waveform row (g K + k) / rows_per_wave and mask row g K + k (every sample when d_masks
// is NULL).
static int ecm_run(dz_ecm* m, const float* d_wave, long long wave_stride, const float* d_masks, int G, int K,
                   int rows_per_wave, int mask_frames, int normalize, float* d_out, hipStream_t st) {
    const dz_ecm_weights& w = m->w;
    DzRowGeometry& geo = m->geo;
    const int N = G * K, T = geo.Tc;
    const long long NT = (long long)N * T;
    int rc;
    // ---- 1. kept samples, the groups' geometry, the centre-padded rows --------------------------------------
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N);
      if ((rc = geo.prologue(d_wave, wave_stride, d_masks, mask_frames, G, K, rows_per_wave, st))) return rc; }
    m->lastN = N;
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N);
      if ((rc = dz_launch_ecm_prep(geo.sig, geo.lstride, geo.lens, N, K, m->csig, geo.lstride, m->lmax, st))) return rc; }
    // ---- 2. STFT as one GEMM over the overlapping rows (hop 256 < window 1024), |.|, mel GEMM, log / mean ----
    const dz_layer dft = {w.dft, w.net.zeros, nullptr, nullptr, w.dft_split};
    const dz_layer mel = {w.mel, w.net.zeros, nullptr, nullptr, nullptr};
    if ((rc = DzGemm::conv1d(dft, m->csig, HOP, N, T, NFFT, m->spec, LDS_SPEC, NSPEC, DZ_EPI_BIAS)
                  .xstride(geo.lstride, (long long)T * LDS_SPEC).padded(NFFT, DFT_NPAD).prof(DZ_T_ECAPA_FBANK, N).run(st)))
        return rc;
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N); if ((rc = dz_launch_ecm_magnitude(m->spec, NT, m->mag, st))) return rc; }
    if ((rc = DzGemm::dense(mel, m->mag, LDM, NT, LDM, m->melp, NMEL, NMEL, DZ_EPI_BIAS).padded(LDM, MEL_NPAD)
                  .prof(DZ_T_ECAPA_FBANK, N).run(st)))
        return rc;
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N);
      if ((rc = dz_launch_ecm_post(m->melp, T, N, geo.nvalid, m->tr.feats, st))) return rc; }
    // ---- 3. ECAPA-TDNN -----------------------------------------------------------------------------------------
    if ((rc = m->tr.run(w.net, N, T, geo.nmask, geo.tdev, d_out, st))) return rc;
    if ((rc = dz_launch_nan_rows(d_out, N, EMB, geo.tooshort, st))) return rc;
    return normalize ? dz_launch_l2norm(d_out, N, EMB, 1.0f, st) : 0;
}

extern "C" int dz_ecm_forward(dz_ecm* m, const float* d_wave, long long wave_stride, const float* d_masks, int N,
                              int mask_frames, float* d_out, void* stream) {
    return dz_handle_forward("dz_ecm_forward", m, d_wave, wave_stride, d_masks, N, mask_frames, d_out, stream, ecm_run);
}

extern "C" int dz_ecm_forward_groups(dz_ecm* m, const float* d_wave, long long wave_stride, const float* d_masks,
                                     int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                                     void* stream) {
    return dz_handle_forward_groups("dz_ecm_forward_groups", m, d_wave, wave_stride, d_masks, n_groups, rows_per_group,
                                    mask_frames, normalize, d_out, stream, ecm_run);
}

extern "C" int dz_ecm_peek(dz_ecm* m, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(m && d_ptr && count, "dz_ecm_peek: NULL argument");
    const long long N = m->lastN, NT = N * m->geo.Tc;
    if (frames) *frames = m->geo.Tc;
    switch (which) {
        case 0: *d_ptr = m->tr.feats; *count = NT * NMEL; return 0;
        case 1: *d_ptr = m->tr.b0; *count = NT * 1024; return 0;
        case 2: *d_ptr = m->tr.cat; *count = NT * 3072; return 0;   // holds the logits after a forward
        case 3: *d_ptr = m->tr.mfa; *count = NT * 3072; return 0;
        case 4: *d_ptr = m->tr.pooled; *count = N * 6144; return 0;
        case 5: *d_ptr = m->geo.lens; *count = N; return 0;
        case 6: *d_ptr = m->geo.rep_nvalid; *count = N; return 0;
        case 7: *d_ptr = m->geo.rep_nmask; *count = N; return 0;
        case 8: *d_ptr = m->geo.rep_T; *count = N; return 0;
        case 9: *d_ptr = m->lmax; *count = N; return 0;
        case 10: *d_ptr = m->mag; *count = NT * LDM; return 0;
    }
    dz_set_error("dz_ecm_peek: unknown buffer %d", which);
    return 2;
}
