// dz_ecapa_*: launch sequence of the ECAPA-TDNN embedding (include/diart_amd.h).  Host code.
#include "dz_embed.h"

#include <math.h>
#include <vector>

namespace {

enum { MIN_NUM_SAMPLES = 640, HOP = 160, NFFT = 400, C1 = 1024, C3 = 3072, EMB = 192, FC_SPLIT = 16, SE_SPLIT = 8,
       PLANE_SLACK = 16384 };

}  // namespace

struct dz_ecapa {
    dz_ctx* ctx;
    dz_ecapa_weights w;
    int Nm;
    DzRowGeometry geo;
    char* arena;
    int* h_pin;  // pinned host: lens[Nm] | nvalid[Nm] | nmask[Nm] | tooshort[Nm]
    // device buffers
    float *spec, *pw, *melp;
    DzEcapaTrunk tr;    // features and everything behind them (dz_embed.h)
    int lastN, lastT, lastGroups;
};

// DzRowGeometry (dz_common.h): ECAPA's STFT layout and batch geometry, which sbx_api.hip shares
void DzRowGeometry::init(int num_samples, int min_num_samples, int hop_, int window) {
    S = num_samples;
    hop = hop_;
    Tc = 1 + num_samples / hop;
    min_samples = min_num_samples;
    lstride = ((long long)num_samples + window + 3) / 4 * 4;
}

void DzRowGeometry::carve(Arena& a, size_t rows) {
    sig = a.take(rows * lstride);
    lens = a.take<int>(rows);
    nvalid = a.take<int>(rows);
    nmask = a.take<int>(rows);
    tooshort = a.take<int>(rows);
    tdev = a.take<int>(rows);
    rep_nvalid = a.take<int>(rows);
    rep_nmask = a.take<int>(rows);
    rep_T = a.take<int>(rows);
}

int DzRowGeometry::prologue(const float* d_wave, long long wave_stride, const float* d_masks, int mask_frames, int G,
                            int K, int rows_per_wave, hipStream_t st) {
    const int N = G * K;
    int rc;
    DZ_HIP(hipMemsetAsync(sig, 0, sizeof(float) * (size_t)N * lstride, st));
    if ((rc = dz_launch_mask_compact(d_wave, wave_stride, S, d_masks, mask_frames, N, sig, lstride, lens, st,
                                     rows_per_wave)))
        return rc;
    return dz_launch_ecapa_geometry(lens, G, K, Tc, min_samples, hop, nvalid, nmask, tooshort, tdev, rep_nvalid,
                                    rep_nmask, rep_T, st);
}

// DzEcapaTrunk (dz_embed.h): the buffers of ecapa_network's step 3 for N rows of Tc frames
void DzEcapaTrunk::carve(Arena& a, size_t N, size_t Tc, bool split) {
    const size_t NT = N * Tc;
    feats = a.take<float>(NT * 80);
    b0 = a.take<float>(NT * C1);
    t1 = a.take<float>(NT * C1);
    res = a.take<float>(NT * C1);
    t2 = a.take<float>(NT * C1);
    cat = a.take<float>(NT * C3);   // after the MFA convolution it is reused for the logits
    mfa = a.take<float>(NT * C3);
    a1 = a.take<float>(NT * 128);
    smean = a.take<float>(N * C1);
    sfc1 = a.take<float>(N * 128);
    gate = a.take<float>(N * C1);
    gstat = a.take<float>(N * 2 * C3);
    rb = a.take<float>(N * 128);
    pooled = a.take<float>(N * 2 * C3);
    parts = a.take<float>((size_t)FC_SPLIT * N * EMB);
    b0s = ress = cats = nullptr;
    if (split) {
        // (+ PLANE_SLACK: a 128-row tile that starts inside the last rows of a plane's last k-block reads up to 127
        // rows x 64 bytes past it — zeros through the buffer bounds check when the resource ends there, but a
        // consumer that reads a COLUMN SLICE of a plane (tdnn1 of blocks 1 and 2: k-blocks [32 (i - 1), 32 i) of
        // the concatenation) has a resource that ends further on, so the bytes must exist)
        b0s = a.take<unsigned short>(2 * NT * C1 + PLANE_SLACK);
        ress = a.take<unsigned short>(2 * NT * C1 + PLANE_SLACK);
        cats = a.take<unsigned short>(2 * NT * C3 + PLANE_SLACK);
    }
}

static void ecapa_carve(dz_ecapa* e, Arena& a) {
    const size_t N = e->Nm, NT = N * e->geo.Tc;
    e->spec = a.take<float>(NT * 404);
    e->pw = a.take<float>(NT * 204);
    e->melp = a.take<float>(NT * 80);
    e->tr.carve(a, N, e->geo.Tc, e->w.mfa.wsplit != nullptr);
    e->geo.carve(a, N);
}

extern "C" int dz_ecapa_frames_for(int num_samples) { return num_samples > 0 ? 1 + num_samples / HOP : 0; }

extern "C" int dz_ecapa_create(dz_ctx* ctx, const dz_ecapa_weights* w, int max_rows, int num_samples,
                               dz_ecapa** out) {
    dz_ecapa* e = nullptr;
    if (int rc = dz_handle_create("dz_ecapa_create", ctx, w, max_rows, num_samples, MIN_NUM_SAMPLES, ecapa_carve, &e))
        return rc;
    const hipError_t err = hipHostMalloc((void**)&e->h_pin, sizeof(int) * 4 * max_rows, hipHostMallocDefault);
    if (err != hipSuccess) {
        e->h_pin = nullptr;
        dz_set_error("dz_ecapa_create: hipHostMalloc failed: %s", hipGetErrorString(err));
        dz_ecapa_destroy(e);
        return 1;
    }
    *out = e;
    return 0;
}

extern "C" int dz_ecapa_destroy(dz_ecapa* e) {
    if (e && e->h_pin) (void)hipHostFree(e->h_pin);
    return dz_handle_destroy(e);
}

// a wide 1 x 1 layer (ReLU -> BN) over NT rows: both operands pre-split (k_gemm_pre.hip) when the producer wrote
// `planes` — the k-block of the layer's first input column inside kb-major planes of ldx columns (hi | lo, xplane
// apart) — else over the f32 rows X
static int wide(const dz_layer& L, const float* X, int ldx, const void* planes, long long xplane, int N, long long NT,
                int C, float* Y, hipStream_t st) {
    return DzGemm::dense(L, planes ? nullptr : X, ldx, NT, C, Y, C, C, DZ_EPI_RELU_BN).xplanes(planes, xplane)
        .prof(DZ_T_ECAPA_WIDE, N).run(st);
}

static int ecapa_network(dz_ecapa* e, int N, int T, const int* tdev, float* d_out, hipStream_t st);

extern "C" int dz_ecapa_forward(dz_ecapa* e, const float* d_wave, long long wave_stride,
                                const float* d_masks, int N, int mask_frames, float* d_out,
                                void* stream) {
    if (int rc = dz_check_rows_forward("dz_ecapa_forward", e, e ? e->Nm : 0, d_wave, wave_stride, d_masks, N,
                                       mask_frames, d_out))
        return rc;
    DZ_HIP(hipSetDevice(e->ctx->device));
    DzRangeScope range_scope(e->ctx->oflag_dev);
    hipStream_t st = (hipStream_t)stream;
    int rc;

    // ---- 1. mask -> kept samples, zero padded rows (200 leading zeros = centred STFT) ---------
    DZ_HIP(hipMemsetAsync(e->geo.sig, 0, sizeof(float) * (size_t)N * e->geo.lstride, st));
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N);
      if ((rc = dz_launch_mask_compact(d_wave, wave_stride, e->geo.S, d_masks, mask_frames, N, e->geo.sig,
                                       e->geo.lstride, e->geo.lens, st)))
          return rc; }
    int* h_lens = e->h_pin;
    int* h_nvalid = h_lens + e->Nm;
    int* h_nmask = h_nvalid + e->Nm;
    int* h_short = h_nmask + e->Nm;
    DZ_HIP(hipMemcpyAsync(h_lens, e->geo.lens, sizeof(int) * N, hipMemcpyDeviceToHost, st));
    DZ_HIP(hipStreamSynchronize(st));   // the batch geometry (frames) depends on the longest row
    // a row whose kept samples hold a NaN / Inf comes back as -(len + 1): it keeps its place in the batch geometry
    // (speechbrain pads and normalises by the longest row whatever its values) and its embedding is NaN — what the
    // reference computes for it, and what the split-f16 layers' clamps would otherwise turn into a finite vector
    std::vector<char> bad((size_t)N, 0);
    for (int i = 0; i < N; ++i)
        if (h_lens[i] < 0) { h_lens[i] = -h_lens[i] - 1; bad[i] = 1; }
    int lmax = 0;
    for (int i = 0; i < N; ++i) lmax = h_lens[i] > lmax ? h_lens[i] : lmax;
    e->lastN = N;
    e->lastGroups = 0;
    if (lmax < MIN_NUM_SAMPLES) {       // "every signal is too short": all NaN
        for (int i = 0; i < N; ++i) h_short[i] = 1;
        DZ_HIP(hipMemcpyAsync(e->geo.tooshort, h_short, sizeof(int) * N, hipMemcpyHostToDevice, st));
        DZ_HIP(hipMemsetAsync(e->geo.nvalid, 0, sizeof(int) * N, st));     // (no frames: what peek 6 / 7 report)
        DZ_HIP(hipMemsetAsync(e->geo.nmask, 0, sizeof(int) * N, st));
        e->lastT = 0;
        return dz_launch_nan_rows(d_out, N, EMB, e->geo.tooshort, st);
    }
    const int T = 1 + lmax / HOP;
    e->lastT = T;
    for (int i = 0; i < N; ++i) {
        const bool too_short = h_lens[i] < MIN_NUM_SAMPLES;
        h_short[i] = too_short || bad[i];       // (only dz_launch_nan_rows reads it)
        // float32 arithmetic of torch: wav_lens / max_len, then * T
        const float rel = too_short ? 1.0f : (float)h_lens[i] / (float)lmax;
        const float v = rel * (float)T;
        int nv = (int)nearbyintf(v);            // torch.round: half to even
        nv = nv < 1 ? 1 : (nv > T ? T : nv);
        h_nvalid[i] = nv;
        int nm = (int)ceilf(v);                 // #{t : (float)t < v}
        nm = nm < 1 ? 1 : (nm > T ? T : nm);
        h_nmask[i] = nm;
    }
    DZ_HIP(hipMemcpyAsync(e->geo.nvalid, h_nvalid, sizeof(int) * N, hipMemcpyHostToDevice, st));
    DZ_HIP(hipMemcpyAsync(e->geo.nmask, h_nmask, sizeof(int) * N, hipMemcpyHostToDevice, st));
    DZ_HIP(hipMemcpyAsync(e->geo.tooshort, h_short, sizeof(int) * N, hipMemcpyHostToDevice, st));
    if ((rc = ecapa_network(e, N, T, nullptr, d_out, st))) return rc;
    return dz_launch_nan_rows(d_out, N, EMB, e->geo.tooshort, st);
}

// Steps 2 - 3 of a forward (Fbank, ECAPA-TDNN, fc -> d_out, before the NaN rows) over the N rows of e->geo.sig
// laid out T frames apart, whose geometry (geo.nvalid, geo.nmask) is already on the device.  tdev: NULL (every row has
// T frames) or the device [N] frame count of each row (the groups forward: T = the handle's Tc; a row reflects
// and takes its top-dB maximum at its own count, and the frames past it are computed but read by no output).
static int ecapa_network(dz_ecapa* e, int N, int T, const int* tdev, float* d_out, hipStream_t st) {
    int rc;
    const dz_ecapa_weights& w = e->w;

    // ---- 2. Fbank: STFT as one GEMM over overlapping rows (hop 160 < window 400) ---------------
    const dz_layer dft = {w.dft, w.zeros, nullptr, nullptr, w.dft_split};
    const dz_layer mel = {w.mel, w.zeros, nullptr, nullptr, nullptr};
    if ((rc = dz_fbank_front(dft, mel, e->geo.sig, e->geo.lstride, N, T, e->spec, e->pw, 80, 128, e->melp, st,
                             DZ_T_ECAPA_FBANK)))
        return rc;
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N); if ((rc = dz_launch_fbank_post(e->melp, 80, T, N, e->geo.nvalid, e->tr.feats, st, tdev))) return rc; }

    return e->tr.run(w, N, T, e->geo.nmask, tdev, d_out, st);
}

// Step 3 of a forward, which the mel-spectrogram ECAPA (ecm_api.hip) shares: block 0 through dz_asp_tail over the
// features [N][T][80] of this trunk -> d_out [N][192].  nmask [N]: the frames of the squeeze-excitation means and the
// pooling; tdev as above.
int DzEcapaTrunk::run(const dz_ecapa_weights& w, int N, int T, const int* nmask, const int* tdev, float* d_out,
                      hipStream_t st) const {
    const DzEcapaTrunk* e = this;
    int rc;
    const long long NT = (long long)N * T;
    // ---- 3. ECAPA-TDNN -------------------------------------------------------------------------
    // Split-f16 precision: the seven wide 1 x 1 layers (tdnn1 / tdnn2 of the three blocks, the MFA convolution: 84 % of
    // the network's MACs) run on k_gemm_pre.hip — both operands as ready f16 planes moved by LDS-DMA — so whatever
    // produces their input (block 0, the Res2Net convolutions, the squeeze-excitation's gate + residual pass) also
    // writes it as kb-major planes of N T rows; the f32 copies stay for the consumers that are not GEMMs.
    const bool pre = e->b0s != nullptr;
    const long long p1 = NT * C1, p3 = NT * C3;          // elements between the hi and lo planes
    // block 0: Conv1d(80 -> 1024, k5) -> ReLU -> BN
    if ((rc = DzGemm::conv1d(w.block0, e->feats, 80, N, T, 80, e->b0, C1, C1, DZ_EPI_RELU_BN).taps(5, 1, 2).padded(416, C1)
                  .planes_out(pre ? e->b0s : nullptr, p1).tdev(tdev).prof(DZ_T_ECAPA_BLOCK0, N).run(st)))
        return rc;
    const int dil[3] = {2, 3, 4};
    for (int i = 0; i < 3; ++i) {
        const dz_seres2net& b = w.ser[i];
        const float* xin = i == 0 ? e->b0 : e->cat + (size_t)(i - 1) * C1;
        const int ldin = i == 0 ? C1 : C3;
        // tdnn1 (1x1): block 0 reads block0's planes, blocks 1 / 2 columns [1024 (i - 1), 1024 i) of the concatenation's
        if ((rc = wide(b.tdnn1, xin, ldin, pre ? (i == 0 ? e->b0s : e->cats + (size_t)(i - 1) * (C1 / 32) * NT * 32) : nullptr,
                       i == 0 ? p1 : p3, N, NT, C1, e->t1, st)))
            return rc;
        // Res2Net: y0 = x0; y1 = f1(x1); yi = fi(xi + y(i-1))
        if (pre) {      // (y0 is only read by tdnn2: planes alone)
            DzProfScope ps(DZ_T_ECAPA_RES2, N);
            if ((rc = dz_launch_se_apply_planes(e->t1, C1, nullptr, nullptr, 0, nullptr, 0, e->ress, p1, N, T, 128, st))) return rc;
        } else {
            DZ_HIP(hipMemcpy2DAsync(e->res, sizeof(float) * C1, e->t1, sizeof(float) * C1, sizeof(float) * 128,
                                    (size_t)NT, hipMemcpyDeviceToDevice, st));
        }
        for (int j = 1; j < 8; ++j) {
            const float* x2 = j >= 2 ? e->res + (j - 1) * 128 : nullptr;
            // (y7 has no f32 reader when tdnn2 takes the planes)
            if ((rc = DzGemm::conv1d(b.res[j - 1], e->t1 + j * 128, C1, N, T, 128, pre && j == 7 ? nullptr : e->res + j * 128,
                                     C1, 128, DZ_EPI_RELU_BN).taps(3, dil[i], dil[i]).padded(384, 128).x2(x2)
                          .planes_out(pre ? e->ress + (size_t)j * 4 * NT * 32 : nullptr, p1).tdev(tdev)
                          .prof(DZ_T_ECAPA_RES2, N).run(st)))
                return rc;
        }
        // tdnn2 (1x1)
        if ((rc = wide(b.tdnn2, e->res, C1, e->ress, p1, N, NT, C1, e->t2, st))) return rc;
        // squeeze-excitation + residual, written straight into its slice of the concatenation
        { DzProfScope ps(DZ_T_ECAPA_SE, N); if ((rc = dz_launch_se_mean(e->t2, T, C1, C1, N, nmask, e->smean, st))) return rc; }
        // squeeze (N rows x 1024 -> 128): one output tile, so the K loop is split 8 ways (a lone workgroup
        // walking 32 k-tiles took 90 us); the ReLU follows the fixed-order reduce
        if ((rc = dz_splitk_linear(b.se1, e->smean, N, C1, C1, 128, SE_SPLIT, e->parts, 2, e->sfc1, st, DZ_T_ECAPA_SE)))
            return rc;
        if ((rc = DzGemm::dense(b.se2, e->sfc1, 128, N, 128, e->gate, C1, C1, DZ_EPI_BIAS_SIGMOID).prof(DZ_T_ECAPA_SE, N)
                      .run(st)))
            return rc;
        { DzProfScope ps(DZ_T_ECAPA_SE, N);
          if (pre)      // f32 for the next block's residual (the last block has none), planes for its tdnn1 and the MFA convolution
              rc = dz_launch_se_apply_planes(e->t2, C1, e->gate, xin, ldin, i < 2 ? e->cat + (size_t)i * C1 : nullptr, C3,
                                             e->cats + (size_t)i * (C1 / 32) * NT * 32, p3, N, T, C1, st);
          else
              rc = dz_launch_se_apply(e->t2, C1, e->gate, xin, ldin, e->cat + (size_t)i * C1, C3, N, T, C1, st);
          if (rc) return rc; }
    }
    // multi-layer feature aggregation
    if ((rc = wide(w.mfa, e->cat, C3, e->cats, p3, N, NT, C3, e->mfa, st))) return rc;
    // attentive statistics pooling with global context, asp_bn (folded) + fc (dz_asp_tail); the logits go where the
    // concatenation is dead once the MFA layer has consumed it
    const DzAspTail tail = {w.asp_wms, w.zeros, &w.asp_tdnn, &w.asp_conv, &w.fc, e->gstat, e->rb, e->a1, e->cat, e->pooled,
                            e->parts, FC_SPLIT, DZ_T_ECAPA_ASP, DZ_T_ECAPA_FC};
    return dz_asp_tail(tail, e->mfa, N, T, C3, EMB, nmask, d_out, st);
}

// The forward of the rows of n_groups chunks, K (rows_per_group) speaker rows each, every group with its own
// batch geometry — what dz_ecapa_forward computes for that group's K rows alone — in one launch sequence with
// no host round trip: the geometry is derived on the device (dz_launch_ecapa_geometry) and every buffer is laid
// out with the handle's Tc frames per row.  Row g K + k reads waveform row g and mask row g K + k ((G, K, Fw)
// contiguous, the speaker-major OSP weights of dz_seg_forward_osp).
static int ecapa_run_groups(dz_ecapa* e, const float* d_wave, long long wave_stride, const float* d_masks, int G, int K,
                            int rows_per_wave, int mask_frames, int normalize, float* d_out, hipStream_t st) {
    const int N = G * K, Tc = e->geo.Tc;
    int rc;
    { DzProfScope ps(DZ_T_ECAPA_FBANK, N);
      if ((rc = e->geo.prologue(d_wave, wave_stride, d_masks, mask_frames, G, K, rows_per_wave, st))) return rc; }
    e->lastN = N;
    e->lastT = Tc;
    e->lastGroups = 1;
    if ((rc = ecapa_network(e, N, Tc, e->geo.tdev, d_out, st))) return rc;
    if ((rc = dz_launch_nan_rows(d_out, N, EMB, e->geo.tooshort, st))) return rc;
    return normalize ? dz_launch_l2norm(d_out, N, EMB, 1.0f, st) : 0;
}

extern "C" int dz_ecapa_forward_groups(dz_ecapa* e, const float* d_wave, long long wave_stride, const float* d_masks,
                                       int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                                       void* stream) {
    return dz_handle_forward_groups("dz_ecapa_forward_groups", e, d_wave, wave_stride, d_masks, n_groups, rows_per_group,
                                    mask_frames, normalize, d_out, stream, ecapa_run_groups);
}

extern "C" int dz_ecapa_peek(dz_ecapa* e, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(e && d_ptr && count, "dz_ecapa_peek: NULL argument");
    const long long N = e->lastN, T = e->lastT;
    if (frames) *frames = (int)T;
    if (e->lastGroups) {        // the geometry a groups forward reports (ecapa_geometry_kernel)
        switch (which) {
            case 6: *d_ptr = e->geo.rep_nvalid; *count = N; return 0;
            case 7: *d_ptr = e->geo.rep_nmask; *count = N; return 0;
            case 8: *d_ptr = e->geo.rep_T; *count = N; return 0;
        }
    } else if (which == 8) {
        dz_set_error("dz_ecapa_peek: buffer 8 (per-row frames) exists after dz_ecapa_forward_groups only");
        return 2;
    }
    switch (which) {
        case 0: *d_ptr = e->tr.feats; *count = N * T * 80; return 0;
        case 1: *d_ptr = e->tr.b0; *count = N * T * C1; return 0;
        case 2: *d_ptr = e->tr.cat; *count = N * T * C3; return 0;   // holds the logits after a forward
        case 3: *d_ptr = e->tr.mfa; *count = N * T * C3; return 0;
        case 4: *d_ptr = e->tr.pooled; *count = N * 2 * C3; return 0;
        case 5: *d_ptr = e->geo.lens; *count = N; return 0;
        case 6: *d_ptr = e->geo.nvalid; *count = N; return 0;
        case 7: *d_ptr = e->geo.nmask; *count = N; return 0;
    }
    dz_set_error("dz_ecapa_peek: unknown buffer %d", which);
    return 2;
}
