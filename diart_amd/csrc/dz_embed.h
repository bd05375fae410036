// The launch vocabulary of the handles (seg_api.hip, xvec_api.hip, ecapa_api.hip, ecm_api.hip, sbx_api.hip,
// sbr_api.hip, titanet_api.hip, wespeaker_api.hip): one builder for the GEMM descriptor, the launch sequences two
// models share, and the entry points of a handle that owns a DzRowGeometry and one arena.  Host code only.
#pragma once
#include "dz_common.h"

#include <string.h>
#include <new>

// ---------------------------------------------------------------------------
// DzGemm: a DzConvGemm filled by name.  Two constructors give the geometry, chained setters the rare fields, run()
// picks the kernel:
//   pre-split activations (xplanes)              -> k_gemm_pre.hip (run_pooled(): its pooled-epilogue launch)
//   a layer with row-major planes, no split-K,
//     the POOL3 epilogue (SincNet stages 1 / 2)  -> k_conv_pool.hip with the weights' fragment copy (wfrag);
//                                                   DZ_CONV_POOL=0 (experiments): k_gemm_split.hip, Npad as given
//     any other epilogue                         -> k_gemm_split.hip, Npad rounded up to the planes' 128 rows
//   everything else                              -> k_convgemm.hip / k_gemm_f32.hip (exact f32)
// Kpad / Npad default to Cin / Nstore (an unpadded 1 x 1 layer); padded() names the packed sizes otherwise.
// ---------------------------------------------------------------------------
inline bool dz_conv_pool_enabled() {
    const char* v = dz_exp_env("DZ_CONV_POOL");
    return !(v && v[0] == '0');
}

struct DzGemm {
    DzConvGemm p;
    const void *wsplit, *wfrag;
    int tag, units;

    // rows x Cin (ldx floats apart) -> rows x Nstore (ldy apart): one flat batch
    static DzGemm dense(const dz_layer& L, const float* X, int ldx, long long rows, int Cin, float* Y, int ldy,
                        int Nstore, int epi) {
        return conv1d(L, X, ldx, 1, (int)rows, Cin, Y, ldy, Nstore, epi).xstride(0, 0);
    }
    // B items of T frames, ldx / ldy floats per frame and T frames per item; taps() makes it a convolution
    static DzGemm conv1d(const dz_layer& L, const float* X, int ldx, int B, int T, int Cin, float* Y, int ldy,
                         int Nstore, int epi) {
        DzGemm g;
        memset(&g, 0, sizeof(g));
        g.wsplit = L.wsplit;
        g.tag = -1;
        DzConvGemm& p = g.p;
        p.X = X; p.W = L.w; p.bias = L.b; p.e0 = L.s; p.e1 = L.h; p.Y = Y;
        p.B = B; p.Tin = p.Tout = p.Tstore = T; p.Cin = Cin; p.taps = 1; p.dil = 1; p.K = p.Kpad = Cin;
        p.Npad = p.Nstore = Nstore; p.ldx = ldx; p.ldy = ldy; p.epi = epi;
        return g.xstride((long long)T * ldx, (long long)T * ldy);
    }
    // floats between two items of X and of Y (the STFT reads overlapping rows: ldx = hop)
    DzGemm& xstride(long long xbs, long long ybs) { p.xbs = xbs; p.ybs = ybs; return *this; }
    // pad > 0: "same" convolution with reflect padding; 0: valid
    DzGemm& taps(int n, int dil, int pad) {
        p.taps = n; p.dil = dil; p.pad = pad; p.K = n * p.Cin;
        p.Tout = p.Tstore = pad ? p.Tin : p.Tin - (n - 1) * dil;
        return *this;
    }
    DzGemm& padded(int Kpad, int Npad) { p.Kpad = Kpad; p.Npad = Npad; return *this; }
    DzGemm& x2(const float* X2) { p.X2 = X2; return *this; }
    DzGemm& rowbias(const float* rb) { p.rowbias = rb; return *this; }
    DzGemm& splitk(int n, long long ysplit) { p.ksplit = n; p.ysplit = ysplit; return *this; }
    // the input as kb-major f16 planes of ldx columns (hi | lo, xplane elements apart), X is then not read; NULL: no-op
    DzGemm& xplanes(const void* Xs, long long xplane) { p.Xsplit = Xs; p.xplane = Xs ? xplane : 0; return *this; }
    // the output also as kb-major planes, for the next wide layer (split-f16 kernels only); NULL: no-op
    DzGemm& planes_out(void* Ys, long long yplane) { p.Ysplit = Ys; p.yplane = Ys ? yplane : 0; return *this; }
    // InstanceNorm + LeakyReLU of the nld input channels as they are loaded: scale / shift derived by the kernel from the
    // producer's tile partials [B][tiles][nld][2] over T values per channel (split-f16 kernels only) ...
    DzGemm& norm_partials(const float* part, int tiles, int T, const float* gamma, const float* beta, int nld) {
        p.npart = part; p.npart_tiles = tiles; p.npart_T = T; p.ngamma = gamma; p.nbeta = beta;
        p.nld = nld; p.norm_on_load = 1;
        return *this;
    }
    // ... or finalized by dz_launch_finalize_norm: nscale / nshift [B][nld]
    DzGemm& norm_scaled(const float* nscale, const float* nshift, int nld) {
        p.nscale = nscale; p.nshift = nshift; p.nld = nld; p.norm_on_load = 1;
        return *this;
    }
    // the DZ_EPI_POOL3 epilogue (after taps()): MaxPool1d(3) of the output frames, Tout / 3 of them stored per item, and
    // the tile partials [B][ntile][Npad][2] of the pooled rows for the next layer's norm
    DzGemm& pool3(float* partials) {
        p.partials = partials; p.Tstore = p.Tout / 3; p.ybs = (long long)p.Tstore * p.ldy;
        return *this;
    }
    // the layer's planes in conv_pool_h's fragment order (dz_launch_conv_pool_wfrag)
    DzGemm& frag(const void* f) { wfrag = f; return *this; }
    DzGemm& tdev(const int* T) { p.Tdev = T; return *this; }
    DzGemm& prof(int t, int u) { tag = t; units = u; return *this; }

    int run(hipStream_t st) {
        DzProfScope ps(tag, units);     // (no tag: no bracket)
        if (p.Xsplit) {
            p.X = p.W = nullptr;        // (both operands are the planes)
            p.Wsplit = wsplit;
            return dz_launch_gemm_pre(p, st);
        }
        if (wsplit && p.ksplit <= 1) {
            p.Wsplit = wsplit;
            if (p.epi == DZ_EPI_POOL3)      // (k_gemm_split.hip takes POOL3 with Npad == 64 only: no rounding)
                return dz_conv_pool_enabled() ? dz_launch_conv_pool(p, st, wfrag) : dz_launch_gemm_split(p, st);
            p.Npad = (p.Npad + 127) / 128 * 128;       // (the DFT's planes are packed with 512 rows)
            return dz_launch_gemm_split(p, st);
        }
        DZ_REQUIRE(p.Ysplit == nullptr, "DzGemm: plane output asked of a layer that is not on the split-f16 path");
        return dz_launch_convgemm(p, st);
    }
    // the pre-split route with the x-vector's statistics pooling in the epilogue: pieces into q instead of an output
    int run_pooled(const DzPoolFuse& q, hipStream_t st) {
        DzProfScope ps(tag, units);
        p.X = p.W = nullptr;
        p.Wsplit = wsplit;
        return dz_launch_gemm_pre_pool(p, q, st);
    }
};

// ---------------------------------------------------------------------------
// launch sequences that more than one model runs.  `tag` (-1: none): the DzProfScope tag of every launch.
// ---------------------------------------------------------------------------
// Linear(Cin -> N) over `rows` rows with the K loop split nsplit ways into parts [nsplit][rows][N], then the
// fixed-order reduce into out (finish: dz_launch_splitk_finish's mode — 0 plain, 1 L2-normalised, 2 ReLU).  wave_mom /
// rows_per_x: the finish writes NaN rows for the chunks (rows_per_x rows each) whose wave moments are not finite; the
// brackets count chunks.  finish_tag: the finish launch's own tag (default: the GEMM's).
constexpr int DZ_TAG_OF_GEMM = -2;
inline int dz_splitk_linear(const dz_layer& L, const float* X, int rows, int Cin, int Kpad, int N, int nsplit,
                            float* parts, int finish, float* out, hipStream_t st, int tag = -1,
                            int finish_tag = DZ_TAG_OF_GEMM, const float* wave_mom = nullptr, int rows_per_x = 1) {
    const long long ysplit = (long long)rows * N;
    if (int rc = DzGemm::dense(L, X, Cin, rows, Cin, parts, N, N, DZ_EPI_BIAS).padded(Kpad, N).splitk(nsplit, ysplit)
                     .prof(tag, rows / rows_per_x).run(st))
        return rc;
    DzProfScope ps(finish_tag == DZ_TAG_OF_GEMM ? tag : finish_tag, rows / rows_per_x);
    return dz_launch_splitk_finish(parts, nsplit, ysplit, rows, N, finish, out, st, wave_mom, rows_per_x);
}

// speechbrain Fbank up to the mel energies: the STFT of N rows of `sig` (lstride apart, hop 160, window 400) as one
// GEMM over the overlapping rows -> spec [N T][404], |.|^2 -> pw [N T][204], mel GEMM -> melp [N T][nmel].  The
// dB / normalisation pass that follows is each model's own.
inline int dz_fbank_front(const dz_layer& dft, const dz_layer& mel, const float* sig, long long lstride, int N, int T,
                          float* spec, float* pw, int nmel, int mel_npad, float* melp, hipStream_t st, int tag = -1) {
    const long long NT = (long long)N * T;
    int rc;
    if ((rc = DzGemm::conv1d(dft, sig, 160, N, T, 400, spec, 404, 402, DZ_EPI_BIAS).xstride(lstride, (long long)T * 404)
                  .padded(416, 448).prof(tag, N).run(st)))
        return rc;
    { DzProfScope ps(tag, N); if ((rc = dz_launch_power(spec, 404, 201, NT, pw, st))) return rc; }
    return DzGemm::dense(mel, pw, 204, NT, 204, melp, nmel, nmel, DZ_EPI_BIAS).padded(224, mel_npad).prof(tag, N).run(st);
}

// Attentive statistics pooling with global context over x [N][T][C] and the final Linear(2 C -> emb), ECAPA-TDNN's
// and TitaNet's: W [x; mean; std] = Wx x + Wms [mean; std], the second term a per-row bias.  frames [N]: the frames
// each row pools over; gstat / pooled [N][2 C], rb [N][128], a1 [N T][128], logits [N T][C], parts [nsplit][N][emb]
// (>= 128 wide); out [N][emb].
struct DzAspTail {
    const float *wms, *zeros;               // [128][2 C] and a zero bias
    const dz_layer *tdnn, *conv, *fc;
    float *gstat, *rb, *a1, *logits, *pooled, *parts;
    int nsplit, tag_asp, tag_fc;
};
inline int dz_asp_tail(const DzAspTail& a, const float* x, int N, int T, int C, int emb, const int* frames, float* out,
                       hipStream_t st) {
    int rc;
    { DzProfScope ps(a.tag_asp, N); if ((rc = dz_launch_asp_gstats(x, T, C, N, frames, a.gstat, st))) return rc; }
    // (N rows x 2 C -> 128: one output tile and 192 k-tiles — 0.5 ms for a lone workgroup; split-K like fc)
    const dz_layer wms = {a.wms, a.zeros, nullptr, nullptr, nullptr};
    if ((rc = dz_splitk_linear(wms, a.gstat, N, 2 * C, 2 * C, 128, a.nsplit, a.parts, 0, a.rb, st, a.tag_asp))) return rc;
    if ((rc = DzGemm::conv1d(*a.tdnn, x, C, N, T, C, a.a1, 128, 128, DZ_EPI_RELU_BN_TANH).rowbias(a.rb)
                  .prof(a.tag_asp, N).run(st)))
        return rc;
    if ((rc = DzGemm::dense(*a.conv, a.a1, 128, (long long)N * T, 128, a.logits, C, C, DZ_EPI_BIAS).prof(a.tag_asp, N)
                  .run(st)))
        return rc;
    { DzProfScope ps(a.tag_asp, N); if ((rc = dz_launch_asp_pool(x, a.logits, T, C, N, frames, a.pooled, st))) return rc; }
    // the pooled statistics' BatchNorm is folded into fc; split-K with a fixed-order reduce
    return dz_splitk_linear(*a.fc, a.pooled, N, 2 * C, 2 * C, emb, a.nsplit, a.parts, 0, out, st, a.tag_fc);
}

// The buffers and the launch sequence of ECAPA-TDNN behind its features (ecapa_api.hip), for the two handles with that
// network: dz_ecapa (Fbank front end) and dz_ecm (mel-spectrogram front end, ecm_api.hip).
struct DzEcapaTrunk {
    float *feats, *b0, *t1, *res, *t2, *cat, *mfa, *a1;
    float *smean, *sfc1, *gate, *gstat, *rb, *pooled, *parts;
    // split-f16 precision: the inputs of the wide 1 x 1 layers as kb-major f16 planes (k_gemm_pre.hip), [2][C / 32][N T][32]
    unsigned short *b0s, *ress, *cats;
    void carve(Arena& a, size_t N, size_t Tc, bool split);
    int run(const dz_ecapa_weights& w, int N, int T, const int* nmask, const int* tdev, float* d_out,
            hipStream_t st) const;
};

// ---------------------------------------------------------------------------
// entry points of a handle H {dz_ctx* ctx; W w; int Nm; DzRowGeometry geo; char* arena; ...} (dz_sbx, dz_sbr,
// dz_ttn, dz_ecapa, dz_ecm).  `who`: the public function, for the error strings.
// ---------------------------------------------------------------------------
template <typename H>
int dz_handle_destroy(H* h) {
    if (h) {
        if (h->arena) (void)hipFree(h->arena);
        delete h;
    }
    return 0;
}
template <typename H, typename W>
int dz_handle_create(const char* who, dz_ctx* ctx, const W* w, int max_rows, int num_samples, int min_samples,
                     void (*carve)(H*, Arena&), H** out, int hop = 160, int window = 400) {
    DZ_REQUIRE(ctx && w && out, "%s: NULL argument", who);
    DZ_REQUIRE(max_rows >= 1 && num_samples >= min_samples, "%s: max_rows %d, %d samples", who, max_rows, num_samples);
    DZ_HIP(hipSetDevice(ctx->device));
    H* h = new (std::nothrow) H;
    DZ_REQUIRE(h != nullptr, "%s: out of memory", who);
    memset(h, 0, sizeof(*h));
    h->ctx = ctx; h->w = *w; h->Nm = max_rows;
    h->geo.init(num_samples, min_samples, hop, window);
    if (int rc = dz_arena_alloc(who, h, carve)) {
        dz_handle_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}
// run(h, d_wave, wave_stride, d_masks, G, K, rows_per_wave, mask_frames, normalize, d_out, stream): the forward of G
// groups of K rows.  The rows form is one group whose rows each read a waveform row of their own.
template <typename H, typename Run>
int dz_handle_forward(const char* who, H* h, const float* d_wave, long long wave_stride, const float* d_masks, int N,
                      int mask_frames, float* d_out, void* stream, Run run) {
    if (int rc = dz_check_rows_forward(who, h, h ? h->Nm : 0, d_wave, wave_stride, d_masks, N, mask_frames, d_out))
        return rc;
    DZ_HIP(hipSetDevice(h->ctx->device));
    DzRangeScope range_scope(h->ctx->oflag_dev);
    return run(h, d_wave, wave_stride, d_masks, 1, N, 1, mask_frames, 0, d_out, (hipStream_t)stream);
}
template <typename H, typename Run>
int dz_handle_forward_groups(const char* who, H* h, const float* d_wave, long long wave_stride, const float* d_masks,
                             int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                             void* stream, Run run) {
    if (int rc = dz_check_groups_forward(who, h, h ? h->Nm : 0, d_wave, wave_stride, d_masks, n_groups, rows_per_group,
                                         mask_frames, d_out))
        return rc;
    DZ_HIP(hipSetDevice(h->ctx->device));
    DzRangeScope range_scope(h->ctx->oflag_dev);
    return run(h, d_wave, wave_stride, d_masks, n_groups, rows_per_group, rows_per_group, mask_frames, normalize, d_out,
               (hipStream_t)stream);
}
