// dz_sbr_*: launch sequence of the speechbrain ResNet embedding (include/diart_amd.h).  Host code.
// Fbank, the batch geometry and the NaN rules are ECAPA's (k_ecapa.hip, ecapa_api.hip).  The trunk is a 2-D ResNet of
// squeeze-excitation blocks on k_conv2d.hip's masked instances: a group's batch is padded to its own T_g frames, and
// the network sees every frame of that batch, so each row carries its live steps per layer (ext) and every kernel
// keeps zeros behind them.  The trunk runs in passes of at most rows_per_pass rows over one arena; every kernel
// computes a row from that row alone, so the passes do not show in the result.  Per pass row the arena holds the stem's
// output and three buffers per layer (the first convolution's output and two block outputs that alternate), so every
// layer's output outlives the pass (dz_sbr_peek): 109 MB per row for 5 s at 128 / 128 / 256 / 256 channels.
#include "dz_embed.h"

namespace {

enum { NMEL = 80, ATT = 128, EMB = 256, FC_SPLIT = 16, DEFAULT_ROWS_PER_PASS = 16 };

int down(int n, int stride) { return (n - 1) / stride + 1; }

}  // namespace

struct dz_sbr {
    dz_ctx* ctx;
    dz_sbr_weights w;
    int Nm;
    DzRowGeometry geo;
    char* arena;
    int P;                      // rows per pass
    int stride[4];              // of the four layers
    int T[5], F[5], C[5];       // steps per row in the buffers, frequency bins and channels: the stem, layers 1 .. 4
    float *spec, *pw, *melp, *feats, *stem, *R[4][3], *separt, *gate, *a1, *logits, *pooled, *parts;
    const float* L[5];          // where the last pass left the stem's and the layers' outputs
    int* ext;                   // [5][N] of the last forward
    int lastN, lastPass;
};

// the geometry the weights describe; false (with the error set) when they describe none
static bool sbr_shape(dz_sbr* m) {
    const dz_sbr_weights& w = m->w;
    if (w.n_blocks < 4 || w.n_blocks > DZ_SBR_MAX_BLOCKS || w.stem_width < 32) {
        dz_set_error("dz_sbr_create: %d blocks, stem width %d", w.n_blocks, w.stem_width);
        return false;
    }
    m->T[0] = m->geo.Tc; m->F[0] = NMEL; m->C[0] = w.stem_width;
    int T = m->T[0], F = NMEL, C = w.stem_width, layer = -1;
    for (int i = 0; i < w.n_blocks; ++i) {
        const dz_sbr_block& b = w.block[i];
        const bool first = b.layer == layer + 1;
        if ((!first && b.layer != layer) || b.layer > 3 || (i == 0 && !first) || b.width < 32 || b.width > 1024 ||
            b.se_width < 1 || b.se_width > 1024 || (b.stride != 1 && b.stride != 2) ||
            (!first && (b.stride != 1 || b.width != C))) {
            dz_set_error("dz_sbr_create: block %d (layer %d, width %d, stride %d) does not continue the trunk", i, b.layer,
                         b.width, b.stride);
            return false;
        }
        if (!b.conv[0].w || !b.conv[0].b || !b.conv[1].w || !b.conv[1].b || !b.se_w1t || !b.se_b1 || !b.se_w2t || !b.se_b2 ||
            (!b.conv[2].w && (b.stride != 1 || b.width != C))) {
            dz_set_error("dz_sbr_create: block %d has missing weights", i);
            return false;
        }
        if (first) m->stride[b.layer] = b.stride;
        layer = b.layer;
        T = down(T, b.stride); F = down(F, b.stride); C = b.width;
        m->T[layer + 1] = T; m->F[layer + 1] = F; m->C[layer + 1] = C;
    }
    if (layer != 3) {
        dz_set_error("dz_sbr_create: the blocks end at layer %d of 4", layer + 1);
        return false;
    }
    return true;
}

static void sbr_carve(dz_sbr* m, Arena& a) {
    const size_t N = m->Nm, NT = N * m->geo.Tc, P = m->P;
    const size_t CF = (size_t)m->F[4] * m->C[4], CFpad = (CF + 127) / 128 * 128;
    m->spec = a.take<float>(NT * 404);
    m->pw = a.take<float>(NT * 204);
    m->melp = a.take<float>(NT * NMEL);
    m->feats = a.take<float>(NT * NMEL);
    m->stem = a.take<float>(P * m->T[0] * m->F[0] * m->C[0]);
    for (int l = 0; l < 4; ++l)
        for (int i = 0; i < 3; ++i) m->R[l][i] = a.take<float>(P * m->T[l + 1] * m->F[l + 1] * m->C[l + 1]);
    m->separt = a.take<float>(P * DZ_SBR_SE_SLICES * 1024);
    m->gate = a.take<float>(P * 1024);
    m->a1 = a.take<float>(P * m->T[4] * ATT);
    m->logits = a.take<float>(P * m->T[4] * CFpad);
    m->pooled = a.take<float>(N * 2 * CF);
    m->parts = a.take<float>((size_t)FC_SPLIT * N * EMB);
    m->ext = a.take<int>(5 * N);
    m->geo.carve(a, N);
}

extern "C" int dz_sbr_abi_size(void) { return (int)sizeof(dz_sbr_weights); }

extern "C" int dz_sbr_create(dz_ctx* ctx, const dz_sbr_weights* w, int max_rows, int num_samples, dz_sbr** out) {
    DZ_REQUIRE(ctx && w && out, "dz_sbr_create: NULL argument");
    DZ_REQUIRE(w->min_num_samples >= 1 && w->rows_per_pass >= 0, "dz_sbr_create: min_num_samples %d, rows_per_pass %d",
               w->min_num_samples, w->rows_per_pass);
    DZ_REQUIRE(w->dft && w->mel && w->stem_w && w->stem_b && w->att1.w && w->att1.b && w->att1.s && w->att1.h &&
                   w->att2.w && w->att2.b && w->fc.w && w->fc.b && w->zeros,
               "dz_sbr_create: missing weights");
    DZ_REQUIRE(max_rows >= 1 && num_samples >= w->min_num_samples, "dz_sbr_create: max_rows %d, %d samples", max_rows,
               num_samples);
    DZ_HIP(hipSetDevice(ctx->device));
    dz_sbr* m = new (std::nothrow) dz_sbr;
    DZ_REQUIRE(m != nullptr, "dz_sbr_create: out of memory");
    memset(m, 0, sizeof(*m));
    m->ctx = ctx; m->w = *w; m->Nm = max_rows;
    m->P = w->rows_per_pass ? w->rows_per_pass : DEFAULT_ROWS_PER_PASS;
    if (m->P > max_rows) m->P = max_rows;
    m->geo.init(num_samples, w->min_num_samples);
    if (!sbr_shape(m)) {
        dz_sbr_destroy(m);
        return 2;
    }
    if (int rc = dz_arena_alloc("dz_sbr_create", m, sbr_carve)) {
        dz_sbr_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

extern "C" int dz_sbr_destroy(dz_sbr* m) { return dz_handle_destroy(m); }

static int sbr_conv(const dz_wsp_conv& c, const float* X, int n, int Ti, int Fi, int Cin, int Cout, int taps, int stride,
                    int relu, const int* ext_out, float* Y, hipStream_t st) {
    // (time in DzConv2d's F slot, the slow spatial axis; frequency in its T slot)
    return dz_launch_conv2d(dz_conv2d(c.w, c.wsplit, c.b, X, n, Ti, Fi, Cin, Cout, taps, stride, nullptr, relu, ext_out, Y),
                            st);
}

// the stem, the four layers and the attention pooling of rows [r0, r0 + n) -> pooled rows [r0, r0 + n)
static int sbr_pass(dz_sbr* m, int r0, int n, int N, hipStream_t st) {
    const dz_sbr_weights& w = m->w;
    int rc;
    const int* ext = m->ext + r0;        // + l N: the rows' live steps after layer l
    int T = m->T[0], F = NMEL, C = w.stem_width;
    if ((rc = dz_launch_sbr_stem(m->feats + (size_t)r0 * T * NMEL, n, T, NMEL, C, w.stem_w, w.stem_b, ext, m->stem, st)))
        return rc;
    const float* x = m->L[0] = m->stem;
    for (int i = 0, j = 0; i < w.n_blocks; ++i, ++j) {
        const dz_sbr_block& b = w.block[i];
        if (i && b.layer != w.block[i - 1].layer) j = 0;        // j: the block's place in its layer
        const int To = down(T, b.stride), Fo = down(F, b.stride), Co = b.width;
        const int* eo = ext + (size_t)(b.layer + 1) * N;
        float* const* R = m->R[b.layer];
        float* mid = R[0];
        float* y = R[1 + (j & 1)];
        if ((rc = sbr_conv(b.conv[0], x, n, T, F, C, Co, 9, b.stride, 1, eo, mid, st))) return rc;
        const float* r = x;
        if (b.conv[2].w) {
            // (a layer's first block only: the buffer its second block's output goes to is still free)
            if ((rc = sbr_conv(b.conv[2], x, n, T, F, C, Co, 1, b.stride, 0, eo, R[2], st))) return rc;
            r = R[2];
        }
        if ((rc = sbr_conv(b.conv[1], mid, n, To, Fo, Co, Co, 9, 1, 0, eo, y, st))) return rc;
        if ((rc = dz_launch_sbr_se_sum(y, n, To, Fo, Co, eo, m->separt, st))) return rc;
        if ((rc = dz_launch_sbr_se_fc(m->separt, n, Fo, Co, b.se_width, eo, b.se_w1t, b.se_b1, b.se_w2t, b.se_b2, m->gate,
                                      st)))
            return rc;
        if ((rc = dz_launch_sbr_se_apply(y, m->gate, r, n, To, Fo, Co, eo, y, st))) return rc;
        T = To; F = Fo; C = Co;
        x = m->L[b.layer + 1] = y;
    }
    // attention over the F4 C4 channels of each frame: Conv1d(1x1) -> ReLU -> BatchNorm -> Conv1d(1x1) -> softmax
    // over the row's own frames; the dead frames' logits are computed and read by nobody
    const int CF = F * C, CFpad = (CF + 127) / 128 * 128;
    const float* x4 = x;
    const long long rows = (long long)n * T;
    if ((rc = DzGemm::dense(w.att1, x4, CF, rows, CF, m->a1, ATT, ATT, DZ_EPI_RELU_BN).run(st))) return rc;
    if ((rc = DzGemm::dense(w.att2, m->a1, ATT, rows, ATT, m->logits, CF, CF, DZ_EPI_BIAS).padded(ATT, CFpad).run(st)))
        return rc;
    return dz_launch_sbr_att_pool(x4, m->logits, CF, n, T, CF, ext + (size_t)4 * N, m->pooled + (size_t)r0 * 2 * CF, st);
}

static int sbr_run(dz_sbr* m, const float* d_wave, long long wave_stride, const float* d_masks, int G, int K,
                   int rows_per_wave, int mask_frames, int normalize, float* d_out, hipStream_t st) {
    const dz_sbr_weights& w = m->w;
    DzRowGeometry& geo = m->geo;
    const int N = G * K, T = geo.Tc;
    int rc;
    if ((rc = geo.prologue(d_wave, wave_stride, d_masks, mask_frames, G, K, rows_per_wave, st))) return rc;
    m->lastN = N;
    if ((rc = dz_launch_sbr_extents(geo.tdev, N, m->stride[0], m->stride[1], m->stride[2], m->stride[3], m->ext, st)))
        return rc;
    // ---- Fbank(n_mels = 80) and the sentence mean over round(rel T) frames: ECAPA's front end ------------------------
    const dz_layer dft = {w.dft, w.zeros, nullptr, nullptr, w.dft_split};
    const dz_layer mel = {w.mel, w.zeros, nullptr, nullptr, nullptr};
    if ((rc = dz_fbank_front(dft, mel, geo.sig, geo.lstride, N, T, m->spec, m->pw, NMEL, 128, m->melp, st))) return rc;
    if ((rc = dz_launch_fbank_post(m->melp, NMEL, T, N, geo.nvalid, m->feats, st, geo.tdev))) return rc;
    // ---- the trunk and the pooling, rows_per_pass rows at a time ---------------------------------------------------------
    for (int r0 = 0; r0 < N; r0 += m->P) {
        m->lastPass = N - r0 < m->P ? N - r0 : m->P;
        if ((rc = sbr_pass(m, r0, m->lastPass, N, st))) return rc;
    }
    // ---- norm_stats -> fc_embed -> norm_embed, folded: split-K with the fixed-order finish -------------------------
    const int CF2 = 2 * m->F[4] * m->C[4];
    if ((rc = dz_splitk_linear(w.fc, m->pooled, N, CF2, CF2, EMB, FC_SPLIT, m->parts, 0, d_out, st))) return rc;
    if ((rc = dz_launch_nan_rows(d_out, N, EMB, geo.tooshort, st))) return rc;
    return normalize ? dz_launch_l2norm(d_out, N, EMB, 1.0f, st) : 0;
}

extern "C" int dz_sbr_forward(dz_sbr* m, const float* d_wave, long long wave_stride, const float* d_masks, int N,
                              int mask_frames, float* d_out, void* stream) {
    return dz_handle_forward("dz_sbr_forward", m, d_wave, wave_stride, d_masks, N, mask_frames, d_out, stream, sbr_run);
}

extern "C" int dz_sbr_forward_groups(dz_sbr* m, const float* d_wave, long long wave_stride, const float* d_masks,
                                     int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                                     void* stream) {
    return dz_handle_forward_groups("dz_sbr_forward_groups", m, d_wave, wave_stride, d_masks, n_groups, rows_per_group,
                                    mask_frames, normalize, d_out, stream, sbr_run);
}

extern "C" int dz_sbr_peek(dz_sbr* m, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(m && d_ptr && count, "dz_sbr_peek: NULL argument");
    const long long N = m->lastN, n = m->lastPass;
    int T = m->geo.Tc;
    switch (which) {
        case 0: *d_ptr = m->feats; *count = N * T * NMEL; break;
        case 1: case 2: case 3: case 4: case 5: {
            const int l = which - 1;
            DZ_REQUIRE(m->L[l] != nullptr, "dz_sbr_peek: no forward has run");
            *d_ptr = m->L[l]; T = m->T[l];
            *count = n * T * m->F[l] * m->C[l];
            break;
        }
        case 6: *d_ptr = m->pooled; T = m->T[4]; *count = N * 2 * m->F[4] * m->C[4]; break;
        case 7: *d_ptr = m->geo.lens; *count = N; break;
        case 8: *d_ptr = m->geo.rep_T; *count = N; break;
        case 9: *d_ptr = m->ext; *count = 5 * N; break;
        default:
            dz_set_error("dz_sbr_peek: unknown buffer %d", which);
            return 2;
    }
    if (frames) *frames = T;
    return 0;
}

// ---- kernel-level entry points (parity tests) -----------------------------------------------------------------------
extern "C" int dz_k_sbr_se_gate(dz_ctx* ctx, const float* d_y, int rows, int tb, int f, int c, int cr, const int* d_ext,
                                const float* d_w1t, const float* d_b1, const float* d_w2t, const float* d_b2,
                                float* d_part, float* d_gate, void* stream) {
    DZ_REQUIRE(ctx != nullptr, "dz_k_sbr_se_gate: NULL context");
    DZ_HIP(hipSetDevice(ctx->device));
    if (int rc = dz_launch_sbr_se_sum(d_y, rows, tb, f, c, d_ext, d_part, (hipStream_t)stream)) return rc;
    return dz_launch_sbr_se_fc(d_part, rows, f, c, cr, d_ext, d_w1t, d_b1, d_w2t, d_b2, d_gate, (hipStream_t)stream);
}

extern "C" int dz_k_sbr_se_apply(dz_ctx* ctx, const float* d_y, const float* d_gate, const float* d_r, int rows, int tb,
                                 int f, int c, const int* d_ext, float* d_out, void* stream) {
    DZ_REQUIRE(ctx != nullptr, "dz_k_sbr_se_apply: NULL context");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_sbr_se_apply(d_y, d_gate, d_r, rows, tb, f, c, d_ext, d_out, (hipStream_t)stream);
}

extern "C" int dz_k_sbr_att_pool(dz_ctx* ctx, const float* d_x, const float* d_logits, int rows, int tb, int c,
                                 const int* d_ext, float* d_pooled, void* stream) {
    DZ_REQUIRE(ctx != nullptr, "dz_k_sbr_att_pool: NULL context");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_sbr_att_pool(d_x, d_logits, c, rows, tb, c, d_ext, d_pooled, (hipStream_t)stream);
}
