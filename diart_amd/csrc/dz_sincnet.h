// The SincNet front end both original networks start with (seg_api.hip, xvec_api.hip): its geometry, its scratch, its
// launch sequence, and the decision what the first layer behind it reads.  Host code only.
#pragma once
#include "dz_embed.h"

// ---------------------------------------------------------------------------
// geometry of the SincNet front-end for S samples
// ---------------------------------------------------------------------------
struct SincGeom {
    int S, F0, P0, T1, P1, T2, P2;  // conv frames / pooled frames per stage
    int nt0, nt1, nt2;              // tiles carrying instance-norm partials
    bool ok;
};
static SincGeom sinc_geom(int S, bool conv0_split = false) {
    SincGeom g;
    memset(&g, 0, sizeof(g));
    g.S = S;
    if (S < 251) return g;
    g.F0 = (S - 251) / 10 + 1;
    g.P0 = g.F0 / 3;
    g.T1 = g.P0 - 4;
    g.P1 = g.T1 > 0 ? g.T1 / 3 : 0;
    g.T2 = g.P1 - 4;
    g.P2 = g.T2 > 0 ? g.T2 / 3 : 0;
    g.nt0 = conv0_split ? dz_conv0_split_ntile(g.F0) : (g.F0 + 191) / 192;
    g.nt1 = g.T1 > 0 ? dz_convgemm_ntile(g.T1) : 0;
    g.nt2 = g.T2 > 0 ? dz_convgemm_ntile(g.T2) : 0;
    g.ok = g.P2 > 0;
    return g;
}

struct SincScratch {
    float *stats, *y0, *part0, *sc0, *sh0, *y1, *part1, *sc1, *sh1, *y2, *part2, *sc2, *sh2;
    float* y2s;      // y2 normalised + split: the f16 planes [2][Bm * P2 rows][64] (kb-major) the first layer of each network reads
    void *bank_frag, *w1_frag, *w2_frag;     // the sinc bank / conv1 / conv2 weights in their kernels' fragment order (filled once, at create)
    void carve(Arena& a, const SincGeom& g, int Bm) {
        bank_frag = a.take((size_t)dz_sinc_bank_frag_bytes() / 4);
        w1_frag = a.take((size_t)dz_conv_pool_wfrag_bytes(80) / 4);
        w2_frag = a.take((size_t)dz_conv_pool_wfrag_bytes(64) / 4);
        stats = a.take((size_t)Bm * 2 * DZ_WS_G);   // slice moments of the waveform
        y0 = a.take((size_t)Bm * g.P0 * 80);
        part0 = a.take((size_t)Bm * g.nt0 * 80 * 2);
        sc0 = a.take((size_t)Bm * 80);
        sh0 = a.take((size_t)Bm * 80);
        y1 = a.take((size_t)Bm * g.P1 * 64);
        part1 = a.take((size_t)Bm * g.nt1 * 64 * 2);
        sc1 = a.take((size_t)Bm * 64);
        sh1 = a.take((size_t)Bm * 64);
        y2 = a.take((size_t)Bm * g.P2 * 64);
        part2 = a.take((size_t)Bm * g.nt2 * 64 * 2);
        sc2 = a.take((size_t)Bm * 64);
        sh2 = a.take((size_t)Bm * 64);
        y2s = a.take((size_t)Bm * g.P2 * 64);
    }
};

// the register-resident operands of the SincNet kernels in fragment order: once per handle (the weights are final then)
static int sinc_repack(const dz_sincnet_weights& w, const SincScratch& s) {
    int rc = 0;
    if (w.filt_split) rc = dz_launch_sinc_bank_frag(w.filt_split, s.bank_frag, nullptr);
    if (!rc && w.w1_split) rc = dz_launch_conv_pool_wfrag(80, w.w1_split, 416, s.w1_frag, nullptr);
    if (!rc && w.w2_split) rc = dz_launch_conv_pool_wfrag(64, w.w2_split, 320, s.w2_frag, nullptr);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) {
        dz_set_error("sinc_repack: hipStreamSynchronize failed");
        rc = 1;
    }
    return rc;
}

// DZ_FUSED_NORM=0 keeps the three finalize_norm launches of a SincNet; by default (split-f16 path)
// every consumer derives its InstanceNorm scale / shift from the producer's tile partials itself
static bool sinc_fused_norm(const dz_sincnet_weights& w) {
    const char* v = dz_exp_env("DZ_FUSED_NORM");
    return w.w1_split && w.w2_split && dz_conv_pool_enabled() && !(v && v[0] == '0');
}
// norm-on-load of stage i's output (C channels, P frames per chunk) in its consumer: from the stage's tile partials
// when the norms are fused, else from the scale / shift finalize_norm left
static DzGemm& sinc_norm_on_load(DzGemm& g, bool fused, const float* part, int tiles, int P, const float* gamma,
                                 const float* beta, const float* scale, const float* shift, int C) {
    return fused ? g.norm_partials(part, tiles, P, gamma, beta, C) : g.norm_scaled(scale, shift, C);
}

// What the first layer behind the SincNet (the first LSTM projection, tdnn1) reads.  Both handles' create checks make
// the planes of conv1 / conv2 and the row-major planes of that layer all present or all absent.
//   SINC_OUT_PLANES: y2 is normalised and split ONCE (norm_split_kernel) into s.y2s, planes of B * P2 * 64 elements,
//     and the layer runs flattened on the pre-split GEMM — whenever the handle's wide layers do, the weights came with
//     kb-major planes for that layer and the SincNet's norms are the fused ones (tile partials).
//   SINC_OUT_F32: exact-f32 weights (no split planes anywhere in the SincNet) with the f32 MFMA GEMM on: y2 is
//     normalised ONCE into s.y2s as f32 rows (norm_f32_kernel reads the tile partials itself: no third finalize_norm
//     launch) and the layer runs flattened on k_gemm_f32.hip.
//   SINC_OUT_NORM_ON_LOAD: the layer reads y2 per chunk and normalises on load (sinc_y2_norm).  The experiments
//     build's non-fused f16 configurations (DZ_FUSED_NORM=0 / DZ_CONV_POOL=0) and exact f32 without the f32 GEMM.
enum SincOut { SINC_OUT_PLANES, SINC_OUT_F32, SINC_OUT_NORM_ON_LOAD };
static SincOut sinc_out_source(const dz_sincnet_weights& w, bool wide_pre, const void* first_layer_kb) {
    if (wide_pre && first_layer_kb && sinc_fused_norm(w)) return SINC_OUT_PLANES;
    if (!w.filt_split && !w.w1_split && !w.w2_split && dz_option(DZ_OPT_F32_GEMM) != 0) return SINC_OUT_F32;
    return SINC_OUT_NORM_ON_LOAD;
}
static DzGemm& sinc_y2_norm(DzGemm& g, const dz_sincnet_weights& w, const SincGeom& geo, const SincScratch& s) {
    return sinc_norm_on_load(g, sinc_fused_norm(w), s.part2, geo.nt2, geo.P2, w.in2_g, w.in2_b, s.sc2, s.sh2, 64);
}

// wave -> y2 [B][P2][64] (pre-norm) + part2 (or sc2 / sh2), and y2s when `out` says so: 4 launches, 5 with the
// norm pass into y2s, 7 with the finalize_norm launches of the non-fused paths.
// ext_stats: slice moments of these B windows somebody already computed (dz_wave_stats: the
// segmentation and the embedding network normalise the SAME waveform, InstanceNorm1d(1) statistics
// do not depend on the network) — NULL: compute them here.
// ext_conv0: y0 / part0 of these B windows are already (being) written on this stream's dependencies by
// dz_sinc_conv0_pair — the first stage of both networks in one launch
static int run_sincnet(const dz_sincnet_weights& w, const SincGeom& g, const SincScratch& s, const float* wave,
                       long long stride, int B, hipStream_t st, SincOut out, const float* ext_stats = nullptr,
                       bool ext_conv0 = false) {
    int rc;
    const float* stats = ext_stats ? ext_stats : s.stats;
    if (!ext_stats && !ext_conv0) {
        DzProfScope ps(DZ_T_WAVE, B);
        if ((rc = dz_launch_wave_stats(wave, stride, B, g.S, s.stats, st))) return rc;
    }
    if (!ext_conv0) {
        DzProfScope ps(DZ_T_CONV0, B);
        rc = w.filt_split ? dz_launch_sinc_conv0_split(wave, stride, B, g.S, stats, 1, w.wav_gamma, w.wav_beta,
                                                       w.filt_split, s.y0, g.P0, s.part0, g.nt0, st, s.bank_frag)
                          : dz_launch_sinc_conv0(wave, stride, B, g.S, stats, 1, w.wav_gamma, w.wav_beta, w.filt, s.y0,
                                                 g.P0, s.part0, g.nt0, st);
        if (rc) return rc;
    }
    const bool fused = sinc_fused_norm(w);
    const auto finalize = [&](const float* part, int ntile, int C, int P, const float* gamma, const float* beta,
                              float* scale, float* shift) {
        DzProfScope ps(DZ_T_FIN, B);
        return dz_launch_finalize_norm(part, B, ntile, C, P, gamma, beta, scale, shift, st);
    };
    if (!fused && (rc = finalize(s.part0, g.nt0, 80, g.P0, w.in0_g, w.in0_b, s.sc0, s.sh0))) return rc;
    // conv1: 80 -> 60(64), k5, + pool3
    const dz_layer c1 = {w.w1, w.b1, nullptr, nullptr, w.w1_split};
    DzGemm g1 = DzGemm::conv1d(c1, s.y0, 80, B, g.P0, 80, s.y1, 64, 64, DZ_EPI_POOL3).taps(5, 1, 0).padded(416, 64)
                    .pool3(s.part1).frag(s.w1_frag).prof(DZ_T_CONV1, B);
    if ((rc = sinc_norm_on_load(g1, fused, s.part0, g.nt0, g.P0, w.in0_g, w.in0_b, s.sc0, s.sh0, 80).run(st))) return rc;
    if (!fused && (rc = finalize(s.part1, g.nt1, 64, g.P1, w.in1_g, w.in1_b, s.sc1, s.sh1))) return rc;
    // conv2: 60(64) -> 60(64), k5, + pool3
    const dz_layer c2 = {w.w2, w.b2, nullptr, nullptr, w.w2_split};
    DzGemm g2 = DzGemm::conv1d(c2, s.y1, 64, B, g.P1, 64, s.y2, 64, 64, DZ_EPI_POOL3).taps(5, 1, 0).padded(320, 64)
                    .pool3(s.part2).frag(s.w2_frag).prof(DZ_T_CONV2, B);
    if ((rc = sinc_norm_on_load(g2, fused, s.part1, g.nt1, g.P1, w.in1_g, w.in1_b, s.sc1, s.sh1, 64).run(st))) return rc;
    switch (out) {
        case SINC_OUT_PLANES: {
            DzProfScope ps(DZ_T_NSPLIT, B);
            return dz_launch_norm_split(s.y2, s.part2, g.nt2, g.P2, w.in2_g, w.in2_b, s.y2s, (long long)B * g.P2 * 64, B, st);
        }
        case SINC_OUT_F32: {
            DzProfScope ps(DZ_T_NSPLIT, B);
            return dz_launch_norm_f32(s.y2, s.part2, g.nt2, g.P2, w.in2_g, w.in2_b, s.y2s, B, st);
        }
        case SINC_OUT_NORM_ON_LOAD: break;
    }
    return fused ? 0 : finalize(s.part2, g.nt2, 64, g.P2, w.in2_g, w.in2_b, s.sc2, s.sh2);
}

// What a caller handed handle h (dz_seg, dz_emb) for its NEXT SincNet only — moments (dz_*_use_wave_stats) and the first
// stage of B chunks (dz_sinc_conv0_pair): both are consumed, and cleared, here.
template <typename H>
static int sinc_take_handoffs(const char* who, H* h, int B, const float** ext_stats, bool* ext_conv0) {
    *ext_stats = h->ext_stats;
    h->ext_stats = nullptr;
    const int pair_B = h->ext_conv0_B;
    h->ext_conv0_B = 0;
    DZ_REQUIRE(pair_B == 0 || pair_B == B, "%s: dz_sinc_conv0_pair ran for %d chunks, this call has %d", who, pair_B, B);
    *ext_conv0 = pair_B > 0;
    return 0;
}

// what dz_seg_create / dz_emb_create end with: the arena and the SincNet operands in fragment order; on failure destroy(h)
template <typename H>
static int sinc_handle_alloc(const char* who, H* h, void (*carve)(H*, Arena&), int (*destroy)(H*), H** out) {
    int rc = dz_arena_alloc(who, h, carve);
    if (!rc) rc = sinc_repack(h->w.sinc, h->ss);
    if (rc) {
        destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

#ifdef DZ_EXPERIMENTS
// the SincNet side of a segmentation handle, for dz_sinc_conv0_pair (xvec_api.hip), which writes the first stage of
// both networks and leaves each handle its hand-off
struct SincFront {
    dz_ctx* ctx;
    int Bm;
    const SincGeom* g;
    const dz_sincnet_weights* w;
    const SincScratch* ss;
    int* ext_conv0_B;
};
SincFront dz_seg_sinc_front(dz_seg* s);      // seg_api.hip
#endif

static int check_wave(const char* who, const float* d_wave, long long stride, int S) {
    DZ_REQUIRE(d_wave != nullptr, "%s: d_wave is NULL", who);
    DZ_REQUIRE(((uintptr_t)d_wave & 15) == 0 && (stride & 3) == 0,
               "%s: waveform rows must be 16-byte aligned (ptr %p, stride %lld)", who,
               (const void*)d_wave, stride);
    DZ_REQUIRE(stride >= 0, "%s: negative stride", who);
    (void)S;
    return 0;
}
