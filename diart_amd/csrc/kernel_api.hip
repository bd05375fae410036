// dz_k_*: the kernel-level entry points the parity tests and the timing tools call (include/diart_amd.h,
// include/diart_amd_experiments.h): one launcher each, on the caller's buffers.  Host code.
#include "dz_sincnet.h"

// ---------------------------------------------------------------------------
// kernel-level entry points (parity tests)
// ---------------------------------------------------------------------------
extern "C" int dz_k_convgemm(dz_ctx* ctx, const dz_convgemm_desc* d, void* stream) {
    DZ_REQUIRE(ctx && d, "dz_k_convgemm: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_convgemm(*d, (hipStream_t)stream);
}
extern "C" int dz_k_gemm_f32(dz_ctx* ctx, const dz_convgemm_desc* d, void* stream) {
    DZ_REQUIRE(ctx && d, "dz_k_gemm_f32: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_gemm_f32(*d, (hipStream_t)stream);
}
extern "C" int dz_k_gemm_split(dz_ctx* ctx, const dz_convgemm_desc* d, void* stream) {
    DZ_REQUIRE(ctx && d, "dz_k_gemm_split: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_gemm_split(*d, (hipStream_t)stream);
}
extern "C" int dz_k_gemm_pre(dz_ctx* ctx, const dz_convgemm_desc* d, void* stream) {
    DZ_REQUIRE(ctx && d, "dz_k_gemm_pre: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_gemm_pre(*d, (hipStream_t)stream);
}
#ifdef DZ_EXPERIMENTS
// generations 2 / 3 of dz_k_gemm_pre: the same requirements, the context's range flag unless the descriptor names one
static int gemm_gen_open(const char* who, dz_ctx* ctx, const dz_convgemm_desc* d, DzConvGemm* p) {
    DZ_REQUIRE(ctx && d, "%s: NULL argument", who);
    DZ_REQUIRE(d->Wsplit && d->Xsplit && (d->Y || d->Ysplit) && d->B == 1 && d->K == d->Kpad && d->K == d->taps * d->Cin &&
                   d->Cin % 32 == 0 && d->Npad % 128 == 0 && d->pad == 0 && !d->X2 && !d->rowbias && d->ksplit <= 1 &&
                   !d->norm_on_load && d->Tout > 0 && d->Tout == d->Tin - (d->taps - 1) * d->dil && d->ldx % 32 == 0 &&
                   d->xplane % d->ldx == 0 && d->xplane / d->ldx >= d->Tin,
               "%s: the requirements of dz_k_gemm_pre apply", who);
    DZ_HIP(hipSetDevice(ctx->device));
    *p = *d;
    if (!p->oflag) p->oflag = ctx->oflag_dev;
    return 0;
}
extern "C" int dz_k_gemm_g2(dz_ctx* ctx, const dz_convgemm_desc* d, int row_fragments, void* stream) {
    DzConvGemm p;
    if (int rc = gemm_gen_open("dz_k_gemm_g2", ctx, d, &p)) return rc;
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_gemm_g2(p, row_fragments, (hipStream_t)stream);
}
extern "C" int dz_k_gemm_g3(dz_ctx* ctx, const dz_convgemm_desc* d, int row_fragments, void* stream) {
    DzConvGemm p;
    if (int rc = gemm_gen_open("dz_k_gemm_g3", ctx, d, &p)) return rc;
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_gemm_g3(p, row_fragments, (hipStream_t)stream);
}
#endif  // DZ_EXPERIMENTS
extern "C" int dz_k_mlp_head(dz_ctx* ctx, const void* xsplit, long long xplane, const void* w0split,
                             const void* w1split, const float* b0, const float* b1, const float* cw,
                             const float* cb, int rows, int frames, int classes, int speakers, int powerset,
                             float gamma, float beta, float* d_seg, float* d_weights, void* stream) {
    DZ_REQUIRE(ctx, "dz_k_mlp_head: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    DzMlpHead m{};
    m.Xsplit = xsplit; m.xplane = xplane; m.W0split = w0split; m.W1split = w1split;
    m.b0 = b0; m.b1 = b1; m.cw = cw; m.cb = cb;
    m.rows = rows; m.F = frames; m.classes = classes; m.K = speakers; m.powerset = powerset;
    m.gamma = gamma; m.beta = beta; m.seg = d_seg; m.wout = d_weights;
    return dz_launch_mlp_head(m, (hipStream_t)stream);
}
extern "C" int dz_k_seg_head(dz_ctx* ctx, const float* m1, const float* cw, const float* cb, int batch,
                             int frames, int classes, int speakers, int powerset, float* d_seg, float gamma,
                             float beta, int normalize, float* d_weights, void* stream) {
    DZ_REQUIRE(ctx && m1 && cw && cb && d_seg, "dz_k_seg_head: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_seg_head(m1, cw, cb, batch, frames, classes, speakers, powerset, d_seg, gamma, beta,
                              normalize, d_weights, (hipStream_t)stream);
}
extern "C" int dz_k_conv_pool(dz_ctx* ctx, const dz_convgemm_desc* d, void* stream) {
    DZ_REQUIRE(ctx && d, "dz_k_conv_pool: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    // kernel-level entry: the weights go into fragment order on every call (the handles do it once, at create)
    DZ_REQUIRE(d->Wsplit && (d->Cin == 80 || d->Cin == 64), "dz_k_conv_pool: Wsplit is NULL or Cin is not 80 / 64");
    std::lock_guard<std::mutex> frag_lock(ctx->frag_mu);
    if (!ctx->convp_frag) DZ_HIP(hipMalloc(&ctx->convp_frag, (size_t)dz_conv_pool_wfrag_bytes(80)));
    if (ctx->convp_used && ctx->convp_user != (hipStream_t)stream) DZ_HIP(hipStreamSynchronize(ctx->convp_user));
    ctx->convp_user = (hipStream_t)stream; ctx->convp_used = true;
    int rc;
    if (!(dz_option(DZ_OPT_PACK_CACHE) && ctx->convp_src == d->Wsplit && ctx->convp_cin == d->Cin && ctx->convp_kpad == d->Kpad)) {
        if ((rc = dz_launch_conv_pool_wfrag(d->Cin, d->Wsplit, d->Kpad, ctx->convp_frag, (hipStream_t)stream))) return rc;
        ctx->convp_src = d->Wsplit; ctx->convp_cin = d->Cin; ctx->convp_kpad = d->Kpad;
    }
    return dz_launch_conv_pool(*d, (hipStream_t)stream, ctx->convp_frag);
}
#ifdef DZ_EXPERIMENTS
// phase time stamps of conv_pool_h (tools/kbench.py): 2 x 64 shader-clock stamps per workgroup
extern "C" int dz_k_conv_pool_debug(long long* d_stamps) {
    dz_conv_pool_dbg = d_stamps;
    return 0;
}
#endif
extern "C" int dz_k_convgemm_ntile(int t_out) { return dz_convgemm_ntile(t_out); }
extern "C" int dz_k_wave_stats(dz_ctx* ctx, const float* d_wave, long long stride, int batch,
                               int samples, float* d_stats, void* stream) {
    DZ_REQUIRE(ctx && d_stats, "dz_k_wave_stats: NULL argument");
    int rc;
    if ((rc = check_wave("dz_k_wave_stats", d_wave, stride, samples))) return rc;
    DZ_HIP(hipSetDevice(ctx->device));
    // kernel-level entry: slice moments into a throw-away buffer, then the (mean, rstd) contract
    float* mom = nullptr;
    DZ_HIP(hipMalloc((void**)&mom, (size_t)batch * 2 * DZ_WS_G * sizeof(float)));
    rc = dz_launch_wave_stats(d_wave, stride, batch, samples, mom, (hipStream_t)stream);
    if (!rc) rc = dz_launch_wave_stats_combine(mom, batch, samples, d_stats, (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(mom);
    return rc;
}
extern "C" int dz_k_sinc_conv0(dz_ctx* ctx, const float* d_wave, long long stride, int batch,
                               int samples, const float* d_stats, float gamma, float beta,
                               const float* d_filt, float* d_y0, float* d_partials, void* stream) {
    DZ_REQUIRE(ctx && d_stats && d_filt && d_y0 && d_partials, "dz_k_sinc_conv0: NULL argument");
    int rc;
    if ((rc = check_wave("dz_k_sinc_conv0", d_wave, stride, samples))) return rc;
    const SincGeom g = sinc_geom(samples);
    DZ_REQUIRE(g.P0 > 0, "dz_k_sinc_conv0: %d samples is too short", samples);
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_sinc_conv0(d_wave, stride, batch, samples, d_stats, 0, gamma, beta, d_filt, d_y0,
                                g.P0, d_partials, g.nt0, (hipStream_t)stream);
}
extern "C" int dz_k_sinc_conv0_split(dz_ctx* ctx, const float* d_wave, long long stride, int batch,
                                     int samples, const float* d_stats, float gamma, float beta,
                                     const void* d_filt_split, float* d_y0, float* d_partials,
                                     void* stream) {
    DZ_REQUIRE(ctx && d_stats && d_filt_split && d_y0 && d_partials, "dz_k_sinc_conv0_split: NULL argument");
    int rc;
    if ((rc = check_wave("dz_k_sinc_conv0_split", d_wave, stride, samples))) return rc;
    const SincGeom g = sinc_geom(samples, true);
    DZ_REQUIRE(g.P0 > 0, "dz_k_sinc_conv0_split: %d samples is too short", samples);
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    // kernel-level entry: the bank goes into fragment order on every call (the handles do it once, at create)
    // (option "pack_cache", off by default: skip the repack when the bank pointer is the one of the previous call —
    // for the timing tools, whose weights do not change; a framework's allocator may hand the same address out again)
    std::lock_guard<std::mutex> frag_lock(ctx->frag_mu);
    if (!ctx->conv0_frag) DZ_HIP(hipMalloc(&ctx->conv0_frag, (size_t)dz_sinc_bank_frag_bytes()));
    if (ctx->conv0_used && ctx->conv0_user != (hipStream_t)stream) DZ_HIP(hipStreamSynchronize(ctx->conv0_user));
    ctx->conv0_user = (hipStream_t)stream; ctx->conv0_used = true;
    if (!(dz_option(DZ_OPT_PACK_CACHE) && ctx->conv0_src == d_filt_split)) {
        if ((rc = dz_launch_sinc_bank_frag(d_filt_split, ctx->conv0_frag, (hipStream_t)stream))) return rc;
        ctx->conv0_src = d_filt_split;
    }
    return dz_launch_sinc_conv0_split(d_wave, stride, batch, samples, d_stats, 0, gamma, beta,
                                      d_filt_split, d_y0, g.P0, d_partials, g.nt0, (hipStream_t)stream, ctx->conv0_frag);
}
extern "C" int dz_k_conv0_split_ntile(int samples) { return sinc_geom(samples, true).nt0; }
#ifdef DZ_EXPERIMENTS
extern "C" int dz_k_sinc_conv0_pair(dz_ctx* ctx, const float* d_wave, long long stride, int batch, int samples,
                                    const float* d_moments, const void* d_pair_planes, const float* d_pair_bsum,
                                    float gamma_seg, float gamma_emb, float* d_y0_seg, float* d_y0_emb,
                                    float* d_part_seg, float* d_part_emb, void* stream) {
    DZ_REQUIRE(ctx && d_moments && d_pair_planes && d_pair_bsum && d_y0_seg && d_y0_emb && d_part_seg && d_part_emb,
               "dz_k_sinc_conv0_pair: NULL argument");
    const SincGeom g = sinc_geom(samples, true);
    DZ_REQUIRE(batch >= 1 && g.F0 >= 3, "dz_k_sinc_conv0_pair: empty input");
    int rc;
    if ((rc = check_wave("dz_k_sinc_conv0_pair", d_wave, stride, samples))) return rc;
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    return dz_launch_sinc_conv0_pair(d_wave, stride, batch, samples, d_moments, d_pair_planes, d_pair_bsum, gamma_seg,
                                     gamma_emb, d_y0_seg, d_y0_emb, g.P0, d_part_seg, d_part_emb, g.nt0,
                                     (hipStream_t)stream);
}
#endif  // DZ_EXPERIMENTS
extern "C" int dz_k_finalize_norm(dz_ctx* ctx, const float* d_partials, int batch, int ntile,
                                  int channels, int frames, const float* d_gamma,
                                  const float* d_beta, float* d_scale, float* d_shift,
                                  void* stream) {
    DZ_REQUIRE(ctx && d_partials && d_gamma && d_beta && d_scale && d_shift,
               "dz_k_finalize_norm: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_finalize_norm(d_partials, batch, ntile, channels, frames, d_gamma, d_beta,
                                   d_scale, d_shift, (hipStream_t)stream);
}
extern "C" int dz_k_lstm(dz_ctx* ctx, const float* d_gx, const float* d_whh, float* d_hout,
                         int batch, int frames, void* stream) {
    DZ_REQUIRE(ctx && d_gx && d_whh && d_hout, "dz_k_lstm: NULL argument");
    DZ_REQUIRE(batch >= 1 && frames >= 1, "dz_k_lstm: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_lstm(d_gx, d_whh, d_hout, nullptr, 0, batch, frames, 0, (hipStream_t)stream);
}
extern "C" int dz_k_lstm_planes(dz_ctx* ctx, const float* d_gx, const float* d_whh,
                                const void* d_whh_split, int variant, void* d_hsplit, long long hplane,
                                int batch, int frames, void* stream) {
    DZ_REQUIRE(ctx && d_gx && d_hsplit && (d_whh || d_whh_split), "dz_k_lstm_planes: NULL argument");
    DZ_REQUIRE(batch >= 1 && frames >= 1, "dz_k_lstm_planes: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    if (d_whh_split)
        return dz_launch_lstm_mfma(d_gx, d_whh_split, nullptr, d_hsplit, hplane, batch, frames, variant >= 3 ? 1 : 0,
                                   variant, (hipStream_t)stream);     // (variants 3 / 4 exist for unit-major gx only)
    return dz_launch_lstm(d_gx, d_whh, nullptr, d_hsplit, hplane, batch, frames, 0, (hipStream_t)stream);
}
extern "C" int dz_k_lstm_mfma(dz_ctx* ctx, const float* d_gx, const void* d_whh_split, float* d_hout,
                              int batch, int frames, int unit_major, int variant, void* stream) {
    DZ_REQUIRE(ctx && d_gx && d_whh_split && d_hout, "dz_k_lstm_mfma: NULL argument");
    DZ_REQUIRE(batch >= 1 && frames >= 1, "dz_k_lstm_mfma: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_lstm_mfma(d_gx, d_whh_split, d_hout, nullptr, 0, batch, frames, unit_major,
                               variant, (hipStream_t)stream);
}
extern "C" int dz_k_stats_pool(dz_ctx* ctx, const float* d_x, int frames, int channels, int ldx,
                               const float* d_weights, int weight_frames, int rows,
                               int rows_per_x, float* d_out, int ldo, void* stream) {
    DZ_REQUIRE(ctx && d_x && d_out, "dz_k_stats_pool: NULL argument");
    DZ_REQUIRE(rows >= 1 && rows_per_x >= 1 && frames >= 2, "dz_k_stats_pool: empty input");
    DZ_HIP(hipSetDevice(ctx->device));
    DZ_REQUIRE(!d_weights || weight_frames >= 2 || weight_frames <= -2, "dz_k_stats_pool: weight_frames %d", weight_frames);
    return dz_launch_stats_pool(d_x, (long long)frames * ldx, frames, channels, ldx, d_weights,
                                d_weights ? weight_frames : frames, rows, rows_per_x, d_out, ldo,
                                (hipStream_t)stream);
}
extern "C" int dz_k_pool_pieces(int pitch) { return dz_pool_pieces(pitch); }
// tdnn5 + statistics pooling on the caller's buffers, the two ways emb_head (xvec_api.hip) runs them: the pooled
// epilogue + pool_combine, or the plain layer + stats_pool at the handle's chunk stride (pitch rows, not frames)
extern "C" int dz_k_tdnn_pool(dz_ctx* ctx, const dz_convgemm_desc* d, const float* d_weights, int weight_frames,
                              int speakers, int pitch, int frames, int channels, int fused, float* d_part,
                              float* d_s0, float* d_out, int ldo, void* stream) {
    DZ_REQUIRE(ctx && d && d_out, "dz_k_tdnn_pool: NULL argument");
    DZ_REQUIRE(d->epi == DZ_EPI_TDNN && d->taps == 1 && d->B == 1, "dz_k_tdnn_pool: built for the flattened 1 x 1 TDNN layer");
    DZ_REQUIRE(speakers >= 1 && pitch >= 1 && frames >= 2 && frames <= pitch && d->Tout >= pitch && d->Tout % pitch == 0,
               "dz_k_tdnn_pool: %d speakers, %d frames of a pitch of %d rows, %d rows in all", speakers, frames, pitch, d->Tout);
    DZ_REQUIRE(channels >= 1 && channels <= d->Nstore && d->Nstore <= d->Npad && ldo >= 2 * channels,
               "dz_k_tdnn_pool: %d channels of %d stored columns, out rows of %d floats", channels, d->Nstore, ldo);
    DZ_REQUIRE(!d_weights || weight_frames >= 2 || weight_frames <= -2, "dz_k_tdnn_pool: weight_frames %d", weight_frames);
    DZ_HIP(hipSetDevice(ctx->device));
    DzRangeScope range_scope(ctx->oflag_dev);
    hipStream_t st = (hipStream_t)stream;
    const int nx = d->Tout / pitch, Fw = d_weights ? weight_frames : frames;
    int rc;
    if (fused) {
        DZ_REQUIRE(d_part && d_s0, "dz_k_tdnn_pool: the pooled epilogue needs part and s0");
        DzPoolFuse q;
        q.w = d_weights; q.Fw = Fw; q.K = speakers; q.P = pitch; q.T = frames; q.np = dz_pool_pieces(pitch);
        q.part = d_part; q.s0 = d_s0;
        if ((rc = dz_launch_gemm_pre_pool(*d, q, st))) return rc;
        return dz_launch_pool_combine(d_part, d_s0, nx, speakers, q.np, pitch, frames, channels, d->Npad, d_out, ldo, st);
    }
    DZ_REQUIRE(d->Y && d->ldy >= channels, "dz_k_tdnn_pool: the stand-alone pooling reads the layer's f32 output Y");
    DZ_REQUIRE(frames <= 640, "dz_k_tdnn_pool: %d frames per chunk (stats_pool: at most 640)", frames);
    if ((rc = dz_launch_gemm_pre(*d, st))) return rc;
    return dz_launch_stats_pool(d->Y, (long long)pitch * d->ldy, frames, channels, d->ldy, d_weights, Fw, nx * speakers,
                                speakers, d_out, ldo, st);
}
extern "C" int dz_k_powerset(dz_ctx* ctx, const float* d_logits, int rows, int classes,
                             int speakers, float* d_out, void* stream) {
    DZ_REQUIRE(ctx && d_logits && d_out, "dz_k_powerset: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    return dz_launch_powerset(d_logits, rows, classes, speakers, d_out, (hipStream_t)stream);
}
