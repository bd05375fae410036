// dz_emb_*: launch sequence of the pyannote x-vector embedding (include/diart_amd.h): SincNet, five TDNN layers,
// weighted statistics pooling, Linear(3000, 512).  Host code driving the kernels in k_*.hip.
#include "dz_sincnet.h"

struct dz_emb {
    dz_ctx* ctx;
    dz_emb_weights w;
    SincGeom g;
    int Bm, T[5];
    bool pre;    // tdnn2..5 on k_gemm_pre.hip (tdnn1 writes f16 hi/lo planes)
    const float* ext_stats;   // dz_emb_use_wave_stats: consumed (and cleared) by the next forward
    const float* cur_stats;   // the slice moments dz_emb_frames normalised with (NaN rows of dz_emb_pool, dz_ws_bad)
    int ext_conv0_B;          // dz_sinc_conv0_pair: see dz_seg
    char* arena;
    SincScratch ss;
    float *a, *b, *x5, *pooled, *parts, *ppart, *ps0;
    // tdnn5 + statistics pooling in one launch (k_gemm_pre.hip, pooled epilogue): dz_emb_frames then
    // stops after tdnn4 and leaves tdnn5 to the call that brings the pooling weights
    int pending_B;            // > 0: frames of that many chunks are waiting at tdnn4's output
    const float* pending_in;  // tdnn4's planes
    int lastB, last_rows;     // chunks of the last dz_emb_frames, rows of the last pooling (0: none yet): dz_emb_peek
    int info[16];             // dz_emb_peek's record (buffer 8), filled by the peek itself
};
static const int kTdnnTaps[5] = {5, 3, 3, 1, 1};
static const int kTdnnDil[5] = {1, 2, 3, 1, 1};
static const int kTdnnCin[5] = {64, 512, 512, 512, 512};
static const int kTdnnN[5] = {512, 512, 512, 512, 1536};
static const int kPoolLd = 3008;
static const int kMaxSpk = 8;
static const int kEmbSplit = 16;  // split-K of Linear(3000, 512): 8 tiles -> 128 workgroups

extern "C" int dz_emb_frames_for(int num_samples) {
    const int f = sinc_geom(num_samples).P2 - 4 - 4 - 6;
    return f > 0 ? f : 0;
}

static void emb_carve(dz_emb* e, Arena& a) {
    e->ss.carve(a, e->g, e->Bm);
    // every TDNN activation keeps the row pitch of the network input (P2 = 293 frames per chunk,
    // the first T[i] rows valid): layers 2..5 then run as ONE flattened GEMM over Bm * P2 rows
    e->a = a.take((size_t)e->Bm * e->g.P2 * 512);
    e->b = a.take((size_t)e->Bm * e->g.P2 * 512);
    e->x5 = a.take((size_t)e->Bm * e->g.P2 * 1536);
    e->pooled = a.take((size_t)e->Bm * kMaxSpk * kPoolLd);
    const int np = dz_pool_pieces(e->g.P2);
    e->ppart = a.take((size_t)e->Bm * np * 4 * 1536 * 2);      // [chunk][np pieces][<= 4 speakers][1536][2]
    e->ps0 = a.take((size_t)e->Bm * np * 4 * 2);
    e->parts = a.take((size_t)kEmbSplit * e->Bm * kMaxSpk * 512);
}

extern "C" int dz_emb_create(dz_ctx* ctx, const dz_emb_weights* w, int max_batch, int num_samples,
                             dz_emb** out) {
    DZ_REQUIRE(ctx && w && out, "dz_emb_create: NULL argument");
    DZ_REQUIRE(max_batch >= 1, "dz_emb_create: max_batch %d", max_batch);
    DZ_REQUIRE(w->dimension == 512, "dz_emb_create: dimension %d (only 512 is built)", w->dimension);
    const SincGeom g = sinc_geom(num_samples, w->sinc.filt_split != nullptr);
    DZ_REQUIRE(g.ok && g.P2 > 14, "dz_emb_create: %d samples is too short", num_samples);
    DZ_REQUIRE((w->sinc.w1_split != nullptr) == (w->sinc.w2_split != nullptr) &&
                   (w->sinc.w1_split != nullptr) == (w->tw_split[0] != nullptr),
               "dz_emb_create: the split planes of SincNet conv1 / conv2 and of tdnn1 must be all present "
               "or all absent (the consumer of the last SincNet stage finalises its InstanceNorm)");
    DZ_HIP(hipSetDevice(ctx->device));
    dz_emb* e = new (std::nothrow) dz_emb;
    DZ_REQUIRE(e != nullptr, "dz_emb_create: out of memory");
    e->ctx = ctx; e->w = *w; e->g = g; e->Bm = max_batch; e->arena = nullptr; e->ext_stats = nullptr; e->cur_stats = nullptr;
    e->ext_conv0_B = 0;
    e->pending_B = 0; e->pending_in = nullptr;
    e->lastB = e->last_rows = 0;
    e->pre = w->tw_split[0] && w->tw_split[1] && w->tw_split[2] &&
             w->tw_split[3] && w->tw_split[4];
    int t = g.P2;
    for (int i = 0; i < 5; ++i) {
        t -= (kTdnnTaps[i] - 1) * kTdnnDil[i];
        e->T[i] = t;
    }
    return sinc_handle_alloc("dz_emb_create", e, emb_carve, dz_emb_destroy, out);
}

extern "C" int dz_emb_destroy(dz_emb* emb) { return dz_handle_destroy(emb); }

extern "C" int dz_emb_use_wave_stats(dz_emb* emb, const float* d_moments) {
    DZ_REQUIRE(emb != nullptr, "dz_emb_use_wave_stats: NULL handle");
    emb->ext_stats = d_moments;
    return 0;
}

// TDNN layer i (0-based) as ONE flattened GEMM over the B * P2 rows of `in` (cin columns; f16 planes when in_planes)
// -> out: planes for the next layer when the wide layers run on k_gemm_pre.hip, tdnn5 always f32 rows.
// Row pitch P = P2 for every activation: a row whose taps reach past the valid frames of its chunk (t >= T[i])
// computes garbage that no valid row ever reads (a valid output row t < T[i] reads input rows t + tap * dil <
// T[i-1] of the same chunk), in exchange the M tiles are 95 % full instead of 73 % (279 rows in 3 x 128).
static DzGemm emb_tdnn(const dz_emb* e, int i, const void* wsplit, const float* in, bool in_planes, int B, float* out) {
    const long long rows = (long long)B * e->g.P2;
    const int cin = kTdnnCin[i], n = kTdnnN[i], K = cin * kTdnnTaps[i];
    const bool out_planes = e->pre && i < 4;
    const dz_layer L = {e->w.tw[i], e->w.tb[i], e->w.ts[i], e->w.th[i], wsplit};
    return DzGemm::dense(L, in, cin, rows, cin, out_planes ? nullptr : out, n, n, DZ_EPI_TDNN)
        .taps(kTdnnTaps[i], kTdnnDil[i], 0).padded((K + 31) / 32 * 32, n).xplanes(in_planes ? in : nullptr, rows * cin)
        .planes_out(out_planes ? out : nullptr, rows * n).prof(DZ_T_TDNN1 + i, B);
}
// tdnn5 of B chunks from tdnn4's output: the last layer of dz_emb_frames, or what dz_emb_pool owes pending frames
static DzGemm emb_tdnn5(const dz_emb* e, const float* in, int B, float* out) {
    return emb_tdnn(e, 4, e->w.tw_split[4], in, e->pre, B, out);
}

// frame features: wave (B) -> x5 [B][T5][1536], or pending at tdnn4's output
static int emb_frames(dz_emb* e, const float* d_wave, long long stride, int B, hipStream_t st) {
    const dz_emb_weights& w = e->w;
    int rc;
    const float* ext;
    bool pair;
    if ((rc = sinc_take_handoffs("dz_emb_frames", e, B, &ext, &pair))) return rc;
    const SincOut src = sinc_out_source(w.sinc, e->pre, w.tw0_split_kb);
    if ((rc = run_sincnet(w.sinc, e->g, e->ss, d_wave, stride, B, st, src, ext, pair))) return rc;
    e->cur_stats = ext ? ext : e->ss.stats;
    e->pending_B = 0;
    e->lastB = B; e->last_rows = 0;
    // e->pre: tdnn1 writes its output as f16 (hi, lo) planes (same bytes, same buffers), tdnn2..5 run
    // on k_gemm_pre.hip, tdnn5 writes the f32 features the statistics pooling reads
    if (src == SINC_OUT_NORM_ON_LOAD) {      // tdnn1 normalises on load with per-chunk statistics, so it runs per chunk
        const int P = e->g.P2;
        const dz_layer L = {w.tw[0], w.tb[0], w.ts[0], w.th[0], w.tw_split[0]};
        DzGemm g = DzGemm::conv1d(L, e->ss.y2, 64, B, P, 64, e->pre ? nullptr : e->a, 512, 512, DZ_EPI_TDNN).taps(5, 1, 0)
                       .padded(320, 512).planes_out(e->pre ? e->a : nullptr, (long long)B * P * 512).prof(DZ_T_TDNN1, B);
        rc = sinc_y2_norm(g, w.sinc, e->g, e->ss).run(st);
    } else {                                 // the normalised y2 (planes or f32 rows), flattened like the layers behind it
        const bool planes = src == SINC_OUT_PLANES;
        rc = emb_tdnn(e, 0, planes ? w.tw0_split_kb : w.tw_split[0], e->ss.y2s, planes, B, e->a).run(st);
    }
    if (rc) return rc;
    const float* in = e->a;
    for (int i = 1; i < 4; ++i) {
        float* out = (i & 1) ? e->b : e->a;
        if ((rc = emb_tdnn(e, i, w.tw_split[i], in, e->pre, B, out).run(st))) return rc;
        in = out;
    }
    DzGemm g5 = emb_tdnn5(e, in, B, e->x5);
    // (the pooled epilogue walks at most two chunks per 128-row tile: chunk pitch >= 128 rows, i.e. windows of
    // ~2.3 s and longer; shorter windows keep the unfused tdnn5 + stats_pool.  pool_fuse = 0: tdnn5 writes its f32
    // output and stats_pool reads it back)
    if (e->pre && dz_option(DZ_OPT_POOL_FUSE) != 0 && e->g.P2 >= 128 && e->T[4] >= 2 && dz_gemm_pre_pool_ok(g5.p)) {
        // tdnn5 runs with the pooling in its epilogue, i.e. when the weights are known (emb_head)
        e->pending_B = B;
        e->pending_in = in;
        return 0;
    }
    return g5.run(st);
}

static int emb_head(dz_emb* e, const float* d_weights, int Fw, int rows, int rows_per_x,
                    int normalize, float* d_out, hipStream_t st) {
    int rc;
    if (e->w.pool_nearest && d_weights) Fw = -Fw;      // the internal launchers carry the resampling mode in the sign (dz_pool_weight)
    const int nx = rows / rows_per_x, P = e->g.P2;
    bool pooled = false;
    if (e->pending_B > 0) {
        DZ_REQUIRE(nx == e->pending_B, "dz_emb_pool: %d chunks, but the frame features of %d are pending", nx,
                   e->pending_B);
        if (rows_per_x <= 4) {
            DzPoolFuse q;
            q.w = d_weights; q.Fw = Fw; q.K = rows_per_x; q.P = P; q.T = e->T[4]; q.np = dz_pool_pieces(P);
            q.part = e->ppart; q.s0 = e->ps0;
            if ((rc = emb_tdnn5(e, e->pending_in, nx, nullptr).run_pooled(q, st))) return rc;
            // the frames stay pending: tdnn4's planes are intact until the next dz_emb_frames, so a second
            // dz_emb_pool on the same frames (other weights) runs the pooled tdnn5 again
            DzProfScope ps(DZ_T_POOL, nx);
            if ((rc = dz_launch_pool_combine(e->ppart, e->ps0, nx, rows_per_x, dz_pool_pieces(P), P, e->T[4], 1500, 1536,
                                             e->pooled, kPoolLd, st)))
                return rc;
            pooled = true;
        } else {            // more than 4 speakers per chunk: plain tdnn5, then the stand-alone pooling below
            if ((rc = emb_tdnn5(e, e->pending_in, nx, e->x5).run(st))) return rc;
            e->pending_B = 0;
        }
    }
    if (!pooled) {
        DzProfScope ps(DZ_T_POOL, nx);
        if ((rc = dz_launch_stats_pool(e->x5, (long long)P * 1536, e->T[4], 1500, 1536, d_weights, Fw, rows, rows_per_x,
                                       e->pooled, kPoolLd, st)))
            return rc;
    }
    e->last_rows = rows;
    // M = rows is tiny (3 per chunk): split K 16 ways so 128 workgroups share the 3008-deep
    // contraction, then reduce the partials in fixed order (+ L2 normalisation) in one pass
    const dz_layer lin = {e->w.emb_w, e->w.emb_b, nullptr, nullptr, nullptr};
    return dz_splitk_linear(lin, e->pooled, rows, kPoolLd, kPoolLd, 512, kEmbSplit, e->parts, normalize, d_out, st,
                            DZ_T_EMBLIN, DZ_T_L2, e->pre ? e->cur_stats : nullptr, rows_per_x);
}

// The opening of the four entry points: argument checks in their order, the handle's device.  batch_fmt / spk_fmt:
// the entry's own wording of the two range errors (who, value, limit); K = 1: an entry without speakers.  The caller
// then holds a DzRangeScope over its launches.
struct EmbEntry {
    const char *who, *batch_fmt, *spk_fmt;
};
static int emb_open(const EmbEntry& en, dz_emb* e, bool have_args, int batch, int K, bool frames_ok, int weight_frames,
                    bool has_wave, const float* d_wave, long long wave_stride) {
    DZ_REQUIRE(e && have_args, "%s: NULL argument", en.who);
    DZ_REQUIRE(batch >= 1 && batch <= e->Bm, en.batch_fmt, en.who, batch, e->Bm);
    DZ_REQUIRE(K >= 1 && K <= kMaxSpk, en.spk_fmt, en.who, K, kMaxSpk);
    DZ_REQUIRE(frames_ok, "%s: weight_frames %d", en.who, weight_frames);
    if (has_wave)
        if (int rc = check_wave(en.who, d_wave, wave_stride, e->g.S)) return rc;
    DZ_HIP(hipSetDevice(e->ctx->device));
    return 0;
}

extern "C" int dz_emb_forward(dz_emb* e, const float* d_wave, long long wave_stride,
                              const float* d_weights, int n_rows, int weight_frames, float* d_out,
                              void* stream) {
    const EmbEntry en = {"dz_emb_forward", "%s: %d rows outside [1, %d]", ""};
    if (int rc = emb_open(en, e, d_out != nullptr, n_rows, 1, d_weights == nullptr || weight_frames >= 2, weight_frames,
                          true, d_wave, wave_stride))
        return rc;
    DzRangeScope range_scope(e->ctx->oflag_dev);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = emb_frames(e, d_wave, wave_stride, n_rows, st)) return rc;
    return emb_head(e, d_weights, d_weights ? weight_frames : e->T[4], n_rows, 1, 0, d_out, st);
}

extern "C" int dz_emb_forward_multi(dz_emb* e, const float* d_wave, long long wave_stride,
                                    const float* d_weights, int batch, int num_speakers,
                                    int weight_frames, int normalize, float* d_out, void* stream) {
    const EmbEntry en = {"dz_emb_forward_multi", "%s: batch %d outside [1, %d]", "%s: %d speakers outside [1, %d]"};
    if (int rc = emb_open(en, e, d_out && d_weights, batch, num_speakers, weight_frames >= 2, weight_frames, true, d_wave,
                          wave_stride))
        return rc;
    DzRangeScope range_scope(e->ctx->oflag_dev);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = emb_frames(e, d_wave, wave_stride, batch, st)) return rc;
    return emb_head(e, d_weights, weight_frames, batch * num_speakers, num_speakers, normalize,
                    d_out, st);
}

// frame features only (SincNet + 5 TDNN) -> internal buffer; independent of the segmentation,
// so a caller can run it on a second stream beside dz_seg_forward
extern "C" int dz_emb_frames(dz_emb* e, const float* d_wave, long long wave_stride, int batch,
                             void* stream) {
    const EmbEntry en = {"dz_emb_frames", "%s: batch %d outside [1, %d]", ""};
    if (int rc = emb_open(en, e, true, batch, 1, true, 0, true, d_wave, wave_stride)) return rc;
    DzRangeScope range_scope(e->ctx->oflag_dev);
    return emb_frames(e, d_wave, wave_stride, batch, (hipStream_t)stream);
}
// pooling + Linear (+ normalisation) of the frame features left by the last dz_emb_frames
extern "C" int dz_emb_pool(dz_emb* e, const float* d_weights, int batch, int num_speakers,
                           int weight_frames, int normalize, float* d_out, void* stream) {
    const EmbEntry en = {"dz_emb_pool", "%s: batch %d outside [1, %d]", "%s: %d speakers"};
    if (int rc = emb_open(en, e, d_out && d_weights, batch, num_speakers, weight_frames >= 2, weight_frames, false, nullptr, 0))
        return rc;
    DzRangeScope range_scope(e->ctx->oflag_dev);
    return emb_head(e, d_weights, weight_frames, batch * num_speakers, num_speakers, normalize,
                    d_out, (hipStream_t)stream);
}

// Read-only views of the handle's buffers as the last call left them (parity tests): no copy, no launch.  The buffers
// and the record are described at the declaration (include/diart_amd.h).
extern "C" int dz_emb_peek(dz_emb* e, int which, const void** d_ptr, long long* count, int* frames) {
    DZ_REQUIRE(e && d_ptr && count, "dz_emb_peek: NULL argument");
    const SincOut src = sinc_out_source(e->w.sinc, e->pre, e->w.tw0_split_kb);
    const long long B = e->lastB, rows = B * e->g.P2;
    const bool x5_valid = B > 0 && e->pending_B == 0;
    int fr = e->g.P2;
    switch (which) {
        case 0: *d_ptr = src == SINC_OUT_NORM_ON_LOAD ? e->ss.y2 : e->ss.y2s; *count = rows * 64; break;
        case 1: *d_ptr = e->a; *count = rows * 512; fr = e->T[2]; break;
        case 2: *d_ptr = e->b; *count = rows * 512; fr = e->T[3]; break;
        case 3: *d_ptr = x5_valid ? e->x5 : nullptr; *count = x5_valid ? rows * 1536 : 0; fr = e->T[4]; break;
        case 4: *d_ptr = e->pooled; *count = (long long)e->last_rows * kPoolLd; fr = e->T[4]; break;
        case 5: *d_ptr = e->ss.sc2; *count = B * 64; break;
        case 6: *d_ptr = e->ss.sh2; *count = B * 64; break;
        case 7: *d_ptr = e->ss.part2; *count = B * e->g.nt2 * 64 * 2; break;
        case 8: {
            const int form = src == SINC_OUT_PLANES ? 0 : src == SINC_OUT_F32 ? 1 : sinc_fused_norm(e->w.sinc) ? 3 : 2;
            const int rec[16] = {form, e->pre ? 1 : 0, e->lastB, e->pending_B, x5_valid ? 1 : 0, e->last_rows, e->g.P2,
                                 e->T[0], e->T[1], e->T[2], e->T[3], e->T[4], e->g.nt2, kPoolLd, 0, 0};
            memcpy(e->info, rec, sizeof(rec));
            *d_ptr = e->info; *count = 16;
            break;
        }
        default:
            dz_set_error("dz_emb_peek: unknown buffer %d", which);
            return 2;
    }
    if (frames) *frames = fr;
    return 0;
}

#ifdef DZ_EXPERIMENTS
// The first SincNet stage of BOTH networks in one launch (k_front.hip sinc_conv0_pair_kernel): writes y0 / part0
// of the two handles; the next dz_seg_forward* / dz_emb_frames of each handle (same B, enqueued behind this launch:
// the same stream, or one that waits for an event recorded after it) then starts at conv1.
extern "C" int dz_sinc_conv0_pair(dz_seg* seg_handle, dz_emb* emb, const float* d_wave, long long wave_stride, int batch,
                                  const float* d_moments, const void* d_pair_planes, const float* d_pair_bsum,
                                  void* stream) {
    DZ_REQUIRE(seg_handle && emb && d_moments && d_pair_planes && d_pair_bsum, "dz_sinc_conv0_pair: NULL argument");
    const SincFront seg = dz_seg_sinc_front(seg_handle);
    DZ_REQUIRE(seg.ctx == emb->ctx, "dz_sinc_conv0_pair: the two handles belong to different contexts");
    DZ_REQUIRE(batch >= 1 && batch <= seg.Bm && batch <= emb->Bm, "dz_sinc_conv0_pair: batch %d outside [1, %d]", batch,
               seg.Bm < emb->Bm ? seg.Bm : emb->Bm);
    DZ_REQUIRE(seg.g->S == emb->g.S && seg.g->nt0 == emb->g.nt0 && seg.g->P0 == emb->g.P0,
               "dz_sinc_conv0_pair: the handles were created for different window lengths");
    DZ_REQUIRE(seg.w->filt_split && emb->w.sinc.filt_split,
               "dz_sinc_conv0_pair: both networks must be in the split-f16 precision (the exact-f32 path keeps one "
               "launch per network)");
    int rc;
    if ((rc = check_wave("dz_sinc_conv0_pair", d_wave, wave_stride, seg.g->S))) return rc;
    DZ_HIP(hipSetDevice(seg.ctx->device));
    DzRangeScope range_scope(seg.ctx->oflag_dev);
    { DzProfScope ps(DZ_T_CONV0_PAIR, batch);
      if ((rc = dz_launch_sinc_conv0_pair(d_wave, wave_stride, batch, seg.g->S, d_moments, d_pair_planes, d_pair_bsum,
                                          seg.w->wav_gamma, emb->w.sinc.wav_gamma, seg.ss->y0, emb->ss.y0, seg.g->P0,
                                          seg.ss->part0, emb->ss.part0, seg.g->nt0, (hipStream_t)stream)))
          return rc; }
    *seg.ext_conv0_B = emb->ext_conv0_B = batch;
    return 0;
}
#endif  // DZ_EXPERIMENTS
