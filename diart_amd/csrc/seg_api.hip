// dz_seg_*: launch sequence of the pyannote segmentation network (include/diart_amd.h): SincNet, four bidirectional
// LSTM layers (x-projection GEMM + persistent recurrence), the MLP head.  Host code driving the kernels in k_*.hip.
#include "dz_sincnet.h"

struct dz_seg {
    dz_ctx* ctx;
    dz_seg_weights w;
    SincGeom g;
    int Bm;
    bool pre;    // wide layers on k_gemm_pre.hip (activations travel as f16 hi/lo planes)
    const float* ext_stats;   // dz_seg_use_wave_stats: consumed (and cleared) by the next forward
    const float* cur_stats;   // the slice moments the front half of the current forward normalised with (NaN rows, dz_ws_bad)
    int ext_conv0_B;          // dz_sinc_conv0_pair wrote y0 / part0 of this many chunks: consumed by the next forward
    char* arena;
    SincScratch ss;
    float *gx, *gx0, *h0, *h1, *m0, *m1, *logit;
    int front_B;              // dz_seg_front ran for this many chunks and dz_seg_back has not consumed it yet
    hipEvent_t ev_gx0_free;   // recorded behind the layer-0 recurrence: the next dz_seg_front may overwrite gx0
};

extern "C" int dz_seg_frames_for(int num_samples) { return sinc_geom(num_samples).P2; }

static void seg_carve(dz_seg* s, Arena& a) {
    const size_t rows = (size_t)s->Bm * s->g.P2;
    s->ss.carve(a, s->g, s->Bm);
    s->gx = a.take(rows * 1024);
    s->gx0 = a.take(rows * 1024);      // layer 0's x-projection: written by the front half, one step ahead
    s->h0 = a.take(rows * 256);
    s->h1 = a.take(rows * 256);
    s->m0 = a.take(rows * 128);
    s->m1 = a.take(rows * 128);
    s->logit = a.take(rows * 8);
}

extern "C" int dz_seg_create(dz_ctx* ctx, const dz_seg_weights* w, int max_batch, int num_samples,
                             dz_seg** out) {
    DZ_REQUIRE(ctx && w && out, "dz_seg_create: NULL argument");
    DZ_REQUIRE(max_batch >= 1, "dz_seg_create: max_batch %d", max_batch);
    const SincGeom g = sinc_geom(num_samples, w->sinc.filt_split != nullptr);
    DZ_REQUIRE(g.ok, "dz_seg_create: %d samples is too short for SincNet", num_samples);
    DZ_REQUIRE(w->num_classes >= 1 && w->num_classes <= 8, "dz_seg_create: num_classes %d",
               w->num_classes);
    if (w->powerset)
        DZ_REQUIRE(w->num_classes == 1 + w->num_speakers + w->num_speakers * (w->num_speakers - 1) / 2,
                   "dz_seg_create: powerset with %d classes / %d speakers", w->num_classes,
                   w->num_speakers);
    // run_sincnet leaves the last InstanceNorm to the consumer's prologue whenever conv1 / conv2 came
    // with split planes; a first projection WITHOUT planes would then read sc2 / sh2 nobody wrote
    DZ_REQUIRE((w->sinc.w1_split != nullptr) == (w->sinc.w2_split != nullptr) &&
                   (w->sinc.w1_split != nullptr) == (w->wih_split[0] != nullptr),
               "dz_seg_create: the split planes of SincNet conv1 / conv2 and of the first LSTM projection "
               "must be all present or all absent");
    DZ_HIP(hipSetDevice(ctx->device));
    dz_seg* s = new (std::nothrow) dz_seg;
    DZ_REQUIRE(s != nullptr, "dz_seg_create: out of memory");
    s->ctx = ctx; s->w = *w; s->g = g; s->Bm = max_batch; s->arena = nullptr; s->ext_stats = nullptr; s->cur_stats = nullptr;
    s->ext_conv0_B = 0;
    s->front_B = 0; s->ev_gx0_free = nullptr;
    DZ_HIP(hipEventCreateWithFlags(&s->ev_gx0_free, hipEventDisableTiming));
    s->pre = w->wih_split[1] && w->wih_split[2] && w->wih_split[3] &&
             w->lin0_split && w->lin1_split;
    return sinc_handle_alloc("dz_seg_create", s, seg_carve, dz_seg_destroy, out);      // (on failure: the arena, the event)
}

extern "C" int dz_seg_destroy(dz_seg* seg) {
    if (seg) {
        if (seg->arena) (void)hipFree(seg->arena);
        if (seg->ev_gx0_free) (void)hipEventDestroy(seg->ev_gx0_free);
        delete seg;
    }
    return 0;
}

extern "C" int dz_seg_use_wave_stats(dz_seg* seg, const float* d_moments) {
    DZ_REQUIRE(seg != nullptr, "dz_seg_use_wave_stats: NULL handle");
    seg->ext_stats = d_moments;
    return 0;
}

#ifdef DZ_EXPERIMENTS
SincFront dz_seg_sinc_front(dz_seg* s) { return {s->ctx, s->Bm, &s->g, &s->w.sinc, &s->ss, &s->ext_conv0_B}; }
#endif

static bool mlp_head_enabled() {
    static const bool on = [] {
        const char* e = dz_exp_env("DZ_MLP_HEAD");
        return !(e && e[0] == '0');
    }();
    return on;
}

// The opening of every entry point: argument checks (d_wave: entries with a front half), the handle's device.  The
// caller then holds a DzRangeScope over its launches.
static int seg_open(dz_seg* s, bool have_out, int B, bool has_wave, const float* d_wave, long long wave_stride) {
    DZ_REQUIRE(s && have_out, "dz_seg_forward: NULL argument");
    DZ_REQUIRE(B >= 1 && B <= s->Bm, "dz_seg_forward: batch %d outside [1, %d]", B, s->Bm);
    if (has_wave)
        if (int rc = check_wave("dz_seg_forward", d_wave, wave_stride, s->g.S)) return rc;
    DZ_HIP(hipSetDevice(s->ctx->device));
    return 0;
}

// Front half: SincNet, then layer 0's x-projection of both directions as one GEMM (N = 1024) into gx0, reading what
// sinc_out_source says.  Leaves front_B = B and cur_stats = the moments these chunks were normalised with.
static int seg_front_half(dz_seg* s, const float* d_wave, long long wave_stride, int B, hipStream_t st) {
    const dz_seg_weights& w = s->w;
    const int F = s->g.P2;
    const long long rows = (long long)B * F;
    int rc;
    const float* ext;
    bool pair;
    if ((rc = sinc_take_handoffs("dz_seg_forward", s, B, &ext, &pair))) return rc;
    const SincOut src = sinc_out_source(w.sinc, s->pre, w.wih0_split_kb);
    if ((rc = run_sincnet(w.sinc, s->g, s->ss, d_wave, wave_stride, B, st, src, ext, pair))) return rc;
    s->cur_stats = ext ? ext : s->ss.stats;
    const dz_layer L = {w.wih[0], w.bih[0], nullptr, nullptr, src == SINC_OUT_PLANES ? w.wih0_split_kb : w.wih_split[0]};
    // y2 per chunk with its norm on load, or one flattened GEMM without a prologue over y2s: normalised planes
    // (k_gemm_pre.hip) or exact-f32 rows (k_gemm_f32.hip)
    DzGemm g = src == SINC_OUT_NORM_ON_LOAD
                   ? DzGemm::conv1d(L, s->ss.y2, 64, B, F, 64, s->gx0, 1024, 1024, DZ_EPI_BIAS)
                   : DzGemm::dense(L, s->ss.y2s, 64, rows, 64, s->gx0, 1024, 1024, DZ_EPI_BIAS)
                         .xplanes(src == SINC_OUT_PLANES ? s->ss.y2s : nullptr, rows * 64);
    if (src == SINC_OUT_NORM_ON_LOAD) sinc_y2_norm(g, w.sinc, s->g, s->ss);
    if ((rc = g.prof(DZ_T_PROJ0, B).run(st))) return rc;
    s->front_B = B;
    return 0;
}

// Back half: 4 x persistent recurrence, the x-projections of layers 1 .. 3 between them, the MLP head — of the B chunks
// whose layer-0 projection the front half left in gx0.
// With s->pre the hidden states travel as f16 (hi, lo) planes (same bytes as f32, same buffers)
// and the projections of layers 1..3 and the MLP run on k_gemm_pre.hip.
static int seg_back_half(dz_seg* s, int B, float* d_out, float* d_osp, float gamma, float beta, int normalize,
                         float* d_vad, hipStream_t st, int track = DZ_TRACK_SPEECH) {
    const dz_seg_weights& w = s->w;
    const int F = s->g.P2;
    const long long rows = (long long)B * F;
    int rc;
    const float* lin = nullptr;
    for (int layer = 0; layer < 4; ++layer) {
        float* const gxl = layer == 0 ? s->gx0 : s->gx;
        if (layer > 0) {
            const dz_layer L = {w.wih[layer], w.bih[layer], nullptr, nullptr, w.wih_split[layer]};
            if ((rc = DzGemm::dense(L, lin, 256, rows, 256, gxl, 1024, 1024, DZ_EPI_BIAS)
                          .xplanes(s->pre ? lin : nullptr, rows * 256).prof(DZ_T_PROJ, B).run(st)))
                return rc;
        }
        float* hout = (layer & 1) ? s->h1 : s->h0;
        { DzProfScope ps(DZ_T_REC, B);
          // gx columns are unit-major (weights.py permutes the rows of W_ih); 16 chains per
          // workgroup on the matrix cores when the layer came with split planes of W_hh
          float* hf = s->pre ? nullptr : hout;
          void* hs = s->pre ? (void*)hout : nullptr;
          rc = w.whh_split[layer]
                   ? dz_launch_lstm_mfma(gxl, w.whh_split[layer], hf, hs, rows * 256, B, F, 1, w.lstm_variant, st)
                   : dz_launch_lstm(gxl, w.whh[layer], hf, hs, rows * 256, B, F, 1, st);
          if (rc) return rc; }
        if (layer == 0) {            // gx0 has been read: the next front half may overwrite it
            DZ_HIP(hipEventRecord(s->ev_gx0_free, st));
            s->front_B = 0;
        }
        lin = hout;
    }
    // default precision, no min-max normalisation of the OSP weights (it needs whole chunks): MLP +
    // classifier + activation + OSP in ONE launch (k_mlp_head.hip); DZ_MLP_HEAD=0: three launches
    if (s->pre && mlp_head_enabled() && !(d_osp && normalize) && w.num_classes <= 8) {
        DzMlpHead m{};
        m.Xsplit = lin; m.xplane = rows * 256;
        m.W0split = w.lin0_split; m.W1split = w.lin1_split;
        m.b0 = w.lin0_b; m.b1 = w.lin1_b; m.cw = w.cls_w; m.cb = w.cls_b;
        m.rows = B * F; m.F = F; m.classes = w.num_classes; m.K = w.num_speakers; m.powerset = w.powerset;
        m.gamma = gamma; m.beta = beta; m.seg = d_out; m.wout = d_osp; m.vad = d_vad; m.track = track;
        m.wave_mom = s->cur_stats;        // (split-f16 path: its clamps turn NaN into finite values)
        DzProfScope ps(DZ_T_MLP, B);
        return dz_launch_mlp_head(m, st);
    }
    // Linear(256,128)+leaky, Linear(128,128)+leaky: with s->pre from planes, through planes (m0), to f32 rows (m1)
    const dz_layer lin0 = {w.lin0_w, w.lin0_b, nullptr, nullptr, w.lin0_split};
    const dz_layer lin1 = {w.lin1_w, w.lin1_b, nullptr, nullptr, w.lin1_split};
    if ((rc = DzGemm::dense(lin0, lin, 256, rows, 256, s->pre ? nullptr : s->m0, 128, 128, DZ_EPI_BIAS_LEAKY)
                  .xplanes(s->pre ? lin : nullptr, rows * 256).planes_out(s->pre ? s->m0 : nullptr, rows * 128)
                  .prof(DZ_T_MLP, B).run(st)))
        return rc;
    if ((rc = DzGemm::dense(lin1, s->m0, 128, rows, 128, s->m1, 128, 128, DZ_EPI_BIAS_LEAKY)
                  .xplanes(s->pre ? s->m0 : nullptr, rows * 128).prof(DZ_T_MLP, B).run(st)))
        return rc;
    // classifier + sigmoid / powerset decision (+ OverlappedSpeechPenalty weights): one launch
    DzProfScope ps(DZ_T_CLS, B);
    return dz_launch_seg_head(s->m1, w.cls_w, w.cls_b, B, F, w.num_classes, w.num_speakers, w.powerset, d_out, gamma,
                              beta, normalize, d_osp, st, s->pre ? s->cur_stats : nullptr, d_vad, track);
}

// the whole network on one stream
static int seg_forward(dz_seg* s, const float* d_wave, long long wave_stride, int B, float* d_out, float* d_osp,
                       float gamma, float beta, int normalize, float* d_vad, void* stream, int track = DZ_TRACK_SPEECH) {
    if (int rc = seg_open(s, d_out != nullptr, B, true, d_wave, wave_stride)) return rc;
    DzRangeScope range_scope(s->ctx->oflag_dev);
    if (int rc = seg_front_half(s, d_wave, wave_stride, B, (hipStream_t)stream)) return rc;
    return seg_back_half(s, B, d_out, d_osp, gamma, beta, normalize, d_vad, (hipStream_t)stream, track);
}
extern "C" int dz_seg_forward(dz_seg* s, const float* d_wave, long long wave_stride, int B,
                              float* d_out, void* stream) {
    return seg_forward(s, d_wave, wave_stride, B, d_out, nullptr, 0.f, 0.f, 0, nullptr, stream);
}
extern "C" int dz_seg_forward_osp(dz_seg* s, const float* d_wave, long long wave_stride, int B,
                                  float* d_out, float gamma, float beta, int normalize,
                                  float* d_weights, void* stream) {
    DZ_REQUIRE(d_weights != nullptr, "dz_seg_forward_osp: d_weights is NULL");
    return seg_forward(s, d_wave, wave_stride, B, d_out, d_weights, gamma, beta, normalize, nullptr, stream);
}
// VoiceActivityDetection's hot path (reference blocks/vad.py:146-148): the forward pass whose head also
// writes the speech track d_vad (B,F), the max over speakers of d_out (B,F,K) (dz_vad_frame), so that the
// engine's step never reads the scores back for the reduction
extern "C" int dz_seg_forward_vad(dz_seg* s, const float* d_wave, long long wave_stride, int B, float* d_out,
                                  float* d_vad, void* stream) {
    DZ_REQUIRE(d_out && d_vad, "dz_seg_forward_vad: NULL output");
    DZ_REQUIRE(B >= 1, "dz_seg_forward_vad: batch %d < 1", B);
    DZ_REQUIRE(wave_stride >= 0, "dz_seg_forward_vad: negative stride %lld", wave_stride);
    DZ_REQUIRE(s != nullptr, "dz_seg_forward_vad: NULL handle");
    DZ_REQUIRE(B <= s->Bm, "dz_seg_forward_vad: batch %d outside [1, %d]", B, s->Bm);
    return seg_forward(s, d_wave, wave_stride, B, d_out, nullptr, 0.f, 0.f, 0, d_vad, stream);
}
// dz_seg_forward_vad with the track chosen by the caller: DZ_TRACK_SPEECH is that function, DZ_TRACK_OVERLAP makes the
// head write OverlappedSpeechDetection's track, the second largest of each frame's K >= 2 scores (dz_overlap_frame)
extern "C" int dz_seg_forward_track(dz_seg* s, const float* d_wave, long long wave_stride, int B, float* d_out,
                                    float* d_track, int track, void* stream) {
    DZ_REQUIRE(d_out && d_track, "dz_seg_forward_track: NULL output");
    DZ_REQUIRE(B >= 1, "dz_seg_forward_track: batch %d < 1", B);
    DZ_REQUIRE(wave_stride >= 0, "dz_seg_forward_track: negative stride %lld", wave_stride);
    DZ_REQUIRE(track == DZ_TRACK_SPEECH || track == DZ_TRACK_OVERLAP, "dz_seg_forward_track: unknown track %d", track);
    DZ_REQUIRE(s != nullptr, "dz_seg_forward_track: NULL handle");
    DZ_REQUIRE(B <= s->Bm, "dz_seg_forward_track: batch %d outside [1, %d]", B, s->Bm);
    DZ_REQUIRE(track != DZ_TRACK_OVERLAP || (s->w.num_speakers >= 2 && s->w.num_speakers <= 8),
               "dz_seg_forward_track: the overlap track needs 2 <= speakers <= 8 (got %d)", s->w.num_speakers);
    return seg_forward(s, d_wave, wave_stride, B, d_out, nullptr, 0.f, 0.f, 0, d_track, stream, track);
}
// OverlappedSpeechDetection's reduction alone, for scores that are already on the device (the blocks pipeline):
// d_out (rows) = the second largest of each of the `rows` rows of K scores, `row_stride` floats apart
extern "C" int dz_overlap_track(const float* d_scores, long long row_stride, long long rows, int K, float* d_out,
                                void* stream) {
    DZ_REQUIRE(d_scores && d_out, "dz_overlap_track: NULL argument");
    DZ_REQUIRE(K >= 2 && K <= 8, "dz_overlap_track: 2 <= speakers <= 8 (got %d)", K);
    DZ_REQUIRE(rows >= 1, "dz_overlap_track: rows %lld < 1", rows);
    DZ_REQUIRE(row_stride >= 0, "dz_overlap_track: negative stride %lld", row_stride);
    DZ_REQUIRE(row_stride >= K, "dz_overlap_track: rows %lld floats apart hold no %d scores", row_stride, K);
    return dz_launch_overlap_track(d_scores, row_stride, rows, K, d_out, (hipStream_t)stream);
}
// The two halves of dz_seg_forward_osp for a caller that keeps the stateless front end of the NEXT step
// off the long dependent chain of this one (StreamBatch): dz_seg_front(t + 2) — SincNet and the first
// x-projection, on a stream of its own — runs under the recurrences of dz_seg_back(t) on the same handle.
// The only buffer both halves touch is gx0; the front half waits (on the GPU) for the event the back half
// records behind the layer-0 recurrence that reads it.
extern "C" int dz_seg_front(dz_seg* s, const float* d_wave, long long wave_stride, int B, void* stream) {
    DZ_REQUIRE(s != nullptr, "dz_seg_front: NULL handle");
    if (int rc = seg_open(s, true, B, true, d_wave, wave_stride)) return rc;
    DzRangeScope range_scope(s->ctx->oflag_dev);
    DZ_HIP(hipStreamWaitEvent((hipStream_t)stream, s->ev_gx0_free, 0));   // (never recorded yet: no-op)
    if (int rc = seg_front_half(s, d_wave, wave_stride, B, (hipStream_t)stream)) return rc;
    // (front half alone with the handle's OWN moments: the next dz_seg_front may overwrite them before this step's
    // back half reads them — the NaN rows then come from caller-owned moments only, dz_seg_use_wave_stats)
    if (s->cur_stats == s->ss.stats) s->cur_stats = nullptr;
    return 0;
}
extern "C" int dz_seg_back(dz_seg* s, int B, float* d_out, float gamma, float beta, int normalize,
                           float* d_weights, void* stream) {
    DZ_REQUIRE(s != nullptr, "dz_seg_back: NULL handle");
    DZ_REQUIRE(B == s->front_B, "dz_seg_back: %d chunks, but dz_seg_front prepared %d", B, s->front_B);
    if (int rc = seg_open(s, d_out != nullptr, B, false, nullptr, 0)) return rc;
    DzRangeScope range_scope(s->ctx->oflag_dev);
    return seg_back_half(s, B, d_out, d_weights, gamma, beta, normalize, nullptr, (hipStream_t)stream);
}
