/*
 * diart_amd.h — C ABI of libdiart_amd.so: diart's per-chunk diarization hot path
 * on MI355X (gfx950), hand-written HIP.
 *
 * The reference (juanmc2005/diart v0.9) has no FFI: its plugin boundary is Python
 * duck typing ("Custom models", /root/reference/README.md:186-209).  Each entry point
 * below states which reference call it replaces; `diart_amd/_lib.py` holds the ctypes
 * binding a maintainer would add, and INTEGRATION.md shows how the resulting objects
 * plug into diart.models.SegmentationModel / EmbeddingModel unchanged.
 *
 * Conventions: every function returns 0 on success, non-zero on failure with a
 * message retrievable through dz_last_error() (thread local).  All `d_*` pointers
 * are DEVICE pointers owned by the caller (torch-ROCm tensors); the library only
 * borrows them for the duration of the call and owns nothing but its scratch arena.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls on one
 * handle must be serialised by the caller; distinct handles are independent.
 */
#ifndef DIART_AMD_H
#define DIART_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define DZ_VERSION 230   /* 2.3: kb-major f16 planes for the LDS-DMA kernels; dz_seg_front / dz_seg_back */

typedef struct dz_ctx dz_ctx;
typedef struct dz_seg dz_seg;
typedef struct dz_emb dz_emb;
typedef struct dz_clu dz_clu;

const char* dz_last_error(void);
int dz_version(void);
/* Run-time options of the library, by name; both return 2 (+ dz_last_error) for an unknown name.
 *   "f32_gemm"  (default 1): the wide exact-f32 layers on k_gemm_f32.hip; 0 = on k_convgemm.hip
 *   "pool_fuse" (default 1): statistics pooling inside the last x-vector layer's epilogue; 0 = two launches
 *   "pack_cache" (default 0): dz_k_sinc_conv0_split / dz_k_conv_pool re-order their register-resident operand into the
 *               kernel's fragment order on every call (the handles do it once, at create); 1 = skip that when the operand
 *               pointer is the previous call's (timing tools with fixed weights only)
 * Process-wide, read at every launch: set them while no forward pass is being enqueued.               */
int dz_set_option(const char* name, int value);
int dz_get_option(const char* name, int* value);
/* 1 when the library was compiled with -DDZ_EXPERIMENTS (diart_amd_experiments.h; the never-default kernels
 * and the timing-only modes whose results are wrong exist in that build only), else 0.                */
int dz_has_experiments(void);
/* Host worker pool (clustering / output tail of the N streams of a step): how long an idle worker polls for
 * the next job before it sleeps, in microseconds (default 40; 0 = sleep at once, for ranks with < 4 cores). */
int dz_host_pool_set_spin(int microseconds);

/* one context per (process, GPU) */
int dz_ctx_create(int hip_device, dz_ctx** out);
int dz_ctx_destroy(dz_ctx* ctx);
/* The default arithmetic ("f16x3") represents every GEMM operand as two f16 numbers, i.e. |x| <=
 * 65504; an f32 reference has no such limit.  Operands beyond it are clamped AND flagged: this
 * returns 0 if no kernel of the context has seen one since the last reset, 6 (with a message)
 * otherwise.  Call it after the stream(s) have been synchronised; reset != 0 clears the flag.   */
int dz_range_check(dz_ctx* ctx, int reset);

/* SincNet(stride 10) frame count for a chunk of `num_samples` (293 for 80000):
 * the F of SegmentationModel's (batch, frames, speakers) output,
 * /root/reference/src/diart/models.py:188-198. */
int dz_seg_frames_for(int num_samples);
/* frames left after the 5 TDNN layers (279 for 80000). */
int dz_emb_frames_for(int num_samples);

/* ---- packed weights (device pointers, fp32; layouts in DESIGN.md §3) ------- */
typedef struct {
    float wav_gamma, wav_beta;   /* InstanceNorm1d(1, affine) on the waveform        */
    const float* filt;           /* [128][96]  folded sinc FIR bank (weights.py fold_sinc_filters) */
    const float* in0_g;          /* [80]  InstanceNorm1d(80) gamma                   */
    const float* in0_b;          /* [80]                     beta                    */
    const float* w1;             /* [64][416]  conv1 [co][tap*80+ci], zero padded    */
    const float* b1;             /* [64]                                             */
    const float* in1_g;          /* [64]                                             */
    const float* in1_b;          /* [64]                                             */
    const float* w2;             /* [64][320]  conv2 [co][tap*64+ci]                 */
    const float* b2;             /* [64]                                             */
    const float* in2_g;          /* [64]                                             */
    const float* in2_b;          /* [64]                                             */
    const void* w1_split;        /* split-f16 planes of w1 / w2 (optional, NULL = exact f32)  */
    const void* w2_split;
    const void* filt_split;      /* [2][96][256] f16 planes of the UNFOLDED sinc bank, rows >= 80 and
                                    taps >= 251 zero (optional; NULL = the exact-f32 folded kernel) */
} dz_sincnet_weights;

typedef struct {
    dz_sincnet_weights sinc;
    const float* wih[4];         /* [1024][Kpad] rows = dir*512 + unit*4 + gate (unit-major: the
                                    recurrence reads the four gates of a unit as one 16-byte word) */
    const float* bih[4];         /* [1024]  b_ih + b_hh, same row order                */
    const float* whh[4];         /* [2][512][128]  PyTorch row order (gate*128 + unit) */
    const float* lin0_w;         /* [128][256] */
    const float* lin0_b;         /* [128]      */
    const float* lin1_w;         /* [128][128] */
    const float* lin1_b;         /* [128]      */
    const float* cls_w;          /* [64][128]  classifier rows, zero padded          */
    const float* cls_b;          /* [64]       */
    int num_classes;             /* K (multilabel) or 7 (powerset)                   */
    int powerset;                /* 1: log-softmax -> hard multilabel (models.py:29-39) */
    int num_speakers;            /* speakers of the multilabel output (3)            */
    /* split-f16 matrix path (optional; NULL = exact-f32 MFMA for that layer): the same matrices
     * as two f16 planes [2][Npad][Kpad], hi = f16(W), lo = f16((W - hi) * 2^11) (weights.py split_f16).
     * wih_split[0] row-major; wih_split[1..3], lin0_split and lin1_split — the layers whose operands go
     * global -> LDS by LDS-DMA — in the "kb-major" order [2][Kpad / 32][Npad][32] (weights.py kb_major):
     * element (n, k) of a plane at ((k / 32) * Npad + n) * 32 + k % 32                                  */
    const void* wih_split[4];
    const void* lin0_split;
    const void* lin1_split;
    /* W_hh as f16 planes [2 dir][2 (hi, lo*2^11)][512][128], PyTorch row order: the recurrence then
     * runs 16 chains per workgroup on the matrix cores (k_lstm_mfma.hip); NULL = one chain per CU on
     * the f32 vector units (k_lstm.hip, exact f32)                                               */
    const void* whh_split[4];
    int lstm_variant;            /* how whh_split was prepared (weights.py lstm_whh_planes): 0 / 3 = split_f16 of
                                    W_hh (3: gx by LDS-DMA); 1 / 2 (experiments build) = activation scales folded
                                    in, H scaled by 2^0 / 2^8; 4 = the software-pipelined kernel: gate rows times
                                    -log2(e) (i, f, o) / -2 log2(e) (g), columns in the kernel's k' order, AND
                                    wih / wih_split / bih carry the same row scales (gx arrives pre-scaled)      */
    const void* wih0_split_kb;   /* W_ih of layer 0 once more as kb-major planes [2][64 / 32][1024][32] (optional): the first
                                    projection then reads the SincNet output as planes a one-off norm_split_kernel wrote
                                    and runs on k_gemm_pre.hip like layers 1..3 (see dz_emb_weights.tw0_split_kb)        */
} dz_seg_weights;

typedef struct {
    dz_sincnet_weights sinc;
    const float* tw[5];          /* TDNN conv weights [Npad][Kpad], [co][tap*Cin+ci] */
    const float* tb[5];          /* conv bias [Npad]                                 */
    const float* ts[5];          /* folded BatchNorm1d(eval) scale  [Npad]           */
    const float* th[5];          /* folded BatchNorm1d(eval) shift  [Npad]           */
    const float* emb_w;          /* [512][3008]  Linear(3000, D), zero padded        */
    const float* emb_b;          /* [512] */
    int dimension;               /* D = 512 */
    const void* tw_split[5];     /* split-f16 planes of tw[i] (optional, NULL = exact f32): tw_split[0] row-major
                                    [2][Npad][Kpad], tw_split[1..4] kb-major (see dz_seg_weights)  */
    const void* tw0_split_kb;    /* tdnn1's planes once more in the kb-major order (optional): with them — and the SincNet's fused
                                    norms — the last SincNet stage's output is normalised and split ONCE (norm_split_kernel)
                                    and tdnn1 runs on the pre-split GEMM (k_gemm_pre.hip) like tdnn2..5                     */
    int pool_nearest;            /* how StatsPool resamples the (N, Fw) pooling weights to the T feature frames: 0 =
                                    F.interpolate(mode="linear", align_corners=False) (pyannote.audio 2.x .. 3.0),
                                    1 = mode="nearest" (pyannote.audio >= 3.1)                                     */
} dz_emb_weights;

/* ---- segmentation: replaces the callable behind SegmentationModel.__call__ --
 * /root/reference/src/diart/models.py:188-198 (-> pyannote PyanNet.forward, :133)
 * waveform (B,1,S) -> (B,F,K).  d_wave rows are `wave_stride` floats apart so a
 * rolling window can be addressed in place (operators.py:44-100).
 * A window holding a NaN / Inf sample gives a NaN row (what PyTorch's InstanceNorm1d makes of
 * it; blocks/clustering.py:137-145 then ignores the chunk) in BOTH arithmetic modes, and never
 * touches the other rows of the batch; the same holds for the embedding entry points below.  */
int dz_seg_create(dz_ctx* ctx, const dz_seg_weights* w, int max_batch, int num_samples, dz_seg** out);
int dz_seg_forward(dz_seg* seg, const float* d_wave, long long wave_stride, int batch,
                   float* d_out, void* stream);
/* The same forward pass that also leaves the OverlappedSpeechPenalty weights of its output
 * (blocks/embedding.py:98-107 -> functional.py:6-13; d_weights (B,K,F) speaker-major, the layout
 * dz_emb_pool consumes) — the N-stream driver's seg -> OSP hand-off without a launch of its own. */
int dz_seg_forward_osp(dz_seg* seg, const float* d_wave, long long wave_stride, int batch, float* d_out,
                       float gamma, float beta, int normalize, float* d_weights, void* stream);
/* dz_seg_forward that also writes the VoiceActivityDetection speech track: d_vad (B,F) = max over speakers of
 * d_out (B,F,K), NaN where the row is NaN (reference blocks/vad.py:146-148).  Computed by the head kernel
 * that writes d_out; honours dz_seg_use_wave_stats like dz_seg_forward_osp.                               */
int dz_seg_forward_vad(dz_seg* seg, const float* d_wave, long long wave_stride, int batch,
                       float* d_out, float* d_vad, void* stream);
/* dz_seg_forward_vad with the track chosen by the caller.  DZ_TRACK_SPEECH: d_track is dz_seg_forward_vad's d_vad,
 * from the same code.  DZ_TRACK_OVERLAP: the OverlappedSpeechDetection track (pyannote's pipeline of that name on
 * the (frames, speakers) scores), d_track (B,F) = the SECOND LARGEST of each frame's K scores counted with
 * multiplicity, torch.sort(d_out, -1, descending=True).values[..., 1]: NaN is ordered above every number, so a frame
 * with one NaN score gets its largest number and a frame with two gets NaN; a window with non-finite samples has NaN
 * rows and a NaN track.  For a powerset model d_out is the hard 0/1 decision, and the track is 1 exactly where a
 * two-speaker class wins.  Refused (status 2, the message names the function, nothing is launched): NULL handle or
 * outputs, batch < 1 or > max_batch, negative stride, a track that is neither of the two, and for DZ_TRACK_OVERLAP a
 * model with fewer than 2 (or more than 8) speakers: one speaker has no overlap, and it is not answered with zeros. */
enum { DZ_TRACK_SPEECH = 0, DZ_TRACK_OVERLAP = 1 };
int dz_seg_forward_track(dz_seg* seg, const float* d_wave, long long wave_stride, int batch,
                         float* d_out, float* d_track, int track, void* stream);
/* The reduction of DZ_TRACK_OVERLAP alone, for scores already on the device: d_scores holds `rows` rows of K scores,
 * `row_stride` >= K floats apart; d_out (rows) gets each row's second largest as above.  One thread per row; packed
 * rows (row_stride == K) are loaded by whole waves.  Refused like the above: NULL pointers, K < 2 or K > 8, rows < 1,
 * a negative stride or one below K.                                                                               */
int dz_overlap_track(const float* d_scores, long long row_stride, long long rows, int K, float* d_out, void* stream);
int dz_seg_destroy(dz_seg* seg);

/* ---- embedding: replaces the callable behind EmbeddingModel.__call__ --------
 * /root/reference/src/diart/models.py:248-265 (-> XVectorSincNet.forward, :262)
 * waveform (N,1,S), weights (N,Fw) or NULL -> (N,D)                             */
int dz_emb_create(dz_ctx* ctx, const dz_emb_weights* w, int max_batch, int num_samples, dz_emb** out);
int dz_emb_forward(dz_emb* emb, const float* d_wave, long long wave_stride,
                   const float* d_weights, int n_rows, int weight_frames,
                   float* d_out, void* stream);
/* De-duplicated form of SpeakerEmbedding.__call__ (blocks/embedding.py:51-65): the
 * reference repeats each waveform K times and runs the full network per copy; only
 * the statistics pooling depends on the speaker, so frame features are computed once
 * per chunk and pooled K times.  d_weights is (B,K,Fw) speaker-major ("(batch spk)
 * frame", embedding.py:58); output (B,K,D).  normalize!=0 additionally applies
 * EmbeddingNormalization(norm=1) (functional.py:16-27).                          */
int dz_emb_forward_multi(dz_emb* emb, const float* d_wave, long long wave_stride,
                         const float* d_weights, int batch, int num_speakers,
                         int weight_frames, int normalize, float* d_out, void* stream);
/* dz_seg_forward_osp in two halves, for a caller that keeps the stateless front end of its NEXT step off
 * the dependent chain of the current one: dz_seg_front — SincNet + the first LSTM x-projection — may be
 * enqueued (on any stream) while dz_seg_back of the previous step on the SAME handle is still running its
 * recurrences; the handle orders the one buffer they share on the GPU.  dz_seg_back consumes what the last
 * dz_seg_front left (same batch) and must be ordered behind it by the caller (stream order or an event).   */
int dz_seg_front(dz_seg* seg, const float* d_wave, long long wave_stride, int batch, void* stream);
int dz_seg_back(dz_seg* seg, int batch, float* d_out, float gamma, float beta, int normalize,
                float* d_weights /* may be NULL: no OSP weights */, void* stream);

/* InstanceNorm1d(1) statistics of `batch` windows (the first op of BOTH networks' SincNet: the
 * reference computes them once per model, models.py:133 and :262 each run their own front end) as
 * dz_wave_stats_floats() floats per window (slice means and M2s, merged by the consumer).  A handle
 * told about them with dz_*_use_wave_stats skips its own pass over the waveform in its NEXT forward /
 * dz_emb_frames call (one use, rows in the same order as that call's windows; the caller orders the
 * streams).                                                                                      */
int dz_wave_stats_floats(void);
int dz_wave_stats(dz_ctx* ctx, const float* d_wave, long long wave_stride, int batch, int num_samples,
                  float* d_moments, void* stream);
int dz_seg_use_wave_stats(dz_seg* seg, const float* d_moments);
int dz_emb_use_wave_stats(dz_emb* emb, const float* d_moments);

/* The two halves of dz_emb_forward_multi.  dz_emb_frames (SincNet + TDNN stack, 99.5 % of the
 * embedding FLOPs) does not depend on the segmentation, so it can run on a second stream while
 * dz_seg_forward's latency-bound LSTM occupies a handful of CUs; dz_emb_pool then consumes the
 * OSP weights.  The frame features stay in the handle's scratch between the two calls, and until the
 * next dz_emb_frames: dz_emb_pool may be called again on the same frames with other weights (on the
 * split-f16 path with windows of >= 128 frames the last TDNN layer runs inside dz_emb_pool, with the
 * pooling in its epilogue, so every call pays for that layer again).                               */
int dz_emb_frames(dz_emb* emb, const float* d_wave, long long wave_stride, int batch, void* stream);
int dz_emb_pool(dz_emb* emb, const float* d_weights, int batch, int num_speakers,
                int weight_frames, int normalize, float* d_out, void* stream);
/* pointer + element count of a buffer of the handle as the LAST call left it (parity tests): a view, no copy and no
 * launch.  B = chunks of the last dz_emb_frames / forward, P2 = frames per chunk at the SincNet's output = the row
 * pitch of every activation; rows t >= the layer's valid frame count of a chunk are never read and hold anything.
 * Counts are in 4-byte elements; "planes" = the two kb-major f16 planes (hi, lo * 2^11) of [B * P2 rows][n],
 * [2][n / 32][B * P2][32], which take the same bytes as the f32 rows.
 *   0  the last SincNet stage as tdnn1 consumes it, (B * P2, 64), channels 60 .. 63 padding; the record's `form`:
 *        0 normalised planes  1 normalised f32 rows  2 raw y2, scale / shift (5, 6) applied on load
 *        3 raw y2, normalised on load from the tile partials (7)
 *   1  tdnn3's output, 2  tdnn4's output: (B * P2, 512), planes when the record says so, else f32 rows (tdnn1's and
 *        tdnn2's outputs are overwritten by then)
 *   3  tdnn5's output (B * P2, 1536) f32 rows — only where tdnn5 ran on its own; while the frames are pending at
 *        tdnn4's output (tdnn5 runs inside the pooling call) there is none: *d_ptr = NULL, *count = 0
 *   4  pooled (rows of the last pooling, ld): mean at columns 0 .. 1499, std at 1500 .. 2999
 *   5, 6  InstanceNorm scale / shift of the last SincNet stage (B, 64), written in form 2 only
 *   7  tile partials of the last SincNet stage (B, nt2, 64, 2)
 *   8  the record, 16 ints in HOST memory (valid until the next call on the handle): form, planes (0 / 1), B,
 *        pending chunks, tdnn5 valid (0 / 1), rows of the last pooling, P2, T[0 .. 4] (valid frames behind tdnn1 ..
 *        tdnn5), nt2, ld of pooled, 0, 0
 * *frames receives the valid frames per chunk of that buffer (P2, T[2], T[3], T[4]).                            */
int dz_emb_peek(dz_emb* emb, int which, const void** d_ptr, long long* count, int* frames);
int dz_emb_destroy(dz_emb* emb);

/* ---- ECAPA-TDNN embedding (BASELINE.json config 3): replaces the callable behind
 * EmbeddingModel.__call__ when the embedding is speechbrain/spkrec-ecapa-voxceleb, i.e.
 * pyannote's PretrainedSpeakerEmbedding.__call__(waveforms, masks) reached through the fallback
 * of /root/reference/src/diart/models.py:59 and called at :262.
 * waveform (N,1,S), masks (N,Fw) or NULL -> (N,192); rows whose mask keeps fewer than 640
 * samples come back as NaN (they are dropped by clustering.py:143-145).  The mask selects
 * samples (nearest resampling, > 0.5), rows are zero padded to the longest row of the call and
 * the relative lengths drive the sentence normalisation, the squeeze-excitation means and the
 * attentive statistics pooling exactly as speechbrain's encode_batch does.                  */
typedef struct {
    const float* w;   /* [Npad][Kpad] packed like every convgemm weight                      */
    const float* b;   /* [Npad] bias                                                          */
    const float* s;   /* [Npad] folded BatchNorm scale (NULL if the layer has no norm)        */
    const float* h;   /* [Npad] folded BatchNorm shift                                        */
    const void* wsplit; /* optional split-f16 planes of w: the layer then runs on the f16 matrix cores.  Row-major
                           [2][Npad][Kpad] for block0, the Res2Net convolutions, asp_tdnn and asp_conv (dz_k_gemm_split);
                           kb-major [2][Kpad / 32][Npad][32] for the wide 1 x 1 layers tdnn1, tdnn2 and mfa, which
                           read pre-split activations (dz_k_gemm_pre, see dz_convgemm_desc.Xsplit)       */
} dz_layer;
typedef struct {
    dz_layer tdnn1;    /* 1x1, 1024 -> 1024                                                   */
    dz_layer res[7];   /* Res2Net: 128 -> 128, k = 3, dilation d, reflect "same" padding      */
    dz_layer tdnn2;    /* 1x1                                                                  */
    dz_layer se1;      /* [128][1024]  squeeze                                                 */
    dz_layer se2;      /* [1024][128]  excite                                                  */
} dz_seres2net;
typedef struct {
    const float* dft;      /* [448][416] hamming-windowed DFT: rows 0..200 cos, 201..401 sin  */
    const float* mel;      /* [128][224] triangular mel bank, [mel][bin], zero padded         */
    dz_layer block0;       /* [1024][416], k = tap*80 + mel                                    */
    dz_seres2net ser[3];   /* dilations 2, 3, 4                                                */
    dz_layer mfa;          /* [3072][3072]                                                     */
    dz_layer asp_tdnn;     /* w = columns of the 9216-wide input that multiply x: [128][3072]  */
    const float* asp_wms;  /* [128][6144] columns that multiply the global (mean | std)        */
    dz_layer asp_conv;     /* [3072][128]                                                      */
    dz_layer fc;           /* [192][6144] with asp_bn folded in                                */
    const float* zeros;    /* [6144] zeros                                                     */
    const void* dft_split; /* optional split-f16 planes [2][512][416] of dft (zero padded rows)        */
} dz_ecapa_weights;
typedef struct dz_ecapa dz_ecapa;
int dz_ecapa_frames_for(int num_samples);   /* 1 + S / 160 */
int dz_ecapa_create(dz_ctx* ctx, const dz_ecapa_weights* w, int max_rows, int num_samples,
                    dz_ecapa** out);
int dz_ecapa_forward(dz_ecapa* e, const float* d_wave, long long wave_stride, const float* d_masks,
                     int n_rows, int mask_frames, float* d_out, void* stream);
/* The same network over n_groups independent groups of rows_per_group (K) rows, each group with its own batch
 * geometry: row r = g*K + k reads waveform row g (d_wave + g*wave_stride) and mask row r of d_masks (G,K,Fw)
 * contiguous (the speaker-major layout of dz_seg_forward_osp's weights) -> d_out (G*K, 192); normalize = 1
 * L2-normalises every row (NaN rows stay NaN).  A group's rows are what dz_ecapa_forward returns for those K
 * rows alone (a group whose rows are all too short gives NaN rows; no other group is affected).  The
 * geometry is derived on the device: the call does not synchronise, read device memory from the host or
 * allocate.  G*K <= max_rows.                                                                   */
int dz_ecapa_forward_groups(dz_ecapa* e, const float* d_wave, long long wave_stride, const float* d_masks,
                            int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                            void* stream);
/* device pointer + element count of an intermediate of the LAST forward (parity tests):
 * 0 features (N,T,80)  1 block0 (N,T,1024)  2 ASP logits (N,T,3072; the concatenation's buffer,
 * which holds the attention logits once a forward has returned)  3 mfa (N,T,3072)
 * 4 pooled (N,6144)    5 kept-sample counts (N) as int32, -(count + 1) for a row whose kept
 * samples hold a NaN / Inf (its embedding is NaN)  6 nvalid (N) as int32: frames of the sentence
 * mean, round(float32(len / lmax) * T)  7 nmask (N) as int32: frames of the squeeze-excitation
 * mean and the attentive pooling, #{t : t < float32(len / lmax) * T} (6 and 7 are 0 when every
 * row is too short);  *frames receives T.
 * After dz_ecapa_forward_groups: N = G*K, T = the handle's Tc = 1 + num_samples / 160 and buffers 0 - 3 are
 * Tc-strided (frames at or past a row's own count are padding); 6 / 7 are each group's values as
 * dz_ecapa_forward computes them for that group alone (0 for a group whose rows are all too short), and
 * 8 is the per-row frame count of its group, 1 + lmax_g / 160, as int32 (N) (0 for such a group).
 * Buffer 8 exists after a groups forward only.                                             */
int dz_ecapa_peek(dz_ecapa* e, int which, const void** d_ptr, long long* count, int* frames);
int dz_ecapa_destroy(dz_ecapa* e);

/* ---- mel-spectrogram ECAPA-TDNN (speechbrain/spkrec-ecapa-voxceleb-mel-spec) behind the same masked call:
 * waveform (N,1,S), masks (N,Fw) or NULL -> (N,192), not normalised.  The network is dz_ecapa's (net); the front
 * end is torchaudio's MelSpectrogram as speechbrain's HifiGAN mel_spectogram sets it up — n_fft = win_length = 1024,
 * hop 256, periodic Hann, centred with reflect padding of the batch zero-padded to the longest kept row lmax of the
 * call (of the group, for dz_ecm_forward_groups), magnitude, 80 slaney mel bins — then log(max(x, 1e-5)) and the
 * sentence mean over round(float32(len / lmax) * T) frames, T = 1 + lmax / 256.  Rows below min_num_samples (or with
 * a NaN / Inf kept sample) are NaN, a group whose longest row is below it is all NaN.  DESIGN.md 4.15.             */
typedef struct {
    dz_ecapa_weights net;   /* block0 .. fc and zeros as dz_ecapa_weights; its dft / mel / dft_split are not read */
    const float* dft;       /* [1152][1024] Hann-windowed DFT: rows 0..512 cos, 513..1025 sin, zero rows behind   */
    const void* dft_split;  /* optional split-f16 planes [2][1152][1024] of dft: the STFT then runs on dz_k_gemm_split */
    const float* mel;       /* [128][544] slaney mel bank [mel][bin], zero padded                                  */
    int min_num_samples;    /* > 512 (the reflect padding of the STFT)                                             */
} dz_ecm_weights;
typedef struct dz_ecm dz_ecm;
int dz_ecm_abi_size(void);                /* sizeof(dz_ecm_weights) of the library */
int dz_ecm_frames_for(int num_samples);   /* 1 + S / 256 */
int dz_ecm_create(dz_ctx* ctx, const dz_ecm_weights* w, int max_rows, int num_samples, dz_ecm** out);
/* one call of n_rows rows = one group: no synchronisation, the geometry is derived on the device */
int dz_ecm_forward(dz_ecm* m, const float* d_wave, long long wave_stride, const float* d_masks, int n_rows,
                   int mask_frames, float* d_out, void* stream);
/* n_groups groups of rows_per_group (K) rows as dz_ecapa_forward_groups: row g*K + k reads waveform row g and mask
 * row g*K + k -> d_out (G*K, 192).  A group's rows are what dz_ecm_forward returns for those K rows alone.         */
int dz_ecm_forward_groups(dz_ecm* m, const float* d_wave, long long wave_stride, const float* d_masks,
                          int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                          void* stream);
/* intermediates of the LAST forward, every buffer laid out with the handle's Tc = 1 + num_samples / 256 frames per
 * row (*frames receives Tc; frames at or past a row's own count, buffer 8, are padding):  0 features (N,Tc,80)
 * 1 block0 (N,Tc,1024)  2 ASP logits (N,Tc,3072)  3 mfa (N,Tc,3072)  4 pooled (N,6144)  5 kept-sample counts (N)
 * int32, -(count + 1) for a row with a NaN / Inf sample  6 nvalid (N) int32  7 nmask (N) int32  8 the row's frame
 * count 1 + lmax / 256 of its group (N) int32 (6 - 8 are 0 for a group whose rows are all too short)  9 lmax of
 * the row's group (N) int32  10 the magnitude spectrum (N,Tc,544), bins 0..512, zeros behind.                    */
int dz_ecm_peek(dz_ecm* m, int which, const void** d_ptr, long long* count, int* frames);
int dz_ecm_destroy(dz_ecm* m);

/* ---- WeSpeaker ResNet34 embedding (pyannote/wespeaker-voxceleb-resnet34-LM, pyannote.audio 3.1's
 * WeSpeakerResNet34): the callable behind EmbeddingModel.__call__ for that checkpoint, reached in the reference
 * through PyannoteLoader (diart src/diart/models.py:42-59) and called as
 * model(waveform (N,1,S), weights (N,Fw)) (blocks/embedding.py:56-65).
 * kaldi fbank (80 mel bins, 25 / 10 ms, waveform x 2^15, mean over frames subtracted per row) -> ResNet34 trunk
 * (3x3 convolutions with folded BatchNorm, BasicBlocks [3, 4, 6, 3] at 32 / 64 / 128 / 256 channels, strides
 * 1 / 2 / 2 / 2) -> TSTP statistics pooling of the (256 x 10) x T4 features -> Linear(5120, 256).  Activations are
 * channels-last [row][f][t][c].  A row with a NaN / Inf sample in any of its frames comes back as a NaN row.  */
typedef struct {
    const float* w;      /* [Cout][taps * Cin], k = (kh * 3 + kw) * Cin + c (taps 9) or c (taps 1), BatchNorm folded */
    const float* b;      /* [Cout] folded BatchNorm bias                                                  */
    const void* wsplit;  /* split-f16 planes [2][Cout][taps * Cin] of w: the layer then runs on the f16 matrix cores
                            (three products per pair); NULL: exact-f32 matrix cores                         */
} dz_wsp_conv;
typedef struct {
    const float* mel;           /* [80][257] kaldi mel bank (the Nyquist column is zero)                      */
    dz_wsp_conv conv1;          /* [32][9]: 3x3, 1 -> 32 (w / b only; direct f32 kernel)                      */
    dz_wsp_conv block[16][3];   /* BasicBlocks of layers 1 - 4 in order: conv1 (3x3), conv2 (3x3), shortcut
                                   (1x1, stride 2; w NULL where the shortcut is the identity)                */
    const float* seg_w;         /* [256][5120] seg_1, input index c * 10 + f (mean) | 2560 + c * 10 + f (std) */
    const float* seg_b;         /* [256]                                                                     */
} dz_wsp_weights;
typedef struct dz_wsp dz_wsp;
/* sizeof(dz_wsp_weights): a binding checks its mirror against the library it loaded */
int dz_wsp_abi_size(void);
/* frames of stage `stage` for num_samples samples: 0 = fbank, 1 + (S - 400) / 160 (0 when S < 400); 1 .. 4 = the
 * time axis after layer 1 .. 4 ((T - 1) / stride + 1 per strided layer); -1 on a bad stage                   */
int dz_wsp_frames_for(int num_samples, int stage);
int dz_wsp_create(dz_ctx* ctx, const dz_wsp_weights* w, int max_rows, int num_samples, dz_wsp** out);
/* n_rows rows (d_wave + r * wave_stride) -> d_out (n_rows, 256); d_weights (n_rows, weight_frames) or NULL   */
int dz_wsp_forward(dz_wsp* m, const float* d_wave, long long wave_stride, const float* d_weights, int n_rows,
                   int weight_frames, float* d_out, void* stream);
/* batch windows, num_speakers (K <= 8) weight rows each ((batch, K, weight_frames) speaker-major, contiguous) ->
 * d_out (batch * K, 256): the trunk runs once per window and is pooled K times; normalize = 1 L2-normalises every
 * row (NaN rows stay NaN).  Row b * K + k equals dz_wsp_forward of window b with weight row (b, k).           */
int dz_wsp_forward_multi(dz_wsp* m, const float* d_wave, long long wave_stride, const float* d_weights, int batch,
                         int num_speakers, int weight_frames, int normalize, float* d_out, void* stream);
/* dz_wsp_forward_multi in two halves, for a caller whose weights come from a network that runs beside the trunk
 * (the N-stream engine: the trunk does not depend on the segmentation, only the pooling does).  dz_wsp_forward_multi
 * is exactly dz_wsp_trunk followed by dz_wsp_pool on one stream: the results are the same bits.
 * fbank -> conv1 -> layers 1 - 4 of `batch` windows, into the handle; independent of any weights              */
int dz_wsp_trunk(dz_wsp* m, const float* d_wave, long long wave_stride, int batch, void* stream);
/* TSTP pooling (K weight rows per window) + seg_1 (+ L2 normalisation) of the handle's LAST trunk -> d_out
 * (batch * K, 256); `batch` must be that trunk's batch, otherwise an error and no launch.  The two halves go on one
 * HIP stream, or on two that the caller orders with an event (pool after trunk).  ONE handle carries ONE trunk at a
 * time: its activations and its per-row NaN flags stay in the handle between the halves, so the next dz_wsp_trunk
 * (or dz_wsp_forward / _multi) on the handle is enqueued behind the pooling of the previous one.               */
int dz_wsp_pool(dz_wsp* m, const float* d_weights, int batch, int num_speakers, int weight_frames, int normalize,
                float* d_out, void* stream);
/* device pointer + element count of an intermediate of the LAST forward or half (parity tests); *frames receives the
 * buffer's time axis:  0 fbank (N,80,T) after the mean subtraction  1 conv1 (N,80,T,32)  2 .. 5 layer 1 .. 4
 * (N,F,T_l,C_l)  6 pooled statistics (rows, 5120)  7 fbank (N,80,T) before the mean subtraction             */
int dz_wsp_peek(dz_wsp* m, int which, const void** d_ptr, long long* count, int* frames);
int dz_wsp_destroy(dz_wsp* m);
/* one 2-D convolution of the trunk alone (k_conv2d.hip; parity tests): channels-last d_x [batch][fi][ti][cin] ->
 * d_y [batch][fo][to][cout], fo = (fi - 1) / stride + 1, to likewise; taps 9 = 3x3 with zero padding 1, taps 1 = 1x1
 * without; d_w / d_wsplit as dz_wsp_conv (d_wsplit set: split-f16 matrix cores); epilogue + d_bias[n], + d_r[m][n]
 * when d_r is set, ReLU when relu.  cin % 32 == 0, cout 32, 64 or a multiple of 128, stride 1 or 2; an operand of
 * the split path outside +-65504 raises the context's range flag (dz_range_check)                        */
int dz_k_conv2d(dz_ctx* ctx, const float* d_x, const float* d_w, const void* d_wsplit, const float* d_bias,
                const float* d_r, float* d_y, int batch, int fi, int ti, int cin, int cout, int taps, int stride,
                int relu, void* stream);

/* ---- speechbrain x-vector embedding (speechbrain/spkrec-xvect-voxceleb) behind pyannote's
 * PretrainedSpeakerEmbedding contract, like ECAPA: waveform (N,1,S), masks (N,Fw) or NULL -> (N,512).
 * The mask selects samples (nearest resampling, > 0.5), rows are zero padded to the longest kept row of the
 * call (of the group, for dz_sbx_forward_groups) and the relative lengths drive the sentence mean and the
 * statistics pooling.  Fbank(24 mel bins) -> sentence mean normalisation -> 5 TDNN layers (Conv1d with reflect
 * "same" padding -> LeakyReLU(0.01) -> BatchNorm1d) -> StatisticsPooling (mean + 5e-5, unbiased std + 1e-5 over
 * round(rel * T) frames) -> Linear(3000, 512).  Rows that keep fewer than 480 samples, or whose kept samples hold
 * a NaN / Inf, come back as NaN.  Activations are channels-last [row][t][c].                                  */
typedef struct {
    const float* dft;       /* [448][416] hamming-windowed DFT: rows 0..200 cos, 201..401 sin (as dz_ecapa_weights) */
    const void* dft_split;  /* optional split-f16 planes [2][512][416] of dft                                      */
    const float* mel;       /* [64][224] triangular mel bank, [mel][bin], 24 mel rows, zero padded                  */
    dz_layer tdnn[5];       /* w [Npad][Kpad], k = tap * Cin + c: [512][128] (k5, Cin 24), [512][1536] (k3),
                               [512][1536] (k3), [512][512], [1536][512]; b / s / h [Npad] (BatchNorm folded, after
                               the LeakyReLU); wsplit: optional row-major split-f16 planes [2][Npad][Kpad]          */
    const float* lin_w;     /* [512][3008] Linear(3000, 512), input (mean | std), zero padded columns               */
    const float* lin_b;     /* [512]                                                                              */
    const float* zeros;     /* [1536] zeros (the bias of the DFT and mel layers)                                  */
} dz_sbx_weights;
typedef struct dz_sbx dz_sbx;
/* sizeof(dz_sbx_weights): a binding checks its mirror against the library it loaded */
int dz_sbx_abi_size(void);
int dz_sbx_create(dz_ctx* ctx, const dz_sbx_weights* w, int max_rows, int num_samples, dz_sbx** out);
/* n_rows rows (d_wave + r * wave_stride), d_masks (n_rows, mask_frames) or NULL -> d_out (n_rows, 512): one batch
 * geometry over all n_rows rows (pyannote's call).  Derived on the device: no synchronisation.                */
int dz_sbx_forward(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks, int n_rows,
                   int mask_frames, float* d_out, void* stream);
/* n_groups groups of rows_per_group (K) rows, each group with its own batch geometry, as
 * dz_ecapa_forward_groups: row g*K + k reads waveform row g and mask row g*K + k ((G,K,Fw) contiguous) ->
 * d_out (G*K, 512); normalize = 1 L2-normalises every row (NaN rows stay NaN).  A group's rows are what
 * dz_sbx_forward returns for those K rows alone.  No synchronisation, no allocation.  G*K <= max_rows.          */
int dz_sbx_forward_groups(dz_sbx* m, const float* d_wave, long long wave_stride, const float* d_masks,
                          int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                          void* stream);
/* device pointer + element count of an intermediate of the LAST forward (parity tests); every buffer is laid out
 * with the handle's Tc = 1 + num_samples / 160 frames per row (*frames receives Tc); frames at or past a row's own
 * count (buffer 9) are padding:  0 features (N,Tc,24)  1 .. 4 TDNN layers 1 - 4 (N,Tc,512)  5 TDNN layer 5
 * (N,Tc,1500)  6 pooled statistics (N,3000)  7 kept-sample counts (N) as int32, -(count + 1) for a row with a
 * NaN / Inf sample  8 nvalid (N) as int32, round(float32(len / lmax) * T)  9 the row's frame count T =
 * 1 + lmax / 160 of its group (N) as int32 (8 and 9 are 0 for a group whose rows are all too short).          */
int dz_sbx_peek(dz_sbx* m, int which, const void** d_ptr, long long* count, int* frames);
int dz_sbx_destroy(dz_sbx* m);

/* ---- NeMo TitaNet-L (nvidia/speakerverification_en_titanet_large) behind pyannote's PretrainedSpeakerEmbedding
 * contract (its NeMo wrapper): waveform (N,1,S), masks (N,Fw) or NULL -> (N,192), not normalised.  The mask
 * selects samples (nearest resampling, > 0.5); a row's valid frames come from its OWN kept count and every layer
 * masks its input at them, so a row depends on its group only through the reflect padding at the group's longest
 * row and through the "too short" rules: rows below min_num_samples are NaN, a group whose longest row is below it
 * is all NaN.  Pre-emphasis 0.97 -> STFT (n_fft 512, Hann 400, hop 160, centred) -> 80 slaney mel bins ->
 * log(x + 2^-24) -> per-feature mean / unbiased std over the valid frames -> 5 separable Jasper blocks with masked
 * squeeze-excitation (depthwise conv: k_titanet.hip; pointwise conv with its BatchNorm folded: the wide GEMMs) ->
 * attentive statistics pooling -> BatchNorm1d(6144) folded into Conv1d(6144, 192, 1).  DESIGN.md 4.12.          */
typedef struct {
    const float* dw;        /* depthwise taps [taps][Cpad], tap-major; Cpad = 96 for block 0 (80 mel bins), else 1024 */
    dz_layer pw;            /* pointwise conv x BatchNorm scale: w [Cout][Cpad], b [Cout] = BatchNorm shift; wsplit:
                               optional kb-major split-f16 planes of w (k_gemm_pre)                                   */
} dz_ttn_sep;
typedef struct {
    dz_ttn_sep rep[3];      /* the block's repeats (1 for blocks 0 and 4, 3 for blocks 1 .. 3)                      */
    const float* se1;       /* [C / 8][C]  squeeze: Linear(C, C / 8).weight                                         */
    const float* se2t;      /* [C / 8][C]  excite: Linear(C / 8, C).weight TRANSPOSED                               */
    dz_layer res;           /* blocks 1 .. 3: residual 1 x 1 conv x BatchNorm, as pw                                */
} dz_ttn_block;
typedef struct {
    const float* dft;       /* [640][416] Hann(400)-windowed 512-point DFT of the 400 samples a frame's window
                               covers: rows 0..256 cos, 257..513 sin                                                */
    const void* dft_split;  /* optional split-f16 planes [2][640][416] of dft                                       */
    const float* mel;       /* [128][288] slaney mel bank, [mel][bin], 80 mel rows x 257 bins, zero padded          */
    dz_ttn_block block[5];
    dz_layer asp_tdnn;      /* [128][3072]: the columns of the 9216-wide attention conv that multiply x; s / h =
                               its BatchNorm (after the ReLU)                                                       */
    const float* asp_wms;   /* [128][6144]: the columns that multiply (mean | std)                                  */
    dz_layer asp_conv;      /* [3072][128]                                                                          */
    dz_layer fc;            /* [192][6144] with BatchNorm1d(6144) folded in                                         */
    const float* zeros;     /* [6144] zeros                                                                         */
    int pad_reflect;        /* centred STFT padding: 1 reflect (at the group's longest row), 0 zeros                */
    int frame_pad, frame_nfft;   /* valid frames of len samples = (len + 2 frame_pad - frame_nfft) / 160 + 1        */
    int min_num_samples;    /* >= 201 (the reflect padding reads 200 samples back)                                  */
} dz_ttn_weights;
typedef struct dz_ttn dz_ttn;
int dz_ttn_abi_size(void);                    /* sizeof(dz_ttn_weights) */
int dz_ttn_frames_for(int num_samples);       /* 1 + S / 160: frames every buffer lays a row out with */
int dz_ttn_create(dz_ctx* ctx, const dz_ttn_weights* w, int max_rows, int num_samples, dz_ttn** out);
/* n_rows rows as one group (pyannote's call), d_masks (n_rows, mask_frames) or NULL -> d_out (n_rows, 192).  The
 * geometry is derived on the device: no synchronisation.                                                        */
int dz_ttn_forward(dz_ttn* m, const float* d_wave, long long wave_stride, const float* d_masks, int n_rows,
                   int mask_frames, float* d_out, void* stream);
/* n_groups groups of rows_per_group (K) rows as dz_ecapa_forward_groups: row g*K + k reads waveform row g and mask
 * row g*K + k -> d_out (G*K, 192); normalize = 1 L2-normalises every row.  A group's rows are bit-identical to
 * dz_ttn_forward on those K rows alone.  No synchronisation, no allocation.  G*K <= max_rows.                  */
int dz_ttn_forward_groups(dz_ttn* m, const float* d_wave, long long wave_stride, const float* d_masks,
                          int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                          void* stream);
/* intermediates of the LAST forward, rows laid out with Tc = dz_ttn_frames_for(num_samples) frames (*frames); frames
 * at or past a row's own count (buffer 9) are padding:  0 features (N,Tc,80)  1 .. 4 blocks 0 - 3 (N,Tc,1024)
 * 5 block 4 (N,Tc,3072)  6 pooled statistics (N,6144)  7 kept-sample counts (N) int32, -(count + 1) for a row with
 * a NaN / Inf sample  8 the length the row is padded at (its group's longest row) (N) int32  9 valid frames (N) int32 */
int dz_ttn_peek(dz_ttn* m, int which, const void** d_ptr, long long* count, int* frames);
int dz_ttn_destroy(dz_ttn* m);
/* the depthwise convolution alone (parity tests): x [rows][T][ldx] f32 channels-last with C channels (C % 32 == 0,
 * ldx % 4 == 0, ldx >= C), taps in {1, 3, 7, 11, 15} as [taps][C], frames[rows] valid frames per row (input frames
 * at or past them read as zero), relu = 1 applies ReLU to the input first -> y [rows][T][C] f32 when d_planes is
 * NULL, else the kb-major split-f16 planes [2][C / 32][rows T][32] of the same values.  d_x, d_taps, d_y and
 * d_planes are 16-byte aligned (the kernel moves 16 bytes per lane).                                                */
int dz_k_ttn_depthwise(dz_ctx* ctx, const float* d_x, int ldx, const float* d_taps, int taps, const int* d_frames,
                       int rows, int T, int C, int relu, float* d_y, void* d_planes, void* stream);

/* ---- speechbrain ResNet speaker embedding (speechbrain/spkrec-resnet-voxceleb) behind pyannote's
 * PretrainedSpeakerEmbedding contract, like ECAPA and the speechbrain x-vector: waveform (N,1,S), masks (N,Fw) or
 * NULL -> (N,256), not normalised.  The mask selects samples (nearest resampling, > 0.5), rows are zero padded to the
 * longest kept row of the call (of the group, for dz_sbr_forward_groups): T_g = 1 + lmax / 160 frames.  ECAPA's
 * Fbank(80) + sentence mean -> Conv2d(1, C0, 3) + BatchNorm + ReLU -> four layers of SEBasicBlocks (3x3 convolutions
 * with folded BatchNorm, squeeze-excitation over every position of the padded batch, both axes strided) ->
 * attentive statistics pooling over the T4_g frames of the F4 C4 channels -> BatchNorm1d -> Linear -> BatchNorm1d
 * (both folded into the Linear).  The network does not use the relative lengths: a row depends on its group through
 * T_g only.  Activations are channels-last [row][t][f][c]; every buffer lays a row out with the handle's
 * Tc = 1 + num_samples / 160 steps (halved, rounding up, per strided layer) and holds zeros at or past the row's own.
 * Rows that keep fewer than min_num_samples samples, or whose kept samples hold a NaN / Inf, come back as NaN; a
 * group whose longest row is that short is all NaN.  DESIGN.md 4.18.                                              */
enum { DZ_SBR_MAX_BLOCKS = 32 };
typedef struct {
    dz_wsp_conv conv[3];    /* conv1 (3x3, stride), conv2 (3x3), downsample (1x1, stride; w NULL: identity), BatchNorm folded */
    const float* se_w1t;    /* [C][Cr]  se.fc.0.weight transposed                                                    */
    const float* se_b1;     /* [Cr]                                                                                  */
    const float* se_w2t;    /* [Cr][C]  se.fc.2.weight transposed                                                    */
    const float* se_b2;     /* [C]                                                                                   */
    int width, se_width;    /* C, Cr                                                                                 */
    int stride;             /* of conv1 and the downsample, on both axes                                             */
    int layer;              /* 0 .. 3                                                                                */
} dz_sbr_block;
typedef struct {
    const float* dft;       /* [448][416] hamming-windowed DFT (as dz_ecapa_weights)                                 */
    const void* dft_split;  /* optional split-f16 planes [2][512][416] of dft                                        */
    const float* mel;       /* [128][224] triangular mel bank, 80 mel rows (as dz_ecapa_weights)                     */
    const float* stem_w;    /* [C0][9], k = kt * 3 + kf: conv1 x bn1 scale                                           */
    const float* stem_b;    /* [C0]: (conv1.bias - running_mean) x scale + bn1.bias                                  */
    dz_sbr_block block[DZ_SBR_MAX_BLOCKS];
    dz_layer att1;          /* attention.0 [128][F4 C4] with the columns in this layout's order f C4 + c; s / h =
                               attention.2 (BatchNorm after the ReLU); wsplit: optional row-major split-f16 planes   */
    dz_layer att2;          /* attention.3 [Npad][128], rows f C4 + c, Npad = F4 C4 rounded up to 128                */
    dz_layer fc;            /* [256][2 F4 C4]: norm_stats, fc_embed and norm_embed folded; columns mu | sg           */
    const float* zeros;     /* [512] zeros (the bias of the DFT and mel layers)                                      */
    int n_blocks;
    int stem_width;         /* C0                                                                                    */
    int min_num_samples;    /* >= 1                                                                                  */
    int rows_per_pass;      /* the trunk runs over at most this many rows at a time (0: 32); no result depends on it */
} dz_sbr_weights;
typedef struct dz_sbr dz_sbr;
int dz_sbr_abi_size(void);                    /* sizeof(dz_sbr_weights) */
int dz_sbr_create(dz_ctx* ctx, const dz_sbr_weights* w, int max_rows, int num_samples, dz_sbr** out);
/* n_rows rows as one group (pyannote's call), d_masks (n_rows, mask_frames) or NULL -> d_out (n_rows, 256).  The
 * geometry is derived on the device: no synchronisation.                                                        */
int dz_sbr_forward(dz_sbr* m, const float* d_wave, long long wave_stride, const float* d_masks, int n_rows,
                   int mask_frames, float* d_out, void* stream);
/* n_groups groups of rows_per_group (K) rows as dz_ecapa_forward_groups: row g*K + k reads waveform row g and mask
 * row g*K + k -> d_out (G*K, 256); normalize = 1 L2-normalises every row.  A group's rows are bit-identical to
 * dz_sbr_forward on those K rows alone.  No synchronisation, no allocation.  G*K <= max_rows.                  */
int dz_sbr_forward_groups(dz_sbr* m, const float* d_wave, long long wave_stride, const float* d_masks,
                          int n_groups, int rows_per_group, int mask_frames, int normalize, float* d_out,
                          void* stream);
/* intermediates of the LAST forward (parity tests); *frames receives the buffer's steps per row.  0 features
 * (N,Tc,80)  6 pooled statistics (N, 2 F4 C4) = mu | sg  7 kept-sample counts (N) int32, -(count + 1) for a row
 * with a NaN / Inf sample  8 the group's frame count T_g (N) int32 (0 for a group whose rows are all too short)
 * 9 live steps (5,N) int32 at the stem and after layers 1 .. 4.  The trunk's buffers hold the rows of the last pass
 * (all N rows when N <= rows_per_pass): 1 the stem (n,Tc,80,C0)  2 .. 5 layers 1 .. 4 (n,T_l,F_l,C_l).            */
int dz_sbr_peek(dz_sbr* m, int which, const void** d_ptr, long long* count, int* frames);
int dz_sbr_destroy(dz_sbr* m);
/* dz_k_conv2d's masked instances (k_conv2d.hip; parity tests): d_ext [batch] int32, row b is live for its first
 * d_ext[b] <= fo steps of the f axis; every output at or past them is stored as exactly 0.0.                     */
int dz_k_conv2d_masked(dz_ctx* ctx, const float* d_x, const float* d_w, const void* d_wsplit, const float* d_bias,
                       const float* d_r, const int* d_ext, float* d_y, int batch, int fi, int ti, int cin, int cout,
                       int taps, int stride, int relu, void* stream);
/* the kernels of k_sb_resnet.hip alone (parity tests), activations [rows][tb][f][c], d_ext [rows] int32 live steps:
 * squeeze-excitation gate of d_y -> d_gate (rows, c) through d_part (rows, 16, c) scratch; d_out = ReLU(gate y + r)
 * masked (d_out may be d_y); attention pooling of d_x / d_logits (rows, tb, c) -> d_pooled (rows, 2 c)           */
int dz_k_sbr_se_gate(dz_ctx* ctx, const float* d_y, int rows, int tb, int f, int c, int cr, const int* d_ext,
                     const float* d_w1t, const float* d_b1, const float* d_w2t, const float* d_b2, float* d_part,
                     float* d_gate, void* stream);
int dz_k_sbr_se_apply(dz_ctx* ctx, const float* d_y, const float* d_gate, const float* d_r, int rows, int tb, int f,
                      int c, const int* d_ext, float* d_out, void* stream);
int dz_k_sbr_att_pool(dz_ctx* ctx, const float* d_x, const float* d_logits, int rows, int tb, int c, const int* d_ext,
                      float* d_pooled, void* stream);

/* ---- band-limited resampling: torchaudio's sinc_interp_hann (lowpass_filter_width 6, rolloff 0.99), the filter
 * built in float64 and rounded to float32.  g = gcd(orig, new), o = orig / g, n = new / g, width =
 * ceil(6 o / (0.99 min(o, n))), T = 2 width + o taps per phase; output m = j n + i is sum_k h[i][k] x[j o - width + k]
 * (x = 0 outside the row), ceil(n L / o) outputs for L inputs.  Each output is one fused-multiply-add chain over
 * its T taps in ascending k: a row's outputs do not depend on the batch it comes in.  Ratios whose table exceeds
 * 16 MiB and rates <= 0 are refused (return 2).  Equal rates: the input unchanged.                           */
typedef struct dz_resample dz_resample;
/* host only: phases n, taps T, width and input step o of orig -> new                                           */
int dz_resample_geometry(int orig_freq, int new_freq, int* phases, int* taps, int* width, int* in_step);
/* host only: output length for in_len input samples (in_len at equal rates); -1 on bad rates or overflow       */
long long dz_resample_out_len(int orig_freq, int new_freq, long long in_len);
/* host only: the float32 filter table, phase-major [n][T]                                                      */
int dz_resample_table(int orig_freq, int new_freq, float* out);
/* uploads the table to the context's GPU                                                                       */
int dz_resample_create(dz_ctx* ctx, int orig_freq, int new_freq, dz_resample** out);
/* rows signals of in_len samples (d_in + r * in_stride) -> d_out + r * out_stride, dz_resample_out_len samples
 * each.  Enqueued on `stream`; no synchronisation, no allocation.                                               */
int dz_resample_forward(dz_resample* m, const float* d_in, long long in_stride, long long in_len, int rows,
                        float* d_out, long long out_stride, void* stream);
int dz_resample_destroy(dz_resample* m);

/* ---- volume adjustment: the reference's AdjustVolume block (blocks/utils.py:92-137; csrc/k_volume.hip).  A row is
 * samples * channels interleaved float32 values; rows at any float address, any stride >= that size.  Per (row,
 * channel) signal x: volume = 10 log10(mean(x^2)) (squares in f32, summed in f64), gain = fl32(10^((target_db - volume)
 * / 20)), m = max(fl32(gain max|x|), 1), out = fl32(fl32(gain x) / m).  As in the reference a signal of zero energy, or
 * with a NaN / Inf sample, comes out all NaN.  A signal's bits do not depend on its alignment, its place in the call or
 * the other rows; no atomics.  d_out == d_in with equal strides is in place.  rows, samples >= 1, 1 <= channels <= 8,
 * finite target_db (else return 2, nothing launched).  Enqueued on `stream`; no handle, no allocation.                */
int dz_adjust_volume(dz_ctx* ctx, const float* d_in, long long in_row_stride, float* d_out, long long out_row_stride,
                     int rows, long long samples, int channels, double target_db, void* stream);

/* ---- OverlappedSpeechPenalty: functional.py:6-13 + blocks/embedding.py:98-107
 * d_seg (B,F,K) -> weights.  speaker_major=0: (B,F,K) like the reference block;
 * speaker_major=1: (B,K,F), the layout dz_emb_forward_multi consumes.           */
int dz_osp(dz_ctx* ctx, const float* d_seg, int batch, int frames, int speakers,
           float gamma, float beta, int normalize, int speaker_major,
           float* d_out, void* stream);

/* ---- the `.cpu()` of blocks/segmentation.py:47 and blocks/embedding.py:68 for a whole step: two device
 * buffers (n_a, n_b floats; n_b may be 0) -> two PINNED host buffers in one kernel launch on `stream`
 * (device stores over the host link; all four pointers 16-byte aligned).  Not hipMemcpyAsync: that call
 * now and then blocks its caller for a whole step's latency (csrc/ring.hip).  Complete when an event
 * recorded on `stream` behind it has fired.                                                       */
int dz_results_to_host(dz_ctx* ctx, const float* d_a, float* h_a, long long n_a,
                       const float* d_b, float* h_b, long long n_b, void* stream);

/* ---- EmbeddingNormalization(norm): functional.py:16-27; rows (R,D) in place  */
int dz_l2_normalize(dz_ctx* ctx, float* d_emb, int rows, int dim, float norm, void* stream);

/* ---- cosine distances for N streams at once: mapping.py:171-176 (scipy cdist,
 * fp64).  d_emb (N,K,D) f32, d_centers (N,G,D) f64 -> d_out (N,K,G) f64.        */
int dz_cdist_cosine(dz_ctx* ctx, const float* d_emb, const double* d_centers,
                    int n_streams, int k_local, int g_global, int dim,
                    double* d_out, void* stream);

/* ---- speaker gallery: the nearest enrolled voiceprint of embedding rows (csrc/k_gallery.hip).
 * The reference has no such step.  A gallery is E voiceprints of D floats, STORED NORMALISED: dz_gallery_create divides
 * each host row by its float64 norm, rounds to float32 once and uploads.  dz_gallery_match takes R rows of D floats on
 * the device, row_stride >= D floats apart at any 4-byte address (16-byte loads where base and stride allow, single
 * floats otherwise; the same bits either way), and writes per row
 *     index_out  (int32) the voiceprint of the smallest cosine distance 1 - x.g / (|x| |g|), the LOWEST index among
 *                equal distances; dist_out (f32) that distance; second_out (f32) the smallest distance among the other
 *                voiceprints (+inf when E == 1).
 * A row with a NaN / Inf element, of zero norm or of a norm beyond float32 gets -1 / NaN / NaN and touches no other row.
 * The dot products run on the exact-f32 matrix instructions, every (row, voiceprint) pair in one fixed k order, and the
 * division is by the row's norm (summed in float64) alone: the distance bits of a pair depend on the two vectors only,
 * not on R, E, the voiceprint's place in the gallery, the row's alignment or the rows it is batched with.  Each
 * distance is within (D + 8) 2^-24 of the float64 value.  No atomics: (row tile, gallery tile) partial results go to
 * the handle's scratch and a second kernel folds them.  The three outputs may be device memory or pinned host memory
 * mapped into the device (plain stores from the kernel; complete when an event recorded on `stream` behind the call has
 * fired).  D: a multiple of 64 from 64 to 512; E: 1 .. 65536; R: 1 .. 4096.  Refused (status 2, the message names the
 * function, nothing is launched): NULL handle, rows or outputs; R, E or D out of range; a stride below D; a voiceprint
 * that is not finite or of zero norm.  The handle owns the scratch of ONE match (sized for R = 4096): two streams must
 * not run dz_gallery_match on the same handle at once; give each stream its own handle.  Enqueued on `stream`; no
 * synchronisation, no allocation.                                                                                    */
typedef struct dz_gallery dz_gallery;
int dz_gallery_create(dz_ctx* ctx, const float* voiceprints, int E, int D, dz_gallery** out);
int dz_gallery_destroy(dz_gallery* g);
int dz_gallery_size(dz_gallery* g);   /* E (0 for NULL) */
int dz_gallery_dim(dz_gallery* g);    /* D (0 for NULL) */
int dz_gallery_match(dz_gallery* g, const float* d_rows, long long row_stride, int R, int* index_out, float* dist_out,
                     float* second_out, void* stream);

/* ---- the match normalised against a cohort of impostors: adaptive s-norm (csrc/k_cohort.hip).
 * A cohort is M rows of D floats (1 <= M <= 8192), validated and stored like voiceprints (finite, of non-zero norm,
 * divided by the float64 norm, rounded to float32 once), and top_n in 1 .. M.  For a vector v, (mean, std)(v) are the
 * mean and the population standard deviation (never below 1e-3) of the top_n SMALLEST of its M cosine distances to the
 * cohort.  The normalised distance of row x and voiceprint g at raw distance d is
 *     dn = 0.5 ((d - mean(g)) / std(g) + (d - mean(x)) / std(x))
 * signed, lower is closer: minus the AS-norm score of the similarity 1 - d.
 *   dz_gallery_set_cohort    validates, uploads and computes the E voiceprints' statistics (synchronous; no match of
 *                            the handle may be in flight).  rows == NULL or M == 0 removes the cohort.
 *   dz_gallery_cohort_size   M (0: no cohort, or NULL).
 *   dz_gallery_cohort_stats  (mean, std) of R rows, rows and outputs as dz_gallery_match takes them.
 *   dz_gallery_entry_stats   the E voiceprints' (mean, std) to host memory (synchronous).
 *   dz_gallery_match_norm    dz_gallery_match with dn in the distance's place: index (lowest among equals), dn there,
 *                            the smallest dn among the other voiceprints (+inf when E == 1); -1 / NaN / NaN and NaN
 *                            statistics for an unusable row.  Same domain, outputs and one-match-per-handle rule.
 * dz_gallery_match stays the raw match on a handle with a cohort.  The bits of (mean, std) depend on the vector, the
 * stored cohort and top_n only; those of dn on the two vectors, the cohort and top_n only.  Each mean and std is
 * within (D + 8) 2^-24 + 2^-22 of the float64 value.  Scratch: at most 8 MiB beside the cohort (rows go in passes of
 * 256).  Status 2 (the message names the function, nothing is launched): NULL arguments; M outside 1 .. 8192; top_n
 * outside 1 .. M; a cohort row that is not finite or of zero norm (named by index); cohort_stats, entry_stats or
 * match_norm on a handle without a cohort; the row, stride and alignment checks of dz_gallery_match.              */
int dz_gallery_set_cohort(dz_gallery* g, const float* rows, int M, int top_n);
int dz_gallery_cohort_size(dz_gallery* g);
int dz_gallery_cohort_stats(dz_gallery* g, const float* d_rows, long long row_stride, int R, float* mean_out,
                            float* std_out, void* stream);
int dz_gallery_entry_stats(dz_gallery* g, float* mean_host, float* std_host);
int dz_gallery_match_norm(dz_gallery* g, const float* d_rows, long long row_stride, int R, int* index_out,
                          float* dist_out, float* second_out, void* stream);

/* ---- repeated rows (csrc/k_rows_repeat.hip) ---------------------------------
 * The reference's SpeakerEmbedding hands the model every waveform num_speakers times (blocks/embedding.py:56-59).
 * repeat_out receives the largest R >= 1 that divides n_rows and for which every row i with i % R != 0 is BITWISE equal
 * to row i - 1 (the gcd of n_rows and the lengths of the runs of equal rows; 1 = nothing to share): equal NaN patterns
 * are equal, -0.0 and +0.0 are not.  Rows of num_samples floats, wave_stride floats apart (any stride >= 0 and any
 * float address: 16-byte loads where the rows are 16-byte aligned, 4-byte loads elsewhere).
 * SYNCHRONOUS BY DESIGN: two kernels are enqueued on `stream`, then the call waits for `stream` and reads the four
 * bytes of the answer from pinned host memory; it cannot be captured into a graph.  The flags it works on belong to
 * the context; concurrent callers are serialised by a lock held until the wait is over.                          */
int dz_rows_repeat(dz_ctx* ctx, const float* d_wave, long long wave_stride, int n_rows, int num_samples,
                   void* stream, int* repeat_out);

/* ---- kernel-level entry points ---------------------------------------------
 * The building blocks of dz_seg_forward / dz_emb_forward, exported so that each HIP
 * kernel can be parity-tested on its own against a torch fp32 restatement of the same
 * op (tests/test_gpu_kernels.py).  Layouts: DESIGN.md §3.                          */
enum { DZ_EPI_BIAS = 0, DZ_EPI_BIAS_LEAKY = 1, DZ_EPI_BIAS_SIGMOID = 2, DZ_EPI_TDNN = 3,
       DZ_EPI_POOL3 = 4, DZ_EPI_BIAS_RELU = 5, DZ_EPI_RELU_BN = 6, DZ_EPI_RELU_BN_TANH = 7 };
typedef struct {
    const float* X;       /* [B][Tin][ldx] channels-last input                       */
    const float* W;       /* [Npad][Kpad], k = tap*Cin + c, zero padded              */
    const float* bias;    /* [Npad]                                                  */
    const float* e0;      /* TDNN: folded BatchNorm scale [Npad]                     */
    const float* e1;      /* TDNN: folded BatchNorm shift [Npad]                     */
    const float* nscale;  /* norm-on-load [B][nld] (InstanceNorm+LeakyReLU of input) */
    const float* nshift;
    float* Y;             /* [B][Tstore][ldy]                                        */
    float* partials;      /* POOL3: [B][ntile][Npad][2] (sum, sumsq) of pooled rows  */
    int B, Tin, Tout, Cin, taps, dil, K, Kpad, Npad, Nstore, ldx, ldy, nld, Tstore;
    long long xbs, ybs;   /* batch strides in floats                                 */
    int norm_on_load;     /* 0/1                                                     */
    int epi;              /* DZ_EPI_*                                                */
    int ksplit;           /* 0/1: off.  >1 (DZ_EPI_BIAS only): split z of the K loop writes its
                             partial sums to Y + z*ysplit (bias in split 0); the caller reduces */
    long long ysplit;     /* floats between the partial outputs of consecutive splits */
    int agroup;           /* activation tiles swept together per XCD (0 = default 4)  */
    int pad;              /* >0: "same" convolution, reflect padding of `pad` frames  */
    const float* X2;      /* optional second input with X's geometry, added on load   */
    const float* rowbias; /* optional [B][Npad] per-batch-item bias added to `bias`   */
    const void* Wsplit;   /* split-f16 path: W as two f16 planes [2][Npad][Kpad], hi = f16(W),
                             lo = f16((W - hi) * 2^11) (weights.py split_f16); NULL on the f32 path   */
    /* pre-split activations (k_gemm_pre.hip): the input as two f16 planes of R = xplane / ldx >= Tin rows
     * x ldx columns, hi at Xsplit, lo (scaled by 2^11) xplane ELEMENTS further, each plane in kb-major
     * order: [ldx / 32][R][32], element (t, c) at ((c / 32) * R + t) * 32 + c % 32 — the 32-wide k-tile
     * of consecutive rows is contiguous.  dz_k_gemm_pre also expects Wsplit in that order
     * ([Kpad / 32][Npad][32] per plane).  The output, when Ysplit is set (dz_k_gemm_pre, dz_k_gemm_split),
     * is written in the same form (yplane / ldy rows x ldy columns, lo plane yplane elements further; batch
     * item b of dz_k_gemm_split owns rows b * ybs / ldy ..) so that the next layer reads plain bytes.
     * Y (f32, row-major) and Ysplit may both be set.                                            */
    const void* Xsplit;
    long long xplane;
    void* Ysplit;
    long long yplane;
    /* norm-on-load without a finalize launch: instead of nscale / nshift the kernel is handed the
     * producer's tile partials [B][npart_tiles][nld][2] (sum, sumsq over npart_T values per channel)
     * and the InstanceNorm affine, and derives scale / shift itself (same f64 fixed-order
     * arithmetic as dz_k_finalize_norm).  Split-f16 path only (dz_k_gemm_split, dz_k_conv_pool).  */
    const float* npart;
    const float* ngamma;
    const float* nbeta;
    int npart_tiles, npart_T;
    int* oflag;           /* device-visible int set to 1 when an operand of the split-f16 path lies
                             outside +-65504 (it is then clamped); NULL = the context's flag, read
                             with dz_range_check                                                 */
    const int* Tdev;      /* optional device [B] frame count of each batch item (padded RELU_BN layers only):
                             reflect padding of the output frames t < Tdev[b] happens at Tdev[b] instead of
                             Tin (rows of different lengths laid out Tin frames apart; pad < Tdev[b]).  NULL:
                             every item reflects at Tin                                           */
} dz_convgemm_desc;
int dz_k_convgemm(dz_ctx* ctx, const dz_convgemm_desc* desc, void* stream);
/* the exact-f32 kernel of the wide layers alone (k_gemm_f32.hip; dz_k_convgemm routes to it by itself when the
 * layer is in its domain: f32 operands, no prologue / padding / split-K, Npad % 128 == 0, K = taps * Cin unpadded
 * with Cin % 32 == 0; dz_set_option("f32_gemm", 0) keeps every layer on the round-1 kernel).  Same arithmetic per product (one
 * exact f32 FMA), another order of the k sum.  Error if the layer is outside the domain.               */
int dz_k_gemm_f32(dz_ctx* ctx, const dz_convgemm_desc* desc, void* stream);
/* the same layer on the split-f16 matrix-core path (desc->Wsplit must be set)       */
int dz_k_gemm_split(dz_ctx* ctx, const dz_convgemm_desc* desc, void* stream);
/* ... with the activations pre-split as well (desc->Wsplit and desc->Xsplit set; B = 1, K = taps*Cin
 * unpadded, Cin % 32 == 0): operand tiles go global -> LDS by LDS-DMA                            */
int dz_k_gemm_pre(dz_ctx* ctx, const dz_convgemm_desc* desc, void* stream);
/* SincNet stages 1 / 2 (DZ_EPI_POOL3, k = 5, 64 output columns, Cin 80 or 64, norm-on-load, dense
 * rows) on the dedicated kernel: input tile resident in LDS, weights in registers; same
 * descriptor, outputs and partials as the POOL3 call of dz_k_gemm_split                       */
/* Tail of the segmentation network in one launch (csrc/k_mlp_head.hip: linear[0] -> linear[1] ->
 * classifier -> activation -> OSP weights without min-max) and the stand-alone classifier + activation
 * + OSP kernel it is checked against; inputs as the internal layers pass them (kb-major f16 hi/lo planes:
 * xsplit of exactly `rows` rows x 256, w0split [2][8][128][32], w1split [2][4][128][32]).                */
int dz_k_mlp_head(dz_ctx* ctx, const void* xsplit, long long xplane, const void* w0split, const void* w1split,
                  const float* b0, const float* b1, const float* cw, const float* cb, int rows, int frames,
                  int classes, int speakers, int powerset, float gamma, float beta, float* d_seg,
                  float* d_weights, void* stream);
int dz_k_seg_head(dz_ctx* ctx, const float* m1, const float* cw, const float* cb, int batch, int frames,
                  int classes, int speakers, int powerset, float* d_seg, float gamma, float beta,
                  int normalize, float* d_weights, void* stream);
/* (dz_k_conv_pool and dz_k_sinc_conv0_split first re-order their register-resident operand — desc->Wsplit / d_filt_split —
 * into the kernel's fragment order, in a scratch buffer of the CONTEXT: calls that share a context must be stream-ordered.
 * The network handles keep their own re-ordered copies, made once in dz_seg_create / dz_emb_create.)               */
int dz_k_conv_pool(dz_ctx* ctx, const dz_convgemm_desc* desc, void* stream);
int dz_k_convgemm_ntile(int t_out);
/* d_stats (B, 2) = (mean, 1/sqrt(biased var + 1e-5)) of each window: InstanceNorm1d(1).  Inside
 * the forward passes the 8 slice moments stay separate and the consumer merges them; this entry
 * point runs the slice kernel plus the merge and synchronises the stream.                     */
int dz_k_wave_stats(dz_ctx* ctx, const float* d_wave, long long stride, int batch, int samples,
                    float* d_stats, void* stream);
/* Waveform rows of dz_k_wave_stats, dz_k_sinc_conv0* and every handle (d_wave + b * stride): the first row 16-byte
 * aligned, stride a multiple of 4 floats and >= 0 (checked).  That is ALL: no kernel needs readable zeros —
 * or readable memory at all — behind sample S of a row, and no output depends on what lies there.  wave_stats reads
 * float4s and a < 4-sample tail inside [0, S) of each slice; sinc_conv0 tests every index against S; the split kernels
 * (sinc_conv0_split, sinc_conv0_pair) fetch through a buffer descriptor of S * 4 bytes per row (out-of-range dwords
 * come back as zeros) and test the index against S again when they normalise.  So rows may lie roundup4(S) apart (the
 * dense (k, W) batch of dz_ring_gather: row b + 1 starts right behind row b), or be windows into a longer signal whose
 * next samples follow (the rolling window of ring.hip, addressed in place: [q, q + W) of a row of 2 P live samples).
 * A window with a NaN / Inf sample changes no bit of another row's statistics, y0 or partials
 * (tests/test_gpu_front_f64.py: NaN behind every row, a non-finite neighbour).
 * y0 (B, P0, 80) with P0 = ((S-251)/10+1)/3; partials (B, ntile0, 80, 2), ntile0 = ceil(F0/192);
 * d_filt (128, 96): the folded symmetric bank, see dz_sincnet_weights.filt */
int dz_k_sinc_conv0(dz_ctx* ctx, const float* d_wave, long long stride, int batch, int samples,
                    const float* d_stats, float gamma, float beta, const float* d_filt,
                    float* d_y0, float* d_partials, void* stream);
/* the same layer on the f16 matrix cores (split operands); d_filt_split as dz_sincnet_weights.filt_split;
 * partials (B, ntile, 80, 2) with ntile = dz_k_conv0_split_ntile(samples) (96-frame tiles) */
int dz_k_sinc_conv0_split(dz_ctx* ctx, const float* d_wave, long long stride, int batch, int samples,
                          const float* d_stats, float gamma, float beta, const void* d_filt_split,
                          float* d_y0, float* d_partials, void* stream);
int dz_k_conv0_split_ntile(int samples);
int dz_k_finalize_norm(dz_ctx* ctx, const float* d_partials, int batch, int ntile, int channels,
                       int frames, const float* d_gamma, const float* d_beta, float* d_scale,
                       float* d_shift, void* stream);
/* gx (B*T, 1024) = x-projection incl. biases (PyTorch column order dir*512 + gate*128 + unit),
 * whh (2,512,128) -> hout (B,T,256)                                                  */
int dz_k_lstm(dz_ctx* ctx, const float* d_gx, const float* d_whh, float* d_hout, int batch,
              int frames, void* stream);
/* the same recurrence on the f16 matrix cores, 16 chains per workgroup; d_whh_split / variant as
 * dz_seg_weights.whh_split / lstm_variant; unit_major != 0: gx columns are dir*512 + unit*4 + gate
 * (variants 3 / 4: unit-major only; variant 4: gx already times the gates' activation scales)      */
int dz_k_lstm_mfma(dz_ctx* ctx, const float* d_gx, const void* d_whh_split, float* d_hout,
                   int batch, int frames, int unit_major, int variant, void* stream);
/* either recurrence kernel (d_whh_split NULL: the f32 vector kernel on d_whh) writing h as the two
 * f16 planes of hplane / 256 >= B*T rows x 256 columns a dz_k_gemm_pre consumer reads, in kb-major order
 * (see dz_convgemm_desc.Xsplit): hi = f16(h) at d_hsplit, lo = f16((h - hi) * 2^11) hplane elements
 * further; gx in PyTorch column order (variants 3 / 4: unit-major, as dz_k_lstm_mfma)             */
int dz_k_lstm_planes(dz_ctx* ctx, const float* d_gx, const float* d_whh, const void* d_whh_split,
                     int variant, void* d_hsplit, long long hplane, int batch, int frames, void* stream);
/* weight_frames < 0: |weight_frames| weights per row, resampled with mode="nearest" (see dz_emb_weights.pool_nearest) */
int dz_k_stats_pool(dz_ctx* ctx, const float* d_x, int frames, int channels, int ldx,
                    const float* d_weights, int weight_frames, int rows, int rows_per_x,
                    float* d_out, int ldo, void* stream);
/* The last x-vector layer with its statistics pooling, both ways the embedding handle runs them, on the caller's
 * buffers.  desc: the flattened 1 x 1 TDNN layer over Tout = chunks * pitch rows (DZ_EPI_TDNN, taps = 1, B = 1, kb-major
 * planes, as dz_k_gemm_pre); chunk b owns rows b * pitch .., of which the first `frames` are pooled, each with the
 * `speakers` weight rows b * speakers .. of d_weights (weight_frames and NULL as at dz_k_stats_pool).
 * fused != 0: the pooled epilogue of the layer, then the merge of its tile pieces (speakers <= 4, pitch >= 128);
 *   d_part [chunks][np][speakers][Npad][2] and d_s0 [chunks][np][speakers][2] floats, np = dz_k_pool_pieces(pitch);
 *   desc->Y is not written.
 * fused == 0: the layer writes desc->Y, the stand-alone kernel pools it, chunks pitch * ldy floats apart.
 * d_out [chunks * speakers][ldo]: mean in columns 0 .. channels - 1, std in channels .. 2 channels - 1.           */
int dz_k_pool_pieces(int pitch);
int dz_k_tdnn_pool(dz_ctx* ctx, const dz_convgemm_desc* desc, const float* d_weights, int weight_frames, int speakers,
                   int pitch, int frames, int channels, int fused, float* d_part, float* d_s0, float* d_out, int ldo,
                   void* stream);
int dz_k_powerset(dz_ctx* ctx, const float* d_logits, int rows, int classes, int speakers,
                  float* d_out, void* stream);

/* ---- OnlineSpeakerClustering (host, fp64): blocks/clustering.py:10-218 with
 * the SpeakerMap algebra of mapping.py:179-360 and scipy's rectangular LSAP.   */
int dz_clu_create(double tau_active, double rho_update, double delta_new,
                  int max_speakers, dz_clu** out);
int dz_clu_reset(dz_clu* clu);
/* one chunk: seg (F,K) f32, emb (K,D) f32 (NaN allowed) -> scores (F,G) f64
 * (zeros for unassigned global speakers, mapping.py:341-360).
 * assign_out (K) receives the global speaker of each local speaker or -1.       */
int dz_clu_step(dz_clu* clu, const float* seg, int frames, int k_local,
                const float* emb, int dim, double* scores_out, int* assign_out);
/* the same for n independent streams (one clu handle each), run on host threads;
 * seg (n,F,K), emb (n,K,D), scores (n,F,G), assign (n,K).                        */
int dz_clu_step_batch(dz_clu** clus, int n, const float* seg, int frames, int k_local,
                      const float* emb, int dim, double* scores_out, int* assign_out,
                      int num_threads);
/* state: centers (G,D) f64 copied to `out` (returns 1 if not initialised yet),
 * active mask (G) ints.                                                          */
int dz_clu_get_centers(dz_clu* clu, double* out, int dim);
int dz_clu_get_active(dz_clu* clu, int* out_mask);
/* embedding dimension of the centroid matrix, 0 before the first chunk (centers is None) */
int dz_clu_dim(dz_clu* clu);
int dz_clu_set_state(dz_clu* clu, const double* centers, const int* active_mask, int dim);
int dz_clu_destroy(dz_clu* clu);

/* ---- per-kernel timing (HIP events on the launch stream) for bench.py's roofline leg ----
 * dz_prof_enable(1) starts bracketing every kernel the forward passes launch; dz_prof_collect()
 * synchronises the device and accumulates; dz_prof_get(tag) reads name / total ms / launches. */
int dz_prof_enable(int on);
int dz_prof_pause(int paused);   /* suspend / resume bracketing, accumulators untouched */
int dz_prof_collect(void);
/* chunks: total number of 5 s chunks the tag's bracketed launches processed (a launch of a
 * 32-chunk sub-batch counts 32): the unit the per-launch algorithmic work is priced in */
int dz_prof_get(int tag, const char** name, double* total_ms, long long* launches,
                long long* chunks);

/* ---- device-resident rolling window of N streams ------------------------------------------
 * Replaces rearrange_audio_stream (/root/reference/src/diart/operators.py:44-100) plus the
 * per-chunk upload of the full window (blocks/segmentation.py:47, blocks/embedding.py:52) for the
 * N-stream driver: every step only the `hop` new samples of each stream are pushed (32 KB
 * instead of 320 KB per stream at 5 s / 500 ms); dz_ring_window returns the (pointer, row
 * stride) pair dz_seg_forward / dz_emb_frames read in place.  window % hop == 0.  A ring whose
 * hop is not a multiple of 4 samples (44.1 kHz: 22 050 per 500 ms) serves the per-row entry points,
 * dz_ring_push and dz_ring_read only, at 4-byte granularity: dz_ring_window refuses it (its
 * windows do not start on 16-byte boundaries, which the in-place readers need).
 * slack_blocks extra blocks of history are kept so that pushing block t+1 never overwrites a
 * sample of windows t-slack_blocks+1 .. t (forward passes of those may still be in flight).     */
typedef struct dz_ring dz_ring;
int dz_ring_create(dz_ctx* ctx, int n_streams, int window, int hop, int slack_blocks, dz_ring** out);
int dz_ring_reset(dz_ring* r);
int dz_ring_destroy(dz_ring* r);
/* The three push entry points check their arguments and share ONE path: the block is read where it
 * lies (device memory, or pinned host memory mapped into the GPU) or lands through one asynchronous
 * copy in one of the ring's two landing blocks, used alternately (allocated by dz_ring_create for a
 * mono float32 block of every stream, so the default workload allocates nothing later; they grow on
 * demand for wider client formats), and ONE kernel writes it to the ring.
 * dz_ring_push, the lock-step push: block (n_streams, hop) with block_stride floats between rows,
 * every stream at the common write position, one launch; afterwards every row's own position (below)
 * is that position.  Host memory (on_device = 0;
 * pinned memory makes the copy asynchronous), device memory (on_device = 1), or pinned host memory
 * to be read in place by the GPU when the runtime can map it (on_device = 2; falls back to 0).   */
int dz_ring_push(dz_ring* r, const float* block, long long block_stride, int on_device, void* stream);
/* *filled = min(window, samples pushed): the window is complete once *filled == window.     */
int dz_ring_window(const dz_ring* r, const float** d_wave, long long* stride, int* filled);
/* contiguous (n_streams, window) copy of the current window, device to device.               */
int dz_ring_read(const dz_ring* r, float* d_out, void* stream);
/* Streams that advance at their own pace (one rearrange_audio_stream per stream,
 * /root/reference/src/diart/inference.py:101-147 + console/serve.py:105-127, served as ONE batch):
 * every row has its own write position.  dz_ring_push_rows: row j of block (k, hop) is the next
 * block of stream rows[j] (distinct rows; on_device as for dz_ring_push).  dz_ring_gather: the
 * current windows of the listed streams as a dense (k, window) device batch for dz_seg_forward /
 * dz_emb_frames — each must be complete (dz_ring_filled_row); d_out rows 16-byte aligned (4-byte
 * aligned for a ring whose hop is not a multiple of 4).  dz_ring_reset_row: the stream left. */
int dz_ring_push_rows(dz_ring* r, const float* block, long long block_stride, int on_device,
                      const int* rows, int k, void* stream);
/* Raw client audio: row j of `block` holds hop interleaved frames of `channels` (1 .. 8) values of
 * `format`, rows block_stride_bytes apart.  One kernel converts, averages the channels and writes
 * the block to the ring.  The float32 sample it writes, operation for operation (every format is
 * exact in float32 but for the one rounding named for DZ_PCM_S32):
 *   DZ_PCM_S16 (int16, little-endian): (float)v * (1.0f / 32768.0f);
 *   DZ_PCM_U8 (uint8): ((float)v - 128.0f) * (1.0f / 128.0f);
 *   DZ_PCM_S32 (int32, little-endian): (float)v * (1.0f / 2147483648.0f); the int-to-float conversion
 *     rounds to nearest even (0x7fffffc0 gives 1.0f), the scaling is exact;
 *   DZ_PCM_ULAW (uint8, G.711 mu-law): (float)L * (1.0f / 32768.0f) with
 *     u = ~b & 0xFF; t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7); L = (u & 0x80) ? 0x84 - t : t - 0x84;
 *   DZ_PCM_ALAW (uint8, G.711 A-law): (float)L * (1.0f / 32768.0f) with
 *     a = b ^ 0x55; m = (a & 0x0F) << 4; s = (a >> 4) & 7; t = (s == 0) ? m + 8 : (m + 0x108) << (s - 1);
 *     L = (a & 0x80) ? t : -t;
 *   channels > 1: ((c0 + c1) + c2 ...) / (float)channels, one IEEE division;
 *   DZ_PCM_F32 with one channel: the input bits (what dz_ring_push_rows and dz_ring_push write:
 *     the same kernel).
 * Non-finite float input passes through (a NaN in one channel makes that frame NaN).  Another
 * format value is refused.
 * Rows and ring positions on 16-byte boundaries are moved 16 bytes per lane, others value by value;
 * the samples do not depend on it.
 * dz_pcm_decode: the same per-frame function over one contiguous device buffer of n_frames
 * interleaved frames (d_src aligned to one value), mono float32 to d_dst, without a ring.        */
enum { DZ_PCM_F32 = 0, DZ_PCM_S16 = 1, DZ_PCM_U8 = 2, DZ_PCM_S32 = 3, DZ_PCM_ULAW = 4, DZ_PCM_ALAW = 5 };
int dz_ring_push_rows_pcm(dz_ring* r, const void* block, long long block_stride_bytes, int format, int channels,
                          int on_device, const int* rows, int k, void* stream);
int dz_pcm_decode(dz_ctx* ctx, const void* d_src, long long n_frames, int format, int channels, float* d_dst,
                  void* stream);
int dz_ring_filled_row(const dz_ring* r, int row, int* filled);
int dz_ring_gather(const dz_ring* r, const int* rows, int k, float* d_out, long long out_stride, void* stream);
int dz_ring_reset_row(dz_ring* r, int row);

/* ---- output tail of one stream: DelayedAggregation + Binarize, host fp64 -------------------
 * Replaces, for the N-stream driver, the per-chunk Python tail of SpeakerDiarization.__call__
 * (/root/reference/src/diart/blocks/diarization.py:203-232): DelayedAggregation
 * (blocks/aggregation.py:120-218; strategies :60-118; first-chunk prepend :188-211) followed by
 * Binarize (blocks/utils.py:11-59).  State: the last round(latency/step) permuted score
 * buffers of the stream.  dz_tail_step consumes the (frames, speakers) fp64 scores of the newest
 * chunk (what dz_clu_step wrote), whose frame grid starts at chunk_start seconds with
 * `resolution` seconds per frame (diarization.py:190,195-199), and returns
 *   agg_out  (rows, speakers) aggregated scores of the region [t0, t0 + rows*res), rows <=
 *            dz_tail_max_rows() = frames + 2 (the first chunk of a stream outputs everything up
 *            to the end of its region);
 *   turns_out (nturns, 3) = (start, end, speaker index) of `score > threshold` runs, ordered by
 *            speaker then time; turns_out may be NULL.  More than max_turns turns -> error 5.  */
enum { DZ_AGG_HAMMING = 0, DZ_AGG_MEAN = 1, DZ_AGG_FIRST = 2 };
enum { DZ_CROP_STRICT = 0, DZ_CROP_LOOSE = 1, DZ_CROP_CENTER = 2 };
typedef struct dz_tail dz_tail;
int dz_tail_create(int frames, int speakers, double step, double latency, double threshold,
                   int strategy, int cropping_mode, const double* hamming /* [frames] */,
                   dz_tail** out);
int dz_tail_reset(dz_tail* t);                 /* forgets the buffers and the hysteresis states; keeps the offset */
/* Hysteresis (pyannote's onset / offset): from the next step on a row of a speaker column is on when its score is
 * > threshold while the column is off and > offset while it is on.  The state is kept per speaker column, starts off,
 * crosses from a step into the next one and is cleared by dz_tail_reset; a NaN row is off and leaves the state off.
 * The turns are formed from `on` as before (the row after a step's last closes an open turn).  Valid for any speaker
 * count; any finite offset is accepted, offset == threshold being `score > threshold` row for row, and a non-finite one
 * is status 2.  A tail on which this was never called runs the stateless walk.  A step that returns 5 (more turns
 * than max_turns) has still moved every column's state over all of its rows; like any failed step it leaves its buffer
 * in the handle, so reset the handle before the stream goes on.                                                     */
int dz_tail_set_offset(dz_tail* t, double offset);
int dz_tail_destroy(dz_tail* t);
int dz_tail_max_rows(const dz_tail* t);
int dz_tail_speakers(const dz_tail* t);      /* the `speakers` it was created with */
int dz_tail_step(dz_tail* t, const double* scores, double chunk_start, double resolution,
                 double* agg_out, int* rows_out, double* t0_out, double* res_out,
                 double* turns_out, int max_turns, int* nturns_out);
/* n streams on host threads: scores (n, frames, speakers); chunk_start, resolution (n);
 * agg_out (n, frames + 2, speakers); rows_out, t0_out, res_out, nturns_out (n);
 * turns_out (n, max_turns, 3) or NULL.                                                        */
int dz_tail_step_batch(dz_tail** tails, int n, const double* scores, const double* chunk_start,
                       const double* resolution, double* agg_out, int* rows_out, double* t0_out,
                       double* res_out, double* turns_out, int max_turns, int* nturns_out,
                       int num_threads);

/* ---- file-parallel evaluation: the host half of a GPU step over several files --------------
 * Replaces the per-chunk Python loop of SpeakerDiarization.__call__
 * (/root/reference/src/diart/blocks/diarization.py:193-232) as driven by Benchmark, one file at a
 * time in batches of consecutive windows (/root/reference/src/diart/inference.py:392-432).  The rows
 * of the GPU batch are file-major: file i contributes its next count[i] CONSECUTIVE windows, rows
 * row0[i] .. row0[i] + count[i] - 1 of seg (rows, frames, k_local) / emb (rows, k_local, dim) /
 * chunk_start (rows).  Per file, in window order: dz_clu_step -> dz_tail_step on that file's own
 * handles; files run in parallel on host threads.  turns_out (rows, max_turns, 3), nturns_out (rows):
 * the speech turns each window finalises; assign_out (rows, k_local) or NULL.                    */
int dz_file_step_batch(dz_clu** clus, dz_tail** tails, int n_files, const int* row0, const int* count,
                       const float* seg, int frames, int k_local, const float* emb, int dim,
                       int max_speakers, const double* chunk_start, double resolution,
                       double* turns_out, int max_turns, int* nturns_out, int* assign_out,
                       int num_threads);

/* The VoiceActivityDetection sibling (blocks/vad.py:136-191 of the reference, driven the same way): no clustering.
 * track (rows, frames) float32 = the speech track of every window (max over speakers of the segmentation, what
 * dz_seg_forward_vad writes); tails: per file, built for ONE speaker and `frames` frames.  Per file, in window order:
 * dz_tail_step on that file's own handle (the track widened to fp64); files run in parallel on host threads.  A failing
 * file is reported with its index and the worker's own message; bad arguments return 2 and touch nothing.           */
int dz_file_vad_step_batch(dz_tail** tails, int n_files, const int* row0, const int* count, const float* track,
                           int frames, const double* chunk_start, double resolution, double* turns_out,
                           int max_turns, int* nturns_out, int num_threads);

/* ---- the rows of a file-batch step in one launch (csrc/k_gather.hip) ------------------------
 * rows row0 .. row0+count-1 of d_out receive the windows src + j*hop .. + num_samples of run i (consecutive windows of
 * one file's resident audio).  The runs are passed to the kernel by value, DZ_GATHER_MAX_RUNS per launch (more runs:
 * more launches on the same stream).  No synchronisation, no allocation, nothing read from device memory by the host.
 * A run with count == 0 is skipped.  Errors (code 2, nothing launched): row0 < 0, row0 + count > out_rows,
 * out_stride < num_samples, hop < 1, n_runs < 1, a NULL src with count > 0.  A pure copy: 16-byte loads / stores where
 * a window and its row are both 16-byte aligned, one float at a time otherwise; nothing outside the rows and the
 * first num_samples columns asked for is written.                                                                  */
#define DZ_GATHER_MAX_RUNS 64
typedef struct { const float* src; int row0; int count; } dz_window_run;   /* host array */
int dz_gather_windows(dz_ctx* ctx, const dz_window_run* runs, int n_runs, int num_samples, int hop,
                      float* d_out, long long out_stride, int out_rows, void* stream);

/* ---- hyper-parameter tuning: replay cached model outputs --------------------
 * tau_active, rho_update and delta_new act only after the networks, so a trial is a replay of the
 * cached segmentation (chunks, frames, k_local) and embeddings (chunks, k_local, dim) of every file:
 * clustering -> Hamming aggregation -> binarisation -> error rate.  The chunks of the N files are
 * concatenated (file n: chunk_off[n] .. chunk_off[n + 1]); everything in dz_tune_desc is the same for
 * every trial and is computed once, on the host, when the cache is collected:
 *   pre_max / pre_mean / pre_flags (chunks, k_local)  what identify derives from seg: the float32 max, the
 *       float32 sequential mean, bit 0 = a NaN score, bit 1 = a NaN in the embedding row
 *   plan (chunks, 4 + nwin)  dz_tune_plan: per step {aggregated rows, prepended rows of a first chunk, their
 *       first cropped row, buffers, first cropped row of each buffer}; buffer b of step c is chunk c - buffers + 1 + b
 *   row_off (chunks + 1), row_chunk (total_rows)  the packed output rows: a prefix sum of the rows per step
 *       and each row's step
 * max_speakers <= 32 (a frame's hypothesis is one 32-bit mask) and k_local <= 8.                         */
typedef struct dz_tune_desc {
    const float* seg;
    const float* emb;
    const float* pre_max;
    const float* pre_mean;
    const unsigned char* pre_flags;
    const int* chunk_off;
    const int* plan;
    const int* row_off;
    const int* row_chunk;
    const double* hamming; /* [frames] */
    int N, F, K, D, G, nwin, total_chunks, total_rows;
} dz_tune_desc;
int dz_tune_abi_size(void);
/* The tail's plan of one file (Hamming aggregation, "loose" cropping) from the text dz_tail_step runs (csrc/tail_core.h):
 * starts, resolution (chunks) as dz_tail_step gets them.  plan (chunks, 4 + nwin) with
 * nwin = round(latency / step); t0_out, res_out (chunks): the output grid of every step.  4 = the output
 * region does not map onto the frame grid of every buffer.                                              */
int dz_tune_plan(int chunks, int frames, double step, double latency, const double* starts,
                 const double* resolution, int* plan, double* t0_out, double* res_out);
/* T trials (hparams (T, 3): tau, rho, delta) x N files on the GPU: every pointer of `d` and every array here
 * is device memory.  assign (T, chunks, k_local) int8: the global speaker of every local one or -1;
 * status (T, N): -1, or the first chunk of the file at which dz_clu_step would return non-zero (the chain
 * stops there); bits (T, total_rows): bit g = the aggregated score of global speaker g is > tau.
 * One wavefront walks one (trial, file) chain; its centroids live in work (work_blocks, dim * max_speakers)
 * doubles, one slice per resident workgroup.  phases: 3 = both kernels; 1 = the clustering alone, 2 = the masks
 * alone, from the assignments d_assign holds (measurements).  Enqueued on `stream`, no synchronisation.  */
int dz_tune_replay(dz_ctx* ctx, const dz_tune_desc* d, const double* d_hparams, int trials,
                   signed char* d_assign, int* d_status, unsigned* d_bits, double* d_work, int work_blocks,
                   int phases, void* stream);
/* The same three arrays from host memory.  use_core = 0: with dz_clu_step and dz_tail_step, one handle pair
 * per (trial, file), pairs on host threads (starts, resolution (chunks), step, latency as dz_tail_step gets
 * them).  use_core = 1: the text the kernels are compiled from, run on the host (tests hold it against the
 * former without a GPU).                                                                                */
int dz_tune_replay_host(const dz_tune_desc* d, const double* hparams, int trials, double step, double latency,
                        const double* starts, const double* resolution, signed char* assign, int* status,
                        unsigned* bits, int use_core, int num_threads);
/* The scoring geometry of a cache, the other half of a trial: where the files' steps, rows and frame middles lie and
 * the scoring cells they are scored on.  The same for every trial and computed once; every pointer is host memory for
 * the host entries and device memory for the device entries, as with dz_tune_desc.
 *   file_chunk_off, file_row_off, file_cell_off (N + 1): the steps, packed rows and cells of file n
 *   row_off (chunks + 1), step_rows (chunks): the packed rows of every step, as a prefix sum and as counts
 *   mids (total_rows + chunks): per step its rows + 1 frame middles, timestamp shift added; mid_cell: the cell
 *       that starts at that time
 *   cell_dur, cell_ref (cells): duration and bit mask of the reference speakers of every cell; cell_step (cells): the
 *       step (chunk of the cache) that owns it (step c owns the cells from its first frame middle to the next step's)
 *   dur_prefix, ref_prefix (cells + N): per file its cells + 1 prefix sums of cell_dur and of cell_dur where the
 *       reference is active (file n starts at file_cell_off[n] + n)
 *   max_cells: the cells of the largest file; collar: same-speaker turns closer than it are merged
 * An entry reads the members its comment lists ("cells:") and no other: those may be NULL or 0.  A NULL among the
 * listed pointers is refused with 2 and a message that names the entry and the member.                             */
typedef struct dz_tune_cells {
    const int* file_chunk_off;
    const int* file_row_off;
    const int* row_off;
    const int* step_rows;
    const double* mids;
    const int* mid_cell;
    const int* file_cell_off;
    const double* cell_dur;
    const unsigned long long* cell_ref;
    const int* cell_step;
    const double* dur_prefix;
    const double* ref_prefix;
    int n_files, total_rows, total_chunks, max_cells, max_speakers;
    double collar;
} dz_tune_cells;
int dz_tune_cells_abi_size(void);
/* Diarization error rate components (collar 0, overlap included) of every (trial, file) pair from the packed
 * frame masks bits (T, total_rows), without building annotations: speech turns as Binarize forms them, same-speaker
 * turns closer than `collar` merged as Annotation.support does, then total / correct / false alarm / missed detection /
 * confusion over the file's scoring cells under the optimal one-to-one mapping.  out (T, N, 5).
 * cells: file_row_off, file_chunk_off, step_rows, mids, mid_cell, file_cell_off, cell_dur, cell_ref; n_files,
 * total_rows, max_speakers, collar.                                                                      */
int dz_tune_score(const dz_tune_cells* cells, int trials, const unsigned* bits, double* out, int num_threads);
/* dz_tune_score on the device: d_bits (T, total_rows) as dz_tune_replay wrote them stay there, and d_out
 * (T, N, 5) is all that a call leaves.  One workgroup per (trial, file) pair, score_blocks of them resident,
 * each on its own slice of d_scratch (score_blocks, max_cells + 1) uint32; the steps of a file sorted by time.
 * What differs from dz_tune_score is the order in
 * which the durations are summed (per lane, the lanes in order: the same doubles on every call).  d_err: one
 * int, 0 after the call, or dz_tune_score's return code (4 = a turn off the file's cells, 3 = the assignment
 * problem failed, 2 = a file with more than max_cells cells) of some pair; d_out is then not to be used.
 * Enqueued on `stream`, no synchronisation.
 * cells (the "kernel set"): file_chunk_off, row_off, mids, mid_cell, file_cell_off, cell_dur, cell_ref; n_files,
 * total_rows, max_cells, max_speakers, collar.                                                            */
int dz_tune_score_gpu(dz_ctx* ctx, const dz_tune_cells* d_cells, int trials, const unsigned* d_bits, double* d_out,
                      unsigned* d_scratch, int score_blocks, int* d_err, void* stream);
/* The same from host memory, compiled from the text of the kernel: the `lanes` (at most 256) lanes of a
 * workgroup played in order, "workgroup" b of score_blocks taking pairs b, b + score_blocks, ... on one
 * scratch slice, workgroups on num_threads host threads.  Returns dz_tune_score's codes.  cells: the kernel set. */
int dz_tune_score_core(const dz_tune_cells* cells, int trials, const unsigned* bits, int lanes, int score_blocks,
                       double* out, int num_threads);
/* Tuning VoiceActivityDetection (tau_active alone): one track per chunk, so dz_tune_desc has k_local = 1,
 * seg (chunks, frames) = the max over the local speakers, and emb / pre_* unused (may be NULL).  The
 * aggregated speech score of a packed output row does not depend on tau: dz_tune_vad_rows writes
 * d_agg (total_rows) doubles once per cache (the value dz_tune_replay compares with tau when the one
 * local speaker of every buffer is mapped).  Device memory throughout, enqueued on `stream`.
 * The dz_tune_vad_* calls serve both track pipelines: for OverlappedSpeechDetection seg is the
 * second largest over the local speakers and ref_prefix sums the cells where two different reference
 * speakers are active; nothing in the arithmetic knows which of the two it is given.                   */
int dz_tune_vad_rows(dz_ctx* ctx, const dz_tune_desc* d, double* d_agg, void* stream);
/* T trials x N files from d_agg under the row rule that `cols`, the columns of d_taus (T, cols), selects (any other
 * value returns 2); one pair routine (tc_track_pair in csrc/tune_core.h) under three rules:
 *   cols = 1  (tau_active): row r is speech when agg > tau.
 *   cols = 2  (tau_active, tau_offset), hysteresis: a row is on when agg > tau_active while the track
 *             is off and > tau_offset while it is on (dz_tail_set_offset's rule), the state off at every file's first
 *             step and carried across its steps; the lanes compose the state maps of their steps before they walk
 *             them, so every row's `on` is the sequential rule's.  With tau_offset == tau_active: the doubles of cols = 1.
 *   cols = 4  (tau_active, tau_offset, min_duration_on, min_duration_off), minimum durations where a whole file is
 *             known: the rows and the masks are those of cols = 2 — the masks are taken BEFORE the
 *             durations act; a filled gap is no row.  The file's turns are merged with the collar max(collar,
 *             min_duration_off) (Annotation.support), then a merged span counts unless end - start < min_duration_on,
 *             strictly, both from `mids`: every lane leaves a summary of its steps, one lane composes the summaries in
 *             lane order.  With zero durations: the doubles of cols = 2.
 * The turns, their merging and the scoring cells are dz_tune_score's for one hypothesis label against a reference
 * collapsed to one label (detection error rate: the confusion is 0).  One workgroup per (trial, file); d_out (T, N, 5)
 * is all that a trial leaves.  d_bits (T, total_rows), if not NULL: the rows as 0 / 1 masks (cols = 1: from a kernel
 * of one thread per row, which bounds trials x total_rows as well as trials x files); d_out may be NULL then.
 * taus_host: the trials in host memory, required for cols = 4 and ignored otherwise: the device form cannot read
 * d_taus, and a duration that is negative or not finite is refused before the context or any device pointer is looked
 * at (the callers check tau_offset).  Also refused with 2: a NULL pointer, trials < 1.
 * cells (the "track set"): file_chunk_off, row_off, mids, mid_cell, file_cell_off, dur_prefix, ref_prefix; n_files,
 * total_rows, collar.                                                                                             */
int dz_tune_vad_score(dz_ctx* ctx, const dz_tune_cells* d_cells, int cols, int trials, const double* d_agg,
                      const double* taus_host, const double* d_taus, double* d_out, unsigned* d_bits, void* stream);
/* The same from host memory, compiled from the text of the kernels: taus (T, cols); agg (total_rows), written; bits
 * (T, total_rows) if not NULL; out (T, N, 5) if not NULL, the workgroup's `lanes` lanes played in order.  lanes is at
 * most 256, the workgroup of the kernel and the bound of every sibling *_core entry point (the Python side only ever
 * passes 256); more returns 2, and so does a non-finite tau_offset.  The steps and rows are d's (chunk_off, row_off).
 * cells: mids, mid_cell, file_cell_off, dur_prefix, ref_prefix; collar — for out, and under cols = 2 and 4 for the
 * masks too (with lanes 1 .. 256); cols = 1 with out NULL reads nothing of cells, which may be NULL then.          */
int dz_tune_vad_host(const dz_tune_desc* d, const dz_tune_cells* cells, int cols, const double* taus, int trials,
                     double* agg, unsigned* bits, int lanes, double* out, int num_threads);
/* The components of cols = 4 trials from an independent sequential text, behind masks made elsewhere: one host thread
 * per (trial, file) walks the file's turns from bits (T, total_rows; bit 0) in order, merges, drops and sums the
 * cells one by one.  Of taus (T, 4) the two durations are read.  Returns 4 when a turn does not start and end on the
 * file's cells.  cells: file_chunk_off, row_off, mids, mid_cell, file_cell_off, cell_dur, cell_ref; n_files,
 * total_rows, collar.                                                                                              */
int dz_tune_track_score_dur(const dz_tune_cells* cells, int trials, const unsigned* bits, const double* taus,
                            double* out, int num_threads);
/* The masks of the same trials from an independent text: one dz_tail handle per (trial, file) with dz_tail_set_offset,
 * fed the file's track step by step (starts, resolution (chunks), step, latency as dz_tail_step gets them), the
 * masks read back from the turns it returns.  bits (T, total_rows).                                                  */
int dz_tune_vad_replay_tails(const dz_tune_desc* d, const double* taus, int trials, double step, double latency,
                             const double* starts, const double* resolution, unsigned* bits, int num_threads);
/* Tuning delta_id, the identification distance of a speaker gallery.  A trial's names are the
 * rule of the live engines replayed over the assignments dz_tune_replay wrote: per global speaker the closest
 * match so far, a step's local speaker k with assign = g, match_index = e >= 0 and
 * (double)match_distance <= delta_id replacing it when match_distance < best (float32, strictly); g carries the
 * name of its voiceprint unless another speaker holds the same one with a lower best distance (ties: the lower
 * g).  match_index / match_distance (chunks, k_local): the stored match of every embedding row against the
 * gallery (-1 / NaN: none), the same for every trial; vp_ref (N, voiceprints) int8: the reference bit of file n
 * whose label is voiceprint v's name, or -1.  ident int8: the reference
 * bit of the name speaker g carries in that step, or -1 (no name, or a name no reference label of the file has);
 * hold int32, if not NULL: the voiceprint itself, or -1.  A chain takes nothing from its status chunk on.
 * One clustering trial is named (and scored, below) at `points` (plane, threshold) points, 1 .. 256, plane-major
 * (the sweep): point j reads plane j / (points / planes) of match_index / match_distance (planes,
 * chunks, k_local), 1 .. 8 planes that divide the points, and threshold delta_id[t * points + j] of delta_id
 * (T, points).  ident (T, points, chunks, max_speakers), hold likewise.  One point is points = planes = 1.
 * dz_tune_name: device memory, one wavefront per (trial, point, file) chain, name_blocks workgroups resident; enqueued
 * on `stream`, no synchronisation.  Refused with 2 before anything runs: a NULL pointer (d_hold excepted), trials < 1,
 * max_speakers > 32, voiceprints < 1, points outside 1 .. 256, planes outside 1 .. 8 or not dividing the points. */
int dz_tune_name(dz_ctx* ctx, int trials, int points, int planes, int n_files, int total_chunks, int k_local,
                 int max_speakers, int voiceprints, const int* d_file_chunk_off, const signed char* d_assign,
                 const int* d_status, const int* d_match_index, const float* d_match_distance,
                 const signed char* d_vp_ref, const double* d_delta_id, signed char* d_ident, int* d_hold,
                 int name_blocks, void* stream);
/* The same from host memory, compiled from the text of the kernel, chains on num_threads host threads.     */
int dz_tune_name_host(int trials, int points, int planes, int n_files, int total_chunks, int k_local, int max_speakers,
                      int voiceprints, const int* file_chunk_off, const signed char* assign, const int* status,
                      const int* match_index, const float* match_distance, const signed char* vp_ref,
                      const double* delta_id, signed char* ident, int* hold, int num_threads);
/* Identification error rate components of every (trial, file) pair at one point: dz_tune_score's turns, merging and
 * cells, but the labels are compared as they are (no mapping).  A set bit g of a cell's hypothesis mask stands for
 * ident[cell_step][g], ident (T, chunks, max_speakers).  Per cell with Nref reference labels, Nhyp hypothesis labels
 * and Nboth in both: total += dur Nref, correct += dur Nboth, false alarm += dur max(0, Nhyp - Nref),
 * missed detection += dur max(0, Nref - Nhyp), confusion += dur (min(Nref, Nhyp) - Nboth).  out (T, N, 5).
 * 4 = a turn or a step off the file's cells.  The independent sequential text: the yardstick of the two below.
 * cells: dz_tune_score's and cell_step, total_chunks.                                                       */
int dz_tune_ident_score(const dz_tune_cells* cells, int trials, const unsigned* bits, const signed char* ident,
                        double* out, int num_threads);
/* The same on the device at every point of dz_tune_name's ident (T, points, chunks, max_speakers), as dz_tune_score_gpu
 * is dz_tune_score's: one workgroup per (trial, file) pair, score_blocks of them resident on their slices of d_scratch
 * (score_blocks, max_cells + 1) uint32; the cells' masks once and then every point's components in turn, the sums per
 * lane, the lanes in order (the same doubles on every call, and each point's those of a call with that point alone).
 * d_out (T, points, N, 5).  d_err: one int, 0 after the call, or 4 / 2 as dz_tune_score_gpu.  Enqueued on `stream`, no
 * synchronisation.  Refused with 2 before anything runs: a NULL pointer, trials < 1, points outside 1 .. 256.
 * cells: the kernel set and cell_step, total_chunks.                                                        */
int dz_tune_ident_score_gpu(dz_ctx* ctx, const dz_tune_cells* d_cells, int trials, int points, const unsigned* d_bits,
                            const signed char* d_ident, double* d_out, unsigned* d_scratch, int score_blocks,
                            int* d_err, void* stream);
/* The same from host memory, compiled from the text of the kernel (the lanes of a workgroup played in order,
 * as dz_tune_score_core).                                                                                  */
int dz_tune_ident_score_core(const dz_tune_cells* cells, int trials, int points, const unsigned* bits,
                             const signed char* ident, int lanes, int score_blocks, double* out, int num_threads);

/* Whole-file diarization: centroid-linkage agglomerative clustering of unit rows in float64, and
 * what follows the dendrogram.  A call clusters n_files files: file f owns rows rows_off[f] .. rows_off[f + 1] - 1 of
 * x (rows, D) float64 (rows_off: HOST memory, n_files + 1 ascending ints from 0) and max(n - 1, 0) rows of Z, the
 * files' rows one after another: Z[t] = (smaller id, larger id, height, size), scipy's linkage(x, "centroid")
 * layout.  status (n_files): -1, or the merge at which an index read from memory failed its range check (that
 * file's Z is unfinished).  Rows are expected finite and of unit length (the caller checks).
 * dz_agglo_linkage: x, Z, status and the workspace in device memory, work_bytes >= dz_agglo_work_bytes(n_files,
 * rows_off) (8 n^2 bytes per file and a few arrays per row; -1: bad arguments); enqueued on `stream`, which it
 * waits for once before the first kernel; nothing is read back.  dz_agglo_linkage_host: the same from host memory,
 * compiled from the text of the kernels (csrc/agglo_core.h), files on num_threads host threads.
 * Refused with 2 before anything runs: a NULL pointer, n_files outside 1 .. 1024, D outside 1 .. 1024, a rows_off
 * that does not ascend from 0, a workspace that is too small.                                                  */
long long dz_agglo_work_bytes(int n_files, const int* rows_off);
int dz_agglo_linkage(dz_ctx* ctx, int n_files, const int* rows_off, const double* d_x, int D, double* d_Z,
                     int* d_status, void* d_work, long long work_bytes, void* stream);
int dz_agglo_linkage_host(int n_files, const int* rows_off, const double* x, int D, double* Z, int* status,
                          int num_threads);
/* scipy's fcluster(Z, threshold, "distance") over n leaves (a flat cluster is a maximal subtree whose merge heights
 * are all <= threshold), then the kept clusters: those with at least min_cluster_size leaves, at most max_speakers
 * of them by size (ties: the one whose first leaf comes first), the largest one when none qualifies; numbered
 * 0 .. G - 1 by their first leaf.  labels (n): the kept cluster of each leaf, or -1; *n_kept = G.  n = 0: G = 0;
 * n = 1: one cluster.  2: a NULL pointer, a threshold that is not finite, min_cluster_size or max_speakers below 1,
 * a Z that is no dendrogram over n leaves.  1 (this entry, dz_offline_assign, dz_offline_reconstruct,
 * dz_agglo_linkage_host): no memory.                                                                            */
int dz_agglo_cut(const double* Z, int n, double threshold, int min_cluster_size, int max_speakers, int* labels,
                 int* n_kept);
/* x (rows, D) unit rows; train (n_train): the rows that were clustered, labels (n_train): dz_agglo_cut's.  Cluster
 * g's centroid (centroids (n_kept, D), written) is the mean of its own train rows; assign (rows): the cluster at
 * the lowest cosine distance 1 - x.c / |c| (ties: the lowest).                                                  */
int dz_offline_assign(const double* x, int rows, int D, const int* train, const int* labels, int n_train,
                      int n_kept, int* assign, double* centroids);
/* The timeline of n_files files from their clustered chunks, files on num_threads host threads.  Per file f:
 * seg[f] (chunks[f], F, K) scores, assign[f] (chunks[f], K) the cluster of each local speaker or -1, offset[f]
 * (chunks[f]) the output frame of each chunk's first frame, n_kept[f] clusters, frames[f] output frames ->
 * active[f] (frames[f], n_kept[f]) bytes.  A chunk with a non-finite score takes no part.  A[t][g] = sum over the
 * chunks covering t of the max score of the local speakers assigned to g (0: none); count[t] = min(rint(mean over
 * those chunks of the local speakers above tau_active), G), half to even; g is on at t when it is among the
 * count[t] largest of A[t] (stable: the lower g first) and A[t][g] > 0.  2: a NULL pointer, a chunk that leaves
 * the output frames, an assignment outside the clusters.                                                        */
int dz_offline_reconstruct(int n_files, const float* const* seg, const int* const* assign, const int* const* offset,
                           const int* chunks, int F, int K, const int* n_kept, double tau_active, const int* frames,
                           unsigned char* const* active, int num_threads);

/* sizeof() of the five structs that cross this boundary, in declaration order
 * (dz_sincnet_weights, dz_seg_weights, dz_emb_weights, dz_ecapa_weights, dz_convgemm_desc): a
 * binding checks its own mirror of the layouts against the library it loaded.            */
int dz_abi_struct_sizes(int out[5]);

/* exposed for tests: scipy.optimize.linear_sum_assignment (minimise), rows<=cols
 * or transposed internally; col4row (nr) gets the column of each row.            */
int dz_lsap(const double* cost, int nr, int nc, int* col4row);

#ifdef __cplusplus
}
#endif
#endif /* DIART_AMD_H */
