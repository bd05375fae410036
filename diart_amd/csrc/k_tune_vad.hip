// Tuning VoiceActivityDetection on cached model outputs: there is no clustering and the Hamming
// aggregation does not depend on tau_active, so the aggregated speech score of every packed output row is computed
// once per cache and a trial is one comparison per row plus the detection error rate's bookkeeping.
// These kernels serve both track pipelines: OverlappedSpeechDetection (OsdTuneCache) feeds them the overlap track and
// the prefix sums of the reference's overlap regions.
//
//   tune_vad_rows_kernel          one thread per packed output row: agg[row] in fp64 (tc_vad_row), once per cache and
//                                 device
//   tune_vad_score_kernel<Rule>   one workgroup per (trial, file): tc_track_pair<Rule> (tune_core.h) with the
//                                 workgroup's barrier between its phases.  Every lane walks its steps of the file
//                                 twice; the ends of the lanes' latest turns, as an exclusive running maximum in lane
//                                 order, join the lanes' walks; lane 0 adds the lanes' sums in lane order and writes the
//                                 five components.  Instantiated three times:
//                                   TcPlainRule  taus (T,), a row is on when agg > tau.  No mask leaves the device:
//                                                this instantiation is launched for the components only.
//                                   TcHystRule   taus (T, 2) = (tau_active, tau_offset), DESIGN.md 4.21: a row's state
//                                                depends on the row before it, so each lane first runs the two-state
//                                                machine from both states over its rows and the lanes' state maps,
//                                                composed in lane order, give every lane the state its first row finds.
//                                                The masks come from this kernel too, for the same reason.
//                                   TcDurRule    taus (T, 4) = (tau_active, tau_offset, min_duration_on,
//                                                min_duration_off), DESIGN.md 4.22: TcHystRule's rows and masks; the
//                                                collar is max(collar, min_duration_off) and a merged span shorter than
//                                                min_duration_on does not count.  A span may cross any number of lanes:
//                                                every lane walks its steps once and leaves a summary (first span, last
//                                                span, the sums between), one lane composes the 256 summaries in order.
//   tune_vad_bits_kernel          one thread per (trial, row): agg > tau as the uint32 masks of the diarization replay
//                                 (VadTuneCache.replay with taus (T,); the tests compare them with the host's)
//
// The arithmetic is tune_core.h's, which the host compiles too (dz_tune_vad_host).  No contraction, as in k_tune.hip.
#pragma clang fp contract(off)
#include "dz_common.h"
#define TC_KERNEL_UNIT 1   // tune_core.h: TcDeviceLanes
#include "tune_core.h"

namespace {

constexpr int VAD_ROW_THREADS = 256;

__global__ __launch_bounds__(VAD_ROW_THREADS) void tune_vad_rows_kernel(dz_tune_desc d, double* __restrict__ agg) {
    const int p = blockIdx.x * VAD_ROW_THREADS + threadIdx.x;
    if (p < d.total_rows) agg[p] = tc_vad_row(d, p);
}

__global__ __launch_bounds__(VAD_ROW_THREADS) void tune_vad_bits_kernel(const double* __restrict__ agg,
                                                                        const double* __restrict__ taus, int trials,
                                                                        int total_rows, unsigned* __restrict__ bits) {
    const long long total = (long long)trials * total_rows;
    const long long i = (long long)blockIdx.x * VAD_ROW_THREADS + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i / total_rows), p = (int)(i - (long long)t * total_rows);
    bits[i] = agg[p] > taus[t] ? 1u : 0u;
}

// out (T, N, 5) and bits (T, total_rows) may each be NULL (tc_track_pair)
template <typename Rule>
__global__ __launch_bounds__(TC_TRACK_LANES) void tune_vad_score_kernel(
    const double* __restrict__ agg, const double* __restrict__ taus, int n_files, int total_rows,
    const int* __restrict__ file_chunk_off, const int* __restrict__ row_off, const double* __restrict__ mids,
    const int* __restrict__ mid_cell, const int* __restrict__ file_cell_off, const double* __restrict__ dur_prefix,
    const double* __restrict__ ref_prefix, double collar, double* __restrict__ out, unsigned* __restrict__ bits) {
    __shared__ TcTrackSharedOf<Rule> sh;
    const int pair = blockIdx.x;
    const int t = pair / n_files, n = pair - t * n_files;
    const long pre = (long)file_cell_off[n] + n;          // ncell + 1 prefix values per file
    const TcTrackIn in = {agg, row_off, mids, mid_cell, dur_prefix + pre, ref_prefix + pre, file_chunk_off[n],
                          file_chunk_off[n + 1], file_cell_off[n + 1] - file_cell_off[n], collar};
    // The stateless instantiation is launched for the components alone (its masks are tune_vad_bits_kernel's): it is
    // compiled without the mask loop, and with `out` known, so that no load waits behind a branch on it
    if constexpr (!Rule::stateful) __builtin_assume(out != nullptr);
    tc_track_pair(in, Rule::of(taus, t), sh, out ? out + (size_t)pair * 5 : nullptr,
                  Rule::stateful && bits ? bits + (size_t)t * total_rows : nullptr, TcDeviceLanes{TC_TRACK_LANES});
}

// The checks and the launches of dz_tune_vad_score under one rule.  The stateful rules take their masks from the pair
// kernel; the stateless one keeps them one thread per (trial, row).
template <typename Rule>
int track_score(dz_ctx* ctx, const dz_tune_cells* d_cells, int trials, const double* d_agg, const double* d_taus,
                double* d_out, unsigned* d_bits, void* stream) {
    const char* name = "dz_tune_vad_score";
    const char* missing = tc_cells_missing(d_cells, TC_CELLS_TRACK);
    DZ_REQUIRE(!missing && ctx && d_agg && d_taus && (d_out || d_bits), "%s: NULL argument (%s)", name,
               missing ? missing : "an array of the call");
    const dz_tune_cells& c = *d_cells;
    const int n_files = c.n_files, total_rows = c.total_rows;
    DZ_REQUIRE(trials >= 1 && n_files >= 1 && total_rows >= 1, "%s: empty shape (%d trials, %d files, %d rows)", name, trials,
               n_files, total_rows);
    const long long pairs = (long long)trials * n_files, rows = (long long)trials * total_rows;
    unsigned* pair_bits = Rule::stateful ? d_bits : nullptr;
    if (Rule::stateful)   // (the rows bound is the grid of tune_vad_bits_kernel, which this rule never launches)
        DZ_REQUIRE(pairs < (1ll << 31), "%s: %lld pairs in one call; evaluate fewer trials per batch", name, pairs);
    else
        DZ_REQUIRE(pairs < (1ll << 31) && rows < (1ll << 31) * VAD_ROW_THREADS,
                   "%s: %lld pairs / %lld rows in one call; evaluate fewer trials per batch", name, pairs, rows);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (d_out || pair_bits) {
        DZ_LAUNCH(tune_vad_score_kernel<Rule>, dim3((unsigned)pairs), dim3(TC_TRACK_LANES), 0, st, d_agg, d_taus, n_files,
                  total_rows, c.file_chunk_off, c.row_off, c.mids, c.mid_cell, c.file_cell_off, c.dur_prefix, c.ref_prefix,
                  c.collar, d_out, pair_bits);
        DZ_HIP(hipGetLastError());
    }
    if (d_bits && !pair_bits) {
        const long long blocks = (rows + VAD_ROW_THREADS - 1) / VAD_ROW_THREADS;
        DZ_LAUNCH(tune_vad_bits_kernel, dim3((unsigned)blocks), dim3(VAD_ROW_THREADS), 0, st, d_agg, d_taus, trials,
                  total_rows, d_bits);
        DZ_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" int dz_tune_vad_rows(dz_ctx* ctx, const dz_tune_desc* d, double* d_agg, void* stream) {
    DZ_REQUIRE(ctx && d && d_agg, "dz_tune_vad_rows: NULL argument");
    DZ_REQUIRE(d->seg && d->chunk_off && d->plan && d->row_off && d->row_chunk && d->hamming,
               "dz_tune_vad_rows: NULL pointer in the descriptor");
    DZ_REQUIRE(d->K == 1 && d->N >= 1 && d->F >= 1 && d->nwin >= 1 && d->total_chunks >= d->N && d->total_rows >= 1,
               "dz_tune_vad_rows: one track per chunk expected (k_local %d), %d files, %d chunks, %d rows", d->K, d->N,
               d->total_chunks, d->total_rows);
    DZ_HIP(hipSetDevice(ctx->device));
    const int blocks = (d->total_rows + VAD_ROW_THREADS - 1) / VAD_ROW_THREADS;
    DZ_LAUNCH(tune_vad_rows_kernel, dim3(blocks), dim3(VAD_ROW_THREADS), 0, (hipStream_t)stream, *d, d_agg);
    DZ_HIP(hipGetLastError());
    return 0;
}

// `cols`, the columns of d_taus, selects the rule.  With minimum durations (cols = 4) `taus_host` holds
// the same trials in host memory: the device form cannot read d_taus, and a duration that is negative or not finite is
// refused here, before the context, the descriptor or any device pointer is looked at.
extern "C" int dz_tune_vad_score(dz_ctx* ctx, const dz_tune_cells* d_cells, int cols, int trials, const double* d_agg,
                                 const double* taus_host, const double* d_taus, double* d_out, unsigned* d_bits,
                                 void* stream) {
    switch (cols) {
        case 1: return track_score<TcPlainRule>(ctx, d_cells, trials, d_agg, d_taus, d_out, d_bits, stream);
        case 2: return track_score<TcHystRule>(ctx, d_cells, trials, d_agg, d_taus, d_out, d_bits, stream);
        case 4: break;
        default:
            DZ_REQUIRE(false, "dz_tune_vad_score: taus of %d columns (1: tau_active; 2: and tau_offset; 4: and the two minimum "
                              "durations)", cols);
    }
    DZ_REQUIRE(taus_host, "dz_tune_vad_score: NULL argument (taus_host, which 4 columns need)");
    DZ_REQUIRE(trials >= 1, "dz_tune_vad_score: empty shape (%d trials)", trials);
    for (int t = 0; t < trials; ++t)
        for (int k = 2; k < 4; ++k) {
            const double v = taus_host[4 * (size_t)t + k];
            DZ_REQUIRE(v >= 0.0 && v <= 1.7976931348623157e308, "dz_tune_vad_score: %s of trial %d is %g, not a finite number >= 0",
                       k == 2 ? "min_duration_on" : "min_duration_off", t, v);
        }
    return track_score<TcDurRule>(ctx, d_cells, trials, d_agg, d_taus, d_out, d_bits, stream);
}
