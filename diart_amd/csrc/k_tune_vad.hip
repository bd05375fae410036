// Tuning VoiceActivityDetection on cached model outputs: there is no clustering and the Hamming
// aggregation does not depend on tau_active, so the aggregated speech score of every packed output row is computed
// once per cache and a trial is one comparison per row plus the detection error rate's bookkeeping.
// These kernels serve both track pipelines: OverlappedSpeechDetection (OsdTuneCache) feeds them the overlap track and
// the prefix sums of the reference's overlap regions.
//
//   tune_vad_rows_kernel    one thread per packed output row: agg[row] in fp64 (tc_vad_row), once per cache and device
//   tune_vad_score_kernel   one workgroup per (trial, file).  Lane i walks steps [i * per, (i + 1) * per) of the file
//                           twice (tc_vad_walk): first alone, for the end of its latest-ending turn; an exclusive
//                           running maximum of those ends over the lanes (-infinity for a lane without a turn, so it
//                           carries across any number of empty steps) is "the end of the last turn before this lane";
//                           then again from that end, summing the durations its turns add.  Lane 0 adds the lanes'
//                           sums in lane order and writes the five components.  No mask leaves the device.
//   tune_vad_bits_kernel    one thread per (trial, row): agg > tau as the uint32 masks of the diarization replay
//                           (VadTuneCache.replay; the tests compare them with the host's)
//   tune_vad_hyst_kernel    with an offset threshold (taus (T, 2)): one workgroup per (trial, file) for the components
//                           AND for the masks, because a row's state depends on the row before it.  Each lane first
//                           runs the two-state machine from both states over its rows; the lanes' state maps, composed
//                           in lane order, give every lane the state its first row finds (tc_hyst_pair, DESIGN.md
//                           4.21), and the two walks above then run on the stateful `on`.  (T,) input never comes here.
//
// The arithmetic is tune_core.h's, which the host compiles too (dz_tune_vad_host).  No contraction, as in k_tune.hip.
#pragma clang fp contract(off)
#include "dz_common.h"
#include "tune_core.h"

namespace {

constexpr int VAD_ROW_THREADS = 256;
constexpr int VAD_SCORE_THREADS = 256;

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

__global__ __launch_bounds__(VAD_SCORE_THREADS) void tune_vad_score_kernel(
    const double* __restrict__ agg, const double* __restrict__ taus, int n_files, const int* __restrict__ file_chunk_off,
    const int* __restrict__ row_off, const double* __restrict__ mids, const int* __restrict__ mid_cell,
    const int* __restrict__ file_cell_off, const double* __restrict__ dur_prefix, const double* __restrict__ ref_prefix,
    double collar, double* __restrict__ out) {
    __shared__ double end_e[VAD_SCORE_THREADS];
    __shared__ int end_cell[VAD_SCORE_THREADS];
    __shared__ double sum_hyp[VAD_SCORE_THREADS], sum_both[VAD_SCORE_THREADS];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int t = pair / n_files, n = pair - t * n_files;
    const double tau = taus[t];
    const int c0 = file_chunk_off[n], c1 = file_chunk_off[n + 1];
    const int per = tc_vad_steps_per_lane(c1 - c0, VAD_SCORE_THREADS);
    // (c0 + lane * per stays below c0 + chunks + 256 * per: no overflow for any file that fits an int)
    const int lo = c0 + (lane * per < c1 - c0 ? lane * per : c1 - c0);
    const int hi = lo + per < c1 ? lo + per : c1;
    const long pre = (long)file_cell_off[n] + n;          // ncell + 1 prefix values per file
    const double* dp = dur_prefix + pre;
    const double* rp = ref_prefix + pre;
    const TcVadEnd none = {-INFINITY, 0};
    TcVadSum scratch = {0.0, 0.0};
    const TcVadEnd own = tc_vad_walk(agg, row_off, mids, mid_cell, dp, rp, tau, collar, lo, hi, none, &scratch);
    end_e[lane] = own.e;
    end_cell[lane] = own.cell;
    __syncthreads();
    TcVadEnd before = none;
    for (int j = 0; j < lane; ++j)
        if (end_e[j] > before.e) {
            before.e = end_e[j];
            before.cell = end_cell[j];
        }
    TcVadSum s = {0.0, 0.0};
    tc_vad_walk(agg, row_off, mids, mid_cell, dp, rp, tau, collar, lo, hi, before, &s);
    sum_hyp[lane] = s.hyp;
    sum_both[lane] = s.both;
    __syncthreads();
    if (lane == 0) {
        TcVadSum all = {0.0, 0.0};
        for (int j = 0; j < VAD_SCORE_THREADS; ++j) {
            all.hyp += sum_hyp[j];
            all.both += sum_both[j];
        }
        const int ncell = file_cell_off[n + 1] - file_cell_off[n];
        tc_vad_components(rp[ncell], all, out + (size_t)pair * 5);
    }
}

struct HystLanes {
    int nl;
    template <typename F>
    __device__ void operator()(F f) const {
        f((int)threadIdx.x);
        __syncthreads();
    }
};

// taus (T, 2) = (tau_active, tau_offset); out (T, N, 5) and bits (T, total_rows) may each be NULL (tc_hyst_pair)
__global__ __launch_bounds__(TC_HYST_LANES) void tune_vad_hyst_kernel(
    const double* __restrict__ agg, const double* __restrict__ taus, int n_files, int total_rows,
    const int* __restrict__ file_chunk_off, const int* __restrict__ row_off, const double* __restrict__ mids,
    const int* __restrict__ mid_cell, const int* __restrict__ file_cell_off, const double* __restrict__ dur_prefix,
    const double* __restrict__ ref_prefix, double collar, double* __restrict__ out, unsigned* __restrict__ bits) {
    __shared__ TcHystShared sh;
    const int pair = blockIdx.x;
    const int t = pair / n_files, n = pair - t * n_files;
    const long pre = (long)file_cell_off[n] + n;          // ncell + 1 prefix values per file
    const TcHystIn in = {agg, row_off, mids, mid_cell, dur_prefix + pre, ref_prefix + pre, file_chunk_off[n],
                         file_chunk_off[n + 1], file_cell_off[n + 1] - file_cell_off[n], taus[2 * (size_t)t],
                         taus[2 * (size_t)t + 1], collar};
    tc_hyst_pair(in, sh, out ? out + (size_t)pair * 5 : nullptr, bits ? bits + (size_t)t * total_rows : nullptr,
                 HystLanes{TC_HYST_LANES});
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

extern "C" int dz_tune_vad_score(dz_ctx* ctx, int trials, int n_files, int total_rows, const double* d_agg,
                                 const double* d_taus, const int* d_file_chunk_off, const int* d_row_off,
                                 const double* d_mids, const int* d_mid_cell, const int* d_file_cell_off,
                                 const double* d_dur_prefix, const double* d_ref_prefix, double collar, double* d_out,
                                 unsigned* d_bits, void* stream) {
    DZ_REQUIRE(ctx && d_agg && d_taus && d_file_chunk_off && d_row_off && d_mids && d_mid_cell && d_file_cell_off &&
                   d_dur_prefix && d_ref_prefix && (d_out || d_bits), "dz_tune_vad_score: NULL argument");
    DZ_REQUIRE(trials >= 1 && n_files >= 1 && total_rows >= 1, "dz_tune_vad_score: empty shape (%d trials, %d files, %d rows)",
               trials, n_files, total_rows);
    const long long pairs = (long long)trials * n_files, rows = (long long)trials * total_rows;
    DZ_REQUIRE(pairs < (1ll << 31) && rows < (1ll << 31) * VAD_ROW_THREADS,
               "dz_tune_vad_score: %lld pairs / %lld rows in one call; evaluate fewer trials per batch", pairs, rows);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (d_out) {
        DZ_LAUNCH(tune_vad_score_kernel, dim3((unsigned)pairs), dim3(VAD_SCORE_THREADS), 0, st, d_agg, d_taus, n_files,
                  d_file_chunk_off, d_row_off, d_mids, d_mid_cell, d_file_cell_off, d_dur_prefix, d_ref_prefix, collar, d_out);
        DZ_HIP(hipGetLastError());
    }
    if (d_bits) {
        const long long blocks = (rows + VAD_ROW_THREADS - 1) / VAD_ROW_THREADS;
        DZ_LAUNCH(tune_vad_bits_kernel, dim3((unsigned)blocks), dim3(VAD_ROW_THREADS), 0, st, d_agg, d_taus, trials,
                  total_rows, d_bits);
        DZ_HIP(hipGetLastError());
    }
    return 0;
}

// With hysteresis: d_taus (T, 2) = (tau_active, tau_offset) per trial; everything else is dz_tune_vad_score's.
extern "C" int dz_tune_vad_score_hyst(dz_ctx* ctx, int trials, int n_files, int total_rows, const double* d_agg,
                                      const double* d_taus, const int* d_file_chunk_off, const int* d_row_off,
                                      const double* d_mids, const int* d_mid_cell, const int* d_file_cell_off,
                                      const double* d_dur_prefix, const double* d_ref_prefix, double collar,
                                      double* d_out, unsigned* d_bits, void* stream) {
    DZ_REQUIRE(ctx && d_agg && d_taus && d_file_chunk_off && d_row_off && d_mids && d_mid_cell && d_file_cell_off &&
                   d_dur_prefix && d_ref_prefix && (d_out || d_bits), "dz_tune_vad_score_hyst: NULL argument");
    DZ_REQUIRE(trials >= 1 && n_files >= 1 && total_rows >= 1,
               "dz_tune_vad_score_hyst: empty shape (%d trials, %d files, %d rows)", trials, n_files, total_rows);
    const long long pairs = (long long)trials * n_files;
    DZ_REQUIRE(pairs < (1ll << 31), "dz_tune_vad_score_hyst: %lld pairs in one call; evaluate fewer trials per batch", pairs);
    DZ_HIP(hipSetDevice(ctx->device));
    DZ_LAUNCH(tune_vad_hyst_kernel, dim3((unsigned)pairs), dim3(TC_HYST_LANES), 0, (hipStream_t)stream, d_agg, d_taus,
              n_files, total_rows, d_file_chunk_off, d_row_off, d_mids, d_mid_cell, d_file_cell_off, d_dur_prefix,
              d_ref_prefix, collar, d_out, d_bits);
    DZ_HIP(hipGetLastError());
    return 0;
}
