// Tuning delta_id by replay (dz_tune_name and dz_tune_ident_score_gpu): the names
// a gallery gives the global speakers of every trial, and the identification error rate of every (trial, file) pair,
// from the assignments and masks that dz_tune_replay left on the device -- at one (plane, threshold) point per trial, or
// at up to 256 of them for the price of one clustering replay.
//
//   tune_name_kernel          one wavefront per (trial, point, file) chain, sequential over the file's chunks.  Lane
//                             g < G holds speaker g's closest match so far (best_d, best_e) in registers; a step reads
//                             the chunk's K assignments and its stored match in the point's plane (the same addresses
//                             for every lane), and the holder conflicts are settled by G shuffles.  It writes one byte
//                             per (chunk, g): the reference bit of the name g carries in that step, or "other"; and the
//                             holder itself where asked.  Chunks from the chain's status on change nothing (their
//                             assignments are -1 anyway).
//   tune_ident_score_kernel   one workgroup of 256 lanes per (trial, file) pair, pairs blockIdx.x, blockIdx.x +
//                             gridDim.x, ...: the toggle and prefix-XOR phases of tune_score_kernel (tc_score_cells) on
//                             a scratch slice ONCE, then for every point in turn: per cell the identities of the step
//                             that owns it, popcounts, five sums per lane added in lane order by lane 0.  No assignment
//                             problem, no co-occurrence sweep, 15 KB of LDS.
//
// One point is points = planes = 1 of the same entries.  Both kernels are latency-sized (a chain is
// a dependent walk; a pair is a few thousand cells).  Vector stores only, no floating-point atomics: two calls give
// the same doubles.  The arithmetic is tune_ident_core.h's, which the host compiles too.  No contraction, as in
// k_tune.hip.
#pragma clang fp contract(off)
#include "dz_common.h"
#define TC_KERNEL_UNIT 1   // tune_core.h: TcDeviceLanes
#include "tune_ident_core.h"

namespace {

constexpr int NAME_WAVE = 64;

__global__ __launch_bounds__(NAME_WAVE) void tune_name_kernel(
    int trials, int points, int planes, int n_files, int total_chunks, int K, int G, int V,
    const int* __restrict__ file_chunk_off, const signed char* __restrict__ assign, const int* __restrict__ status,
    const int* __restrict__ match_index, const float* __restrict__ match_distance, const signed char* __restrict__ vp_ref,
    const double* __restrict__ delta_id, signed char* __restrict__ ident, int* __restrict__ hold) {
    const int g = threadIdx.x;
    const long long chains = (long long)trials * points * n_files;
    for (long long chain = blockIdx.x; chain < chains; chain += gridDim.x) {
        const TiChain ch = ti_chain(chain, points, planes, n_files);
        const int n = ch.n;
        const int c0 = file_chunk_off[n], c1 = file_chunk_off[n + 1];
        const int st = status[(long long)ch.t * n_files + n];
        const int stop = st < 0 ? c1 : (c0 + st < c1 ? c0 + st : c1);
        const size_t tj = (size_t)ch.t * points + ch.j;
        const double delta = delta_id[tj];
        const signed char* A = assign + (size_t)ch.t * total_chunks * K;
        const int* MI = match_index + (size_t)ch.plane * total_chunks * K;
        const float* MD = match_distance + (size_t)ch.plane * total_chunks * K;
        signed char* I = ident + tj * total_chunks * G;
        int* H = hold ? hold + tj * total_chunks * G : nullptr;
        float best_d = INFINITY;
        int best_e = -1;
        for (int c = c0; c < c1; ++c) {
            if (c < stop) ti_update(best_d, best_e, g, A + (size_t)c * K, MI + (size_t)c * K, MD + (size_t)c * K, K, delta);
            const int h = ti_hold(best_d, best_e, g, G, [&](int g2, float* d2, int* e2) {
                *d2 = __shfl(best_d, g2, NAME_WAVE);
                *e2 = __shfl(best_e, g2, NAME_WAVE);
            });
            if (g < G) {
                I[(size_t)c * G + g] = ti_identity(h, vp_ref + (size_t)n * V, V);
                if (H) H[(size_t)c * G + g] = h;
            }
        }
    }
}

__global__ __launch_bounds__(TC_SCORE_LANES) void tune_ident_score_kernel(
    const unsigned* __restrict__ bits, const signed char* __restrict__ ident, int trials, int points, int n_files,
    int total_rows, int total_chunks, const int* __restrict__ file_chunk_off, const int* __restrict__ row_off,
    const double* __restrict__ mids, const int* __restrict__ mid_cell, const int* __restrict__ file_cell_off,
    const double* __restrict__ cell_dur, const unsigned long long* __restrict__ cell_ref, const int* __restrict__ cell_step,
    int max_cells, int max_speakers, double collar, double* __restrict__ out, unsigned* scratch, int* err) {
    __shared__ TiScoreShared sh;
    unsigned* slice = scratch + (size_t)blockIdx.x * ((size_t)max_cells + 1);
    const TcScoreCall call = {bits, trials, n_files, total_rows, file_chunk_off, row_off, mids, mid_cell, file_cell_off,
                              cell_dur, cell_ref, max_cells, max_speakers, collar};
    const long long plane = (long long)total_chunks * max_speakers;   // one point's identities of one trial
    tc_score_pairs(call, blockIdx.x, gridDim.x, threadIdx.x == 0, err, [&](long long pair, int t, int cell0, const TcScoreIn& cells) {
        const int n = (int)(pair - (long long)t * n_files);
        const TiScoreIn in = {cells, ident + (size_t)t * points * plane, cell_step + cell0};
        ti_score_pair(in, points, plane, (long long)n_files * 5, sh, slice, out + ((size_t)t * points * n_files + n) * 5, err,
                      TcDeviceLanes{TC_SCORE_LANES});
    });
}

}  // namespace

extern "C" int dz_tune_name(dz_ctx* ctx, int trials, int points, int planes, int n_files, int total_chunks,
                                  int k_local, int max_speakers, int voiceprints, const int* d_file_chunk_off,
                                  const signed char* d_assign, const int* d_status, const int* d_match_index,
                                  const float* d_match_distance, const signed char* d_vp_ref, const double* d_delta_id,
                                  signed char* d_ident, int* d_hold, int name_blocks, void* stream) {
    DZ_REQUIRE(ctx && d_file_chunk_off && d_assign && d_status && d_match_index && d_match_distance && d_vp_ref &&
                   d_delta_id && d_ident, "dz_tune_name: NULL argument");
    DZ_REQUIRE(trials >= 1 && n_files >= 1 && total_chunks >= n_files && k_local >= 1 && k_local <= TC_KMAX &&
                   max_speakers >= 1 && max_speakers <= TC_GMAX && voiceprints >= 1 && name_blocks >= 1,
               "dz_tune_name: bad arguments (%d trials, %d files, %d chunks, %d local / %d global speakers (at most %d / "
               "%d), %d voiceprints, %d workgroups)",
               trials, n_files, total_chunks, k_local, max_speakers, TC_KMAX, TC_GMAX, voiceprints, name_blocks);
    DZ_REQUIRE(points >= 1 && points <= TI_MAX_POINTS && planes >= 1 && planes <= TI_MAX_PLANES && points % planes == 0,
               "dz_tune_name: %d points (1 .. %d) in %d planes (1 .. %d, a divisor of the points)", points,
               TI_MAX_POINTS, planes, TI_MAX_PLANES);
    const long long chains = (long long)trials * points * n_files;
    DZ_REQUIRE(chains < (1ll << 31), "dz_tune_name: %lld chains in one call; evaluate fewer trials per batch", chains);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)(chains < name_blocks ? chains : name_blocks);
    DZ_LAUNCH(tune_name_kernel, dim3(grid), dim3(NAME_WAVE), 0, st, trials, points, planes, n_files, total_chunks, k_local,
              max_speakers, voiceprints, d_file_chunk_off, d_assign, d_status, d_match_index, d_match_distance, d_vp_ref,
              d_delta_id, d_ident, d_hold);
    DZ_HIP(hipGetLastError());
    return 0;
}

extern "C" int dz_tune_ident_score_gpu(dz_ctx* ctx, const dz_tune_cells* d_cells, int trials, int points,
                                       const unsigned* d_bits, const signed char* d_ident, double* d_out,
                                       unsigned* d_scratch, int score_blocks, int* d_err, void* stream) {
    const char* missing = tc_cells_missing(d_cells, TC_CELLS_KERNEL | TC_CELLS_CELL_STEP);
    DZ_REQUIRE(!missing && ctx && d_bits && d_ident && d_out && d_scratch && d_err,
               "dz_tune_ident_score_gpu: NULL argument (%s)", missing ? missing : "an array of the call");
    const dz_tune_cells& c = *d_cells;
    DZ_REQUIRE(trials >= 1 && c.n_files >= 1 && c.total_rows >= 1 && c.total_chunks >= c.n_files && c.max_cells >= 0 &&
                   score_blocks >= 1 && c.max_speakers >= 1 && c.max_speakers <= TC_GMAX,
               "dz_tune_ident_score_gpu: bad arguments (%d trials, %d files, %d rows, %d chunks, %d cells per slice, %d "
               "slices, %d speakers (at most %d))",
               trials, c.n_files, c.total_rows, c.total_chunks, c.max_cells, score_blocks, c.max_speakers, TC_GMAX);
    DZ_REQUIRE(points >= 1 && points <= TI_MAX_POINTS, "dz_tune_ident_score_gpu: %d points (1 .. %d)", points, TI_MAX_POINTS);
    const long long pairs = (long long)trials * c.n_files;
    DZ_REQUIRE(pairs * points < (1ll << 31),
               "dz_tune_ident_score_gpu: %lld pairs x %d points in one call; evaluate fewer trials per batch", pairs, points);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    DZ_HIP(hipMemsetAsync(d_err, 0, sizeof(int), st));
    const int grid = (int)(pairs < score_blocks ? pairs : score_blocks);
    DZ_LAUNCH(tune_ident_score_kernel, dim3(grid), dim3(TC_SCORE_LANES), 0, st, d_bits, d_ident, trials, points, c.n_files,
              c.total_rows, c.total_chunks, c.file_chunk_off, c.row_off, c.mids, c.mid_cell, c.file_cell_off, c.cell_dur,
              c.cell_ref, c.cell_step, c.max_cells, c.max_speakers, c.collar, d_out, d_scratch, d_err);
    DZ_HIP(hipGetLastError());
    return 0;
}
