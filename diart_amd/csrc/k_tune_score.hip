// Scoring SpeakerDiarization tuning trials on the device (dz_tune_score_gpu): the masks that
// tune_mask_kernel wrote stay where they are, and a batch of T trials over N files leaves T x N x 5 doubles.
//
//   tune_score_kernel   one workgroup of 256 lanes per (trial, file) pair, pairs blockIdx.x, blockIdx.x + gridDim.x, ...
//                       Per label of the pair, lane i walks steps [i * per, (i + 1) * per) of the file twice, as
//                       tune_vad_score_kernel does, and every range of cells a merged turn adds toggles bit g of the two
//                       words at its ends in the workgroup's slice of a global scratch array (cells + 1 words of the
//                       largest file; integer atomic XOR).  A prefix XOR over the slice gives the hypothesis mask of
//                       every scoring cell; the sums over the cells (popcounts of the 64-bit reference and the 32-bit
//                       hypothesis mask; the co-occurrence matrix eight entries per pass) are formed per lane and added in
//                       lane order; lane 0 solves the mapping's assignment problem (tc_lsap on a 32 x 64 store in LDS).
//
// The slice is reused by the next pair the workgroup takes and is zeroed at the start of every pair; LDS is written
// before it is read.  A turn that does not lie on the file's cells (dz_tune_score's rc 4) and a failed assignment
// problem (rc 3) raise the call's error word and touch nothing out of range.  No floating-point atomics: two calls give
// the same doubles.  The arithmetic is tune_core.h's, which the host compiles too (dz_tune_score_core); what differs
// from dz_tune_score is the order of the sums.  No contraction, as in k_tune.hip.
#pragma clang fp contract(off)
#include "dz_common.h"
#define TC_KERNEL_UNIT 1   // tune_core.h: TcDeviceLanes
#include "tune_core.h"

namespace {

__global__ __launch_bounds__(TC_SCORE_LANES) void tune_score_kernel(
    const unsigned* __restrict__ bits, int trials, int n_files, int total_rows, const int* __restrict__ file_chunk_off,
    const int* __restrict__ row_off, const double* __restrict__ mids, const int* __restrict__ mid_cell,
    const int* __restrict__ file_cell_off, const double* __restrict__ cell_dur,
    const unsigned long long* __restrict__ cell_ref, int max_cells, int max_speakers, double collar,
    double* __restrict__ out, unsigned* scratch, int* err) {
    __shared__ TcScoreShared sh;
    unsigned* slice = scratch + (size_t)blockIdx.x * ((size_t)max_cells + 1);
    const TcScoreCall call = {bits, trials, n_files, total_rows, file_chunk_off, row_off, mids, mid_cell, file_cell_off,
                              cell_dur, cell_ref, max_cells, max_speakers, collar};
    tc_score_pairs(call, blockIdx.x, gridDim.x, threadIdx.x == 0, err, [&](long long pair, int, int, const TcScoreIn& in) {
        tc_score_pair(in, sh, slice, out + (size_t)pair * 5, err, TcDeviceLanes{TC_SCORE_LANES});
    });
}

}  // namespace

extern "C" int dz_tune_score_gpu(dz_ctx* ctx, const dz_tune_cells* d_cells, int trials, const unsigned* d_bits,
                                 double* d_out, unsigned* d_scratch, int score_blocks, int* d_err, void* stream) {
    const char* missing = tc_cells_missing(d_cells, TC_CELLS_KERNEL);
    DZ_REQUIRE(!missing && ctx && d_bits && d_out && d_scratch && d_err, "dz_tune_score_gpu: NULL argument (%s)",
               missing ? missing : "an array of the call");
    const dz_tune_cells& c = *d_cells;
    DZ_REQUIRE(trials >= 1 && c.n_files >= 1 && c.total_rows >= 1 && c.max_cells >= 0 && score_blocks >= 1 &&
                   c.max_speakers >= 1 && c.max_speakers <= TC_GMAX,
               "dz_tune_score_gpu: bad arguments (%d trials, %d files, %d rows, %d cells per slice, %d slices, %d speakers)",
               trials, c.n_files, c.total_rows, c.max_cells, score_blocks, c.max_speakers);
    const long long pairs = (long long)trials * c.n_files;
    DZ_REQUIRE(pairs < (1ll << 31), "dz_tune_score_gpu: %lld pairs in one call; evaluate fewer trials per batch", pairs);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    DZ_HIP(hipMemsetAsync(d_err, 0, sizeof(int), st));
    const int grid = (int)(pairs < score_blocks ? pairs : score_blocks);
    DZ_LAUNCH(tune_score_kernel, dim3(grid), dim3(TC_SCORE_LANES), 0, st, d_bits, trials, c.n_files, c.total_rows,
              c.file_chunk_off, c.row_off, c.mids, c.mid_cell, c.file_cell_off, c.cell_dur, c.cell_ref, c.max_cells,
              c.max_speakers, c.collar, d_out, d_scratch, d_err);
    DZ_HIP(hipGetLastError());
    return 0;
}
