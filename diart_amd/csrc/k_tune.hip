// Hyper-parameter tuning on cached model outputs (dz_tune_replay): T trials x N files replayed on the GPU.
//
//   tune_cluster_kernel   one wavefront per (trial, file) chain walks the file's chunks in order: dz_clu_step in fp64, its
//                         decisions compiled from the text cluster.cpp compiles (clu_core.h, here on the fixed store).  The
//                         K x G distances and the norms are spread over the lanes, each dot product summed by ONE lane in
//                         the core's order; lane 0 solves the assignment problems while the others wait at the barrier.  A
//                         workgroup is one wavefront and takes chains blockIdx.x, blockIdx.x + gridDim.x, ...; its centroids
//                         (G x D doubles, 80 KiB at 20 x 512) live in its own slice of a global work buffer that stays in
//                         L2 — LDS would hold one such chain per CU, and the lanes that wait for lane 0 need no bandwidth.
//   tune_mask_kernel      one thread per (trial, packed output row): tail.cpp's Hamming aggregation over the step's buffers
//                         in order, the quotient correctly rounded, `> tau` in fp64 -> one uint32 of speakers per row.
//
// Only the launch arguments differ from trial to trial.  No contraction anywhere in this file: a fused multiply-add
// rounds once where the host rounds twice, and the ties these sums decide are real (clustering_crowded.npz step 29).
#pragma clang fp contract(off)
#include "dz_common.h"
#include "tune_core.h"

namespace {

constexpr int TUNE_WAVE = 64;
constexpr int TUNE_MASK_THREADS = 256;

struct TuneBarrier {
    __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(TUNE_WAVE) void tune_cluster_kernel(dz_tune_desc d, const double* __restrict__ hp, int trials,
                                                                 signed char* __restrict__ assign, int* __restrict__ status,
                                                                 double* __restrict__ work) {
    __shared__ TcStep<CluFixed> s;
    const int lane = threadIdx.x;
    double* ctr = work + (size_t)blockIdx.x * d.D * d.G;
    const int chains = trials * d.N;
    for (int chain = blockIdx.x; chain < chains; chain += gridDim.x) {
        const int t = chain / d.N, n = chain - t * d.N;
        const int st = tc_chain(d, n, hp[3 * t], hp[3 * t + 1], hp[3 * t + 2], assign + (size_t)t * d.total_chunks * d.K, ctr,
                                s, lane, TUNE_WAVE, TuneBarrier());
        if (lane == 0) status[chain] = st;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TUNE_MASK_THREADS) void tune_mask_kernel(dz_tune_desc d, const double* __restrict__ hp, int trials,
                                                                      const signed char* __restrict__ assign,
                                                                      unsigned* __restrict__ bits) {
    const long long total = (long long)trials * d.total_rows;
    const long long i = (long long)blockIdx.x * TUNE_MASK_THREADS + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i / d.total_rows), p = (int)(i - (long long)t * d.total_rows);
    bits[i] = tc_row_mask(d, p, hp[3 * t], assign + (size_t)t * d.total_chunks * d.K);
}

}  // namespace

extern "C" int dz_tune_abi_size(void) { return (int)sizeof(dz_tune_desc); }

extern "C" int dz_tune_replay(dz_ctx* ctx, const dz_tune_desc* d, const double* d_hparams, int trials, signed char* d_assign,
                              int* d_status, unsigned* d_bits, double* d_work, int work_blocks, int phases, void* stream) {
    DZ_REQUIRE(ctx && d && d_hparams && d_assign && d_status && d_bits && d_work, "dz_tune_replay: NULL argument");
    DZ_REQUIRE(d->seg && d->emb && d->pre_max && d->pre_mean && d->pre_flags && d->chunk_off && d->plan && d->row_off &&
                   d->row_chunk && d->hamming, "dz_tune_replay: NULL pointer in the descriptor");
    DZ_REQUIRE(trials >= 1 && d->N >= 1 && d->F >= 1 && d->D >= 1 && d->nwin >= 1 && d->total_chunks >= d->N &&
                   d->total_rows >= 1 && work_blocks >= 1 && (phases & 3),
               "dz_tune_replay: empty shape (%d trials, %d files, %d chunks, %d rows)", trials, d->N, d->total_chunks,
               d->total_rows);
    DZ_REQUIRE(d->K >= 1 && d->K <= TC_KMAX && d->G >= 1 && d->G <= TC_GMAX,
               "dz_tune_replay: %d local / %d global speakers (at most %d / %d)", d->K, d->G, TC_KMAX, TC_GMAX);
    const long long chains = (long long)trials * d->N, rows = (long long)trials * d->total_rows;
    DZ_REQUIRE(chains < (1ll << 31) && rows < (1ll << 31) * TUNE_MASK_THREADS,
               "dz_tune_replay: %lld chains / %lld rows in one call; evaluate fewer trials per batch", chains, rows);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (phases & 1) {
        // a chain that stops early leaves -1 in the chunks it did not reach
        DZ_HIP(hipMemsetAsync(d_assign, 0xff, (size_t)trials * d->total_chunks * d->K, st));
        const int grid = (int)(chains < work_blocks ? chains : work_blocks);
        DZ_LAUNCH(tune_cluster_kernel, dim3(grid), dim3(TUNE_WAVE), 0, st, *d, d_hparams, trials, d_assign, d_status, d_work);
        DZ_HIP(hipGetLastError());
    }
    if (phases & 2) {
        const long long blocks = (rows + TUNE_MASK_THREADS - 1) / TUNE_MASK_THREADS;
        DZ_LAUNCH(tune_mask_kernel, dim3((unsigned)blocks), dim3(TUNE_MASK_THREADS), 0, st, *d, d_hparams, trials, d_assign,
                  d_bits);
        DZ_HIP(hipGetLastError());
    }
    return 0;
}
