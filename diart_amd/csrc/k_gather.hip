// dz_gather_windows: the rows of one file-batch step in ONE launch (DESIGN.md "File batches over every engine").
// A step of `FileBatch` carries the next few CONSECUTIVE windows of every open file: run i = `count` windows of
// `num_samples` floats, `hop` apart, of one file's resident audio, into the rows row0 .. row0 + count - 1 of the step's
// stage.  torch did this with one strided `unfold` + `copy_` per open file (up to 16 launches per step); here the runs
// travel BY VALUE in the kernel's arguments (no table upload, nothing the host has to keep alive) and one grid covers
// every row of every run.
//
// One workgroup per (row, column tile of GW_TILE floats).  The workgroup finds its run by walking the table (the index
// is the same for every lane: scalar loads from the argument segment), then copies its tile: 16-byte loads / stores when
// the window's first sample AND the destination row are 16-byte aligned (a tile starts a multiple of 16 bytes into its
// row, so one test serves the tile; uniform per workgroup), one float per lane otherwise (an odd hop, a source one
// float off).  The last S % 4 samples of a row always go one float at a time.  A pure copy: the bytes are the source's.
#include "dz_common.h"

namespace {

constexpr int GW_THREADS = 256;
constexpr int GW_QUADS = 4;                                // 16-byte pieces per lane, all loaded before the first store
constexpr int GW_TILE = GW_THREADS * GW_QUADS * 4;         // 4096 floats = 16 KB per workgroup

struct gather_table {
    dz_window_run run[DZ_GATHER_MAX_RUNS];                 // the non-empty runs of this launch
    int n;
};

// grid (total rows of the table * tiles), GW_THREADS threads
__global__ __launch_bounds__(GW_THREADS) void gather_windows_kernel(gather_table tab, int S, int hop,
                                                                    float* __restrict__ out, long long out_stride,
                                                                    int tiles) {
    int j = blockIdx.x / tiles;                            // row among the rows of the table ...
    const int tile = blockIdx.x - j * tiles;
    int i = 0;
    while (i < tab.n - 1 && j >= tab.run[i].count) {       // ... -> window j of run i (the host sized the grid: j fits)
        j -= tab.run[i].count;
        ++i;
    }
    const int c0 = tile * GW_TILE;
    const int n = min(GW_TILE, S - c0);
    const float* __restrict__ s = tab.run[i].src + (long long)j * hop + c0;
    float* __restrict__ d = out + (long long)(tab.run[i].row0 + j) * out_stride + c0;
    const int tid = threadIdx.x;
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
        const int nq = n >> 2;
        const f32x4* sq = reinterpret_cast<const f32x4*>(s);
        f32x4* dq = reinterpret_cast<f32x4*>(d);
        if (nq == GW_THREADS * GW_QUADS) {                 // a full tile: every load in flight before the stores
            f32x4 v[GW_QUADS];
#pragma unroll
            for (int u = 0; u < GW_QUADS; ++u) v[u] = sq[tid + u * GW_THREADS];
#pragma unroll
            for (int u = 0; u < GW_QUADS; ++u) dq[tid + u * GW_THREADS] = v[u];
        } else {
            for (int q = tid; q < nq; q += GW_THREADS) dq[q] = sq[q];
            if (4 * nq + tid < n) d[4 * nq + tid] = s[4 * nq + tid];
        }
    } else {
        for (int k = tid; k < n; k += GW_THREADS) d[k] = s[k];
    }
}

}  // namespace

extern "C" int dz_gather_windows(dz_ctx* ctx, const dz_window_run* runs, int n_runs, int num_samples, int hop,
                                 float* d_out, long long out_stride, int out_rows, void* stream) {
    DZ_REQUIRE(ctx && runs && d_out, "dz_gather_windows: NULL argument");
    DZ_REQUIRE(n_runs >= 1, "dz_gather_windows: %d runs", n_runs);
    DZ_REQUIRE(num_samples >= 1 && hop >= 1, "dz_gather_windows: windows of %d samples, %d apart", num_samples, hop);
    DZ_REQUIRE(out_rows >= 1 && out_stride >= num_samples,
               "dz_gather_windows: %d rows of stride %lld for windows of %d samples", out_rows, out_stride, num_samples);
    DZ_REQUIRE((((uintptr_t)d_out) & 3) == 0, "dz_gather_windows: %p is not a float address", (const void*)d_out);
    const int tiles = (num_samples + GW_TILE - 1) / GW_TILE;
    // every run is checked before the first launch: a refused call has written nothing
    for (int i = 0; i < n_runs; ++i) {
        const dz_window_run& r = runs[i];
        DZ_REQUIRE(r.count >= 0 && r.row0 >= 0 && (long long)r.row0 + r.count <= out_rows,
                   "dz_gather_windows: run %d covers rows %d .. %lld of %d", i, r.row0, (long long)r.row0 + r.count - 1,
                   out_rows);
        DZ_REQUIRE(r.count == 0 || (r.src && (((uintptr_t)r.src) & 3) == 0),
                   "dz_gather_windows: run %d reads from %p", i, (const void*)r.src);
        DZ_REQUIRE((long long)r.count * tiles <= 0x7fffffffLL / DZ_GATHER_MAX_RUNS,
                   "dz_gather_windows: run %d of %d windows exceeds the grid", i, r.count);
    }
    DZ_HIP(hipSetDevice(ctx->device));
    gather_table tab;
    tab.n = 0;
    long long rows = 0;
    for (int i = 0; i <= n_runs; ++i) {
        if (i < n_runs && runs[i].count > 0) {
            tab.run[tab.n++] = runs[i];
            rows += runs[i].count;
        }
        if (tab.n == DZ_GATHER_MAX_RUNS || (i == n_runs && tab.n > 0)) {
            DZ_LAUNCH(gather_windows_kernel, dim3((unsigned)(rows * tiles)), dim3(GW_THREADS), 0, (hipStream_t)stream,
                      tab, num_samples, hop, d_out, out_stride, tiles);
            DZ_HIP(hipGetLastError());
            tab.n = 0;
            rows = 0;
        }
    }
    return 0;
}
