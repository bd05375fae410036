// Centroid-linkage agglomerative clustering on the device (dz_agglo_linkage): the dendrogram Z of every
// file of a call, float64 throughout, from the text of agglo_core.h.
//
//   agglo_pdist_kernel     the (n, n) squared distances of a file's unit rows: 64 x 64 tiles, 4 x 4 outputs per lane,
//                          the rows' terms added in ascending k whatever the tile (one sequential chain per output)
//   agglo_nn_init_kernel   one wavefront per row: its nearest slot above it, and the slot's initial state
//   agglo_merge_kernel     ONE workgroup per file runs that file's merges one after another, `nsteps` of them per
//                          launch, the state in device memory between launches.  The merges are agglo_core.h's
//                          ag_merge_steps, the loop the host runs too, on the kernel's team (AgBlockTeam: 1 024
//                          lanes, __syncthreads(), ag_block_min); the kernel keeps the entry checks and the last store.
// No workgroup waits for another one: a file's merges are ordered inside its own workgroup by __syncthreads(), the
// launches by the stream.  The host reads nothing back between launches.  There is no atomic of any kind.
// Every index read from device memory is range-checked before it indexes anything: a failed check ends the file with
// its status set to the merge it happened at.
#include "dz_common.h"
#include "agglo_core.h"

#include <vector>

namespace {

struct AgFile {
    long long mat;     // first element of the file's matrix
    long long z;       // first row of the file's Z
    int row0, n;
};

constexpr int AG_TILE = 64, AG_KC = 16;
constexpr int AG_MERGE_THREADS = 1024, AG_MERGE_WAVES = AG_MERGE_THREADS / 64;
constexpr int AG_STEPS_PER_LAUNCH = 2048;
constexpr int AG_MAX_FILES = 1024;

__global__ __launch_bounds__(256) void agglo_pdist_kernel(const AgFile* __restrict__ files, const double* __restrict__ x,
                                                          int D, double* __restrict__ mat) {
    const AgFile f = files[blockIdx.z];
    const int n = f.n, bi = blockIdx.y * AG_TILE, bj = blockIdx.x * AG_TILE;
    if (bi >= n || bj >= n) return;               // the whole workgroup, before its first barrier
    __shared__ double A[AG_TILE][AG_KC + 1], B[AG_TILE][AG_KC + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const double* xf = x + (long long)f.row0 * D;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int k0 = 0; k0 < D; k0 += AG_KC) {
        for (int e = threadIdx.x; e < AG_TILE * AG_KC; e += 256) {
            const int r = e >> 4, c = e & 15;
            const bool kin = k0 + c < D;
            A[r][c] = (kin && bi + r < n) ? xf[(long long)(bi + r) * D + k0 + c] : 0.0;
            B[r][c] = (kin && bj + r < n) ? xf[(long long)(bj + r) * D + k0 + c] : 0.0;
        }
        __syncthreads();
        const int kc = D - k0 < AG_KC ? D - k0 : AG_KC;
        for (int c = 0; c < kc; ++c) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = A[ty * 4 + u][c];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = B[tx * 4 + v][c];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = ag_d2_term(acc[u][v], a[u], b[v]);
        }
        __syncthreads();
    }
    double* mf = mat + f.mat;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = bi + ty * 4 + u;
        if (r >= n) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int c = bj + tx * 4 + v;
            if (c < n) mf[(long long)r * n + c] = acc[u][v];
        }
    }
}

// the lowest (value, index) of a wavefront's lanes, in every lane of it
__device__ __forceinline__ void ag_wave_min(double& best, int& bidx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        ag_take(ov, oi, best, bidx);
    }
}

// row k's nearest active slot above it (lane: 0 .. 63 of one wavefront)
__device__ __forceinline__ void ag_scan_row(const double* row, const int* active, int k, int n,
                                            int lane, double& best, int& bidx) {
    best = INFINITY;
    bidx = AG_NONE;
    for (int m = k + 1 + lane; m < n; m += 64)
        if (active == nullptr || active[m]) ag_take(row[m], m, best, bidx);
    ag_wave_min(best, bidx);
}

__global__ __launch_bounds__(256) void agglo_nn_init_kernel(const AgFile* __restrict__ files, const double* __restrict__ mat,
                                                            double* __restrict__ nn_val, int* __restrict__ nn_idx,
                                                            int* __restrict__ size, int* __restrict__ id,
                                                            int* __restrict__ active, int* __restrict__ stale,
                                                            int* __restrict__ step, int* __restrict__ status) {
    const AgFile f = files[blockIdx.y];
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        step[blockIdx.y] = 0;
        status[blockIdx.y] = AG_OK;
    }
    if (k >= f.n) return;                         // a whole wavefront; the kernel has no barrier
    double best;
    int bidx;
    ag_scan_row(mat + f.mat + (long long)k * f.n, nullptr, k, f.n, lane, best, bidx);
    if (lane == 0) {
        const int s = f.row0 + k;
        nn_val[s] = best;
        nn_idx[s] = bidx == AG_NONE ? -1 : bidx;
        size[s] = 1;
        id[s] = k;
        active[s] = 1;
        stale[s] = 0;
    }
}

// the lowest (value, index) over the workgroup, in every thread of it.  Two barriers: call from all threads.
__device__ __forceinline__ void ag_block_min(double& best, int& bidx, double* s_val, int* s_idx) {
    ag_wave_min(best, bidx);
    if ((threadIdx.x & 63) == 0) {
        s_val[threadIdx.x >> 6] = best;
        s_idx[threadIdx.x >> 6] = bidx;
    }
    __syncthreads();
    best = s_val[0];
    bidx = s_idx[0];
#pragma unroll
    for (int w = 1; w < AG_MERGE_WAVES; ++w) ag_take(s_val[w], s_idx[w], best, bidx);
    __syncthreads();                              // s_val / s_idx are free again
}

// the team of agglo_core.h's merge loop on the device: the workgroup's AG_MERGE_THREADS threads
struct AgBlockTeam {
    double* s_val;     // AG_MERGE_WAVES each, LDS
    int* s_idx;
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return AG_MERGE_THREADS; }
    __device__ void barrier() const { __syncthreads(); }
    __device__ void lowest(double& v, int& idx) const { ag_block_min(v, idx, s_val, s_idx); }
};

__global__ __launch_bounds__(AG_MERGE_THREADS) void agglo_merge_kernel(
    const AgFile* __restrict__ files, int* step, double* g_nn_val, int* g_nn_idx,
    int* g_size, int* g_id, int* g_active, int* g_stale,
    double* g_mat, double* g_z, int* status, int nsteps) {
    const AgFile f = files[blockIdx.x];
    const int n = f.n;
    if (n < 2 || status[blockIdx.x] != AG_OK) return;          // the whole workgroup
    int t = step[blockIdx.x];
    if (t < 0 || t >= n - 1) return;                           // a finished file does nothing
    const AgSlots s = {g_nn_val + f.row0, g_nn_idx + f.row0, g_size + f.row0, g_id + f.row0,
                       g_active + f.row0, g_stale + f.row0, g_mat + f.mat,    g_z + f.z * 4};
    __shared__ double s_val[AG_MERGE_WAVES];
    __shared__ int s_idx[AG_MERGE_WAVES];
    bool bad = false;
    t = ag_merge_steps(s, n, t, nsteps, &bad, AgBlockTeam{s_val, s_idx});
    if (threadIdx.x == 0) {
        step[blockIdx.x] = t;
        if (bad) status[blockIdx.x] = t;
    }
}

struct AgLayout {
    size_t files, step, nn_val, nn_idx, size, id, active, stale, mat, total;
};

// the workspace of a call; false when rows_off is no ascending list from 0
bool ag_layout(int n_files, const int* rows_off, AgLayout& L, std::vector<AgFile>* desc) {
    if (!ag_offsets_ok(n_files, rows_off)) return false;
    long long mat = 0, z = 0;
    for (int f = 0; f < n_files; ++f) {
        const long long n = (long long)rows_off[f + 1] - rows_off[f];
        if (desc) desc->push_back(AgFile{mat, z, rows_off[f], (int)n});
        mat += n * n;
        z += n > 1 ? n - 1 : 0;
    }
    const size_t R = (size_t)rows_off[n_files];
    Arena a;
    L.files = a.used; a.take<AgFile>((size_t)n_files);
    L.step = a.used; a.take<int>((size_t)n_files);
    L.nn_val = a.used; a.take<double>(R);
    L.nn_idx = a.used; a.take<int>(R);
    L.size = a.used; a.take<int>(R);
    L.id = a.used; a.take<int>(R);
    L.active = a.used; a.take<int>(R);
    L.stale = a.used; a.take<int>(R);
    L.mat = a.used; a.take<double>((size_t)mat);
    L.total = a.used;
    return true;
}

}  // namespace

extern "C" long long dz_agglo_work_bytes(int n_files, const int* rows_off) {
    AgLayout L;
    if (!rows_off || n_files < 1 || n_files > AG_MAX_FILES || !ag_layout(n_files, rows_off, L, nullptr)) {
        dz_set_error("dz_agglo_work_bytes: 1 .. %d files and an ascending rows_off from 0 expected", AG_MAX_FILES);
        return -1;
    }
    return (long long)(L.total > 0 ? L.total : 256);
}

extern "C" int dz_agglo_linkage(dz_ctx* ctx, int n_files, const int* rows_off, const double* d_x, int D, double* d_Z,
                                int* d_status, void* d_work, long long work_bytes, void* stream) {
    DZ_REQUIRE(ctx && rows_off && d_status && d_work, "dz_agglo_linkage: NULL argument");
    DZ_REQUIRE(n_files >= 1 && n_files <= AG_MAX_FILES, "dz_agglo_linkage: %d files outside [1, %d]", n_files, AG_MAX_FILES);
    DZ_REQUIRE(D >= 1 && D <= AG_DMAX, "dz_agglo_linkage: dimension %d outside [1, %d]", D, AG_DMAX);
    AgLayout L;
    std::vector<AgFile> desc;
    DZ_REQUIRE(ag_layout(n_files, rows_off, L, &desc), "dz_agglo_linkage: rows_off is no ascending list from 0");
    DZ_REQUIRE(work_bytes >= (long long)L.total, "dz_agglo_linkage: workspace of %lld bytes, %zu needed (dz_agglo_work_bytes)",
               work_bytes, L.total);
    int max_n = 0;
    for (const AgFile& f : desc) max_n = f.n > max_n ? f.n : max_n;
    DZ_REQUIRE(max_n <= 1 || (d_x && d_Z), "dz_agglo_linkage: NULL argument");
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)d_work;
    AgFile* files = (AgFile*)(w + L.files);
    DZ_HIP(hipMemcpyAsync(files, desc.data(), sizeof(AgFile) * (size_t)n_files, hipMemcpyHostToDevice, st));
    DZ_HIP(hipStreamSynchronize(st));             // desc leaves scope with this call; the copy has read it
    int* step = (int*)(w + L.step);
    double* nn_val = (double*)(w + L.nn_val);
    int *nn_idx = (int*)(w + L.nn_idx), *size = (int*)(w + L.size), *id = (int*)(w + L.id);
    int *active = (int*)(w + L.active), *stale = (int*)(w + L.stale);
    double* mat = (double*)(w + L.mat);
    if (max_n < 1) max_n = 1;
    const int tiles = (max_n + AG_TILE - 1) / AG_TILE;
    if (max_n > 1) {
        DZ_LAUNCH(agglo_pdist_kernel, dim3(tiles, tiles, n_files), dim3(256), 0, st, files, d_x, D, mat);
        DZ_HIP(hipGetLastError());
    }
    DZ_LAUNCH(agglo_nn_init_kernel, dim3((max_n + 3) / 4, n_files), dim3(256), 0, st, files, mat, nn_val, nn_idx, size, id,
              active, stale, step, d_status);
    DZ_HIP(hipGetLastError());
    for (int done = 0; done < max_n - 1; done += AG_STEPS_PER_LAUNCH) {
        DZ_LAUNCH(agglo_merge_kernel, dim3(n_files), dim3(AG_MERGE_THREADS), 0, st, files, step, nn_val, nn_idx, size, id,
                  active, stale, mat, d_Z, d_status, AG_STEPS_PER_LAUNCH);
        DZ_HIP(hipGetLastError());
    }
    return 0;
}
