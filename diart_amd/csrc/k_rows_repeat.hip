// "How often is every row of this batch repeated?" — the detector behind repeated_rows="share" (dz_rows_repeat,
// DESIGN.md 4.11).  The reference hands the embedding model every waveform num_speakers times; only the pooling depends
// on the speaker, so a model that knows the repetition R runs its trunk on n / R rows.
//
//   rows_differ_kernel   row i against row i - 1 as 32-bit words (bitwise: equal NaN patterns are equal, -0.0 and +0.0
//                        are not); a thread that meets a difference stores 1 into differs[i].  Every writer stores the
//                        same value: no atomics.  Memory bound: a workgroup walks RR_ROWS + 1 consecutive rows of one
//                        column strip and keeps the predecessor's words in registers, so a row is read (RR_ROWS + 1) /
//                        RR_ROWS times and all loads of a thread are independent.
//   rows_repeat_kernel   one workgroup: R = gcd(n, every i with differs[i]) — the boundaries of the runs of equal rows
//                        sit at 0, at the flagged rows and at n, so that is the gcd of n and the run lengths — and the
//                        flags are cleared for the next call.
#include "dz_common.h"

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_PER = 2;        // words per thread and row
constexpr int RR_ROWS = 8;       // compared rows per workgroup (+ 1 predecessor)

__device__ __forceinline__ uint32_t rr_diff(uint32_t a, uint32_t b) { return a ^ b; }
__device__ __forceinline__ uint32_t rr_diff(uint4 a, uint4 b) {
    return (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
}

// T = uint4 when every row starts on a 16-byte boundary (base aligned, stride a multiple of 4 samples: the only case in
// which two neighbouring rows are both aligned), uint32_t otherwise.  grid = (strips, row groups).
template <typename T>
__global__ __launch_bounds__(RR_THREADS) void rows_differ_kernel(const uint32_t* __restrict__ wave, long long stride,
                                                                 int n_rows, int S, int* __restrict__ differs) {
    constexpr int W = (int)(sizeof(T) / sizeof(uint32_t));
    const int nw = S / W;                                       // whole words of a row
    const int r0 = blockIdx.y * RR_ROWS;                        // the group's first predecessor
    const int nr = min(RR_ROWS, n_rows - 1 - r0);               // rows r0 + 1 .. r0 + nr are compared
    const int w0 = blockIdx.x * (RR_THREADS * RR_PER) + threadIdx.x;
    T v[RR_ROWS + 1][RR_PER];
#pragma unroll
    for (int j = 0; j <= RR_ROWS; ++j) {
        const T* row = reinterpret_cast<const T*>(wave + (long long)(r0 + min(j, nr)) * stride);
#pragma unroll
        for (int k = 0; k < RR_PER; ++k) {
            const int w = w0 + k * RR_THREADS;
            v[j][k] = w < nw ? row[w] : T{};
        }
    }
#pragma unroll
    for (int j = 1; j <= RR_ROWS; ++j) {
        uint32_t d = 0;
#pragma unroll
        for (int k = 0; k < RR_PER; ++k) d |= rr_diff(v[j][k], v[j - 1][k]);
        if (j <= nr && d) differs[r0 + j] = 1;
    }
    if (W > 1 && blockIdx.x == 0 && nw * W + (int)threadIdx.x < S) {   // the S % 4 samples behind the last whole word
        const long long s = nw * W + threadIdx.x;
        uint32_t prev = wave[(long long)r0 * stride + s];
        for (int j = 1; j <= nr; ++j) {
            const uint32_t cur = wave[(long long)(r0 + j) * stride + s];
            if (cur != prev) differs[r0 + j] = 1;
            prev = cur;
        }
    }
}

__device__ __forceinline__ int rr_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

__global__ __launch_bounds__(RR_THREADS) void rows_repeat_kernel(int* __restrict__ differs, int n_rows,
                                                                 int* __restrict__ repeat_out) {
    __shared__ int part[RR_THREADS];
    int g = n_rows;
    for (int i = 1 + threadIdx.x; i < n_rows; i += RR_THREADS)
        if (differs[i]) {
            g = rr_gcd(g, i);
            differs[i] = 0;
        }
    part[threadIdx.x] = g;
    __syncthreads();
    for (int s = RR_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = rr_gcd(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *repeat_out = part[0];
}

}  // namespace

int dz_launch_rows_repeat(const float* wave, long long stride, int n_rows, int S, int* differs, int* repeat_out,
                          hipStream_t st) {
    DZ_REQUIRE(n_rows >= 2 && S >= 1 && stride >= 0, "rows_repeat: %d rows of %d samples, stride %lld", n_rows, S, stride);
    const bool vec = (((uintptr_t)wave & 15) == 0) && (stride & 3) == 0;
    const int words = vec ? S / 4 : S;
    const int gx = words > 0 ? (words + RR_THREADS * RR_PER - 1) / (RR_THREADS * RR_PER) : 1;
    const int gy = (n_rows - 1 + RR_ROWS - 1) / RR_ROWS;
    DZ_REQUIRE(gy <= 65535, "rows_repeat: %d rows (at most %d)", n_rows, 65535 * RR_ROWS);
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(wave);
    if (vec)
        DZ_LAUNCH(rows_differ_kernel<uint4>, dim3(gx, gy), dim3(RR_THREADS), 0, st, bits, stride, n_rows, S, differs);
    else
        DZ_LAUNCH(rows_differ_kernel<uint32_t>, dim3(gx, gy), dim3(RR_THREADS), 0, st, bits, stride, n_rows, S, differs);
    DZ_HIP(hipGetLastError());
    DZ_LAUNCH(rows_repeat_kernel, dim3(1), dim3(RR_THREADS), 0, st, differs, n_rows, repeat_out);
    DZ_HIP(hipGetLastError());
    return 0;
}
