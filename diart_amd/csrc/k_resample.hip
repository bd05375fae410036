// Band-limited resampling (torchaudio's sinc_interp_hann, DESIGN.md "Resampling"): output m = j n + i is
// sum_k h[i][k] x[j o - width + k], x = 0 outside [0, L).  Every output is ONE fused-multiply-add chain over its T
// taps in ascending k, started from 0, with no tap skipped (zero weights and zero padding included): a row's outputs
// do not depend on the batch, the tile or the launch it comes in, and a NaN / Inf sample reaches exactly the outputs
// whose taps cover it.  Host side: resample_api.hip.
//
// Two launch shapes, chosen by the phase count n (the same chain in both):
//   * n >= 64 (44.1, 22.05, 11.025, 88.2 kHz -> 16 kHz): lanes are phases.  A wave owns RS_J consecutive input
//     blocks j, so the J samples it needs at tap k are wave-uniform (scalar loads), and each lane reads its tap from
//     the tap-major table [k][n_pad] (one coalesced 256-byte row per wave and tap, shared by the workgroup's waves
//     through L1).  One table row feeds RS_J fmas.
//   * n < 64 (48, 32, 24, 12, 8 kHz ...): lanes are input blocks j, each lane runs every phase.  The taps of a phase
//     are wave-uniform (phase-major table [i][T], scalar loads); the workgroup's input span is staged in LDS when it
//     fits, and the lane's sample is read once per tap and feeds up to RS_P fmas.
#include "dz_common.h"

namespace {

constexpr int RS_J = 16;   // input blocks per wave (phase-lane shape)
constexpr int RS_P = 8;    // phases per pass (block-lane shape)
constexpr int RS_K = 8;    // taps per step of the phase-lane shape's interior loop
constexpr int RS_SPAN_MAX = 8192;   // block-lane shape: largest input span staged in LDS (floats)

__device__ __forceinline__ float rs_sample(const float* __restrict__ x, long long idx, long long L) {
    // always a valid address (idx clamped), then the value or 0: no per-lane branch around the load
    const long long c = idx < 0 ? 0 : (idx >= L ? L - 1 : idx);
    const float v = x[c];
    return (idx >= 0 && idx < L) ? v : 0.f;
}

// grid (ceil(nj / (4 RS_J)), n_pad / 64, rows), 256 threads.  htap: [T][n_pad] (rows i >= n are zero).
__global__ __launch_bounds__(256) void resample_phase_lanes(const float* __restrict__ in, long long in_stride,
                                                            long long L, const float* __restrict__ htap, int n,
                                                            int n_pad, int o, int width, int T, long long nj,
                                                            long long out_len, float* __restrict__ out,
                                                            long long out_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long j0 = ((long long)blockIdx.x * 4 + wave) * RS_J;
    if (j0 >= nj) return;
    const int i = blockIdx.y * 64 + lane;
    const float* __restrict__ x = in + (long long)blockIdx.z * in_stride;
    const long long base = j0 * o - width;                       // first input sample of block j0's taps
    const bool interior = base >= 0 && base + (long long)(RS_J - 1) * o + T <= L;
    float acc[RS_J];
#pragma unroll
    for (int q = 0; q < RS_J; ++q) acc[q] = 0.f;
    const float* __restrict__ hp = htap + i;
    if (interior) {
        const float* __restrict__ xb = x + base;
        int k = 0;
        for (; k + RS_K <= T; k += RS_K) {       // RS_K taps at a time: a block's samples come in one scalar load
            float hv[RS_K];
#pragma unroll
            for (int kk = 0; kk < RS_K; ++kk) hv[kk] = hp[(long long)(k + kk) * n_pad];
#pragma unroll
            for (int q = 0; q < RS_J; ++q) {
                const float* __restrict__ xq = xb + (long long)q * o + k;
#pragma unroll
                for (int kk = 0; kk < RS_K; ++kk) acc[q] = fmaf(hv[kk], xq[kk], acc[q]);
            }
        }
        for (; k < T; ++k) {
            const float hv = hp[(long long)k * n_pad];
#pragma unroll
            for (int q = 0; q < RS_J; ++q) acc[q] = fmaf(hv, xb[(long long)q * o + k], acc[q]);
        }
    } else {
        for (int k = 0; k < T; ++k) {
            const float hv = hp[(long long)k * n_pad];
#pragma unroll
            for (int q = 0; q < RS_J; ++q) acc[q] = fmaf(hv, rs_sample(x, base + (long long)q * o + k, L), acc[q]);
        }
    }
    if (i >= n) return;
    float* __restrict__ y = out + (long long)blockIdx.z * out_stride;
#pragma unroll
    for (int q = 0; q < RS_J; ++q) {
        const long long m = (j0 + q) * n + i;
        if (j0 + q < nj && m < out_len) y[m] = acc[q];
    }
}

// grid (ceil(nj / 256), 1, rows), 256 threads.  hph: [n][T] (phase-major).  span > 0: the workgroup's input span
// (255 o + T samples from block jb's first tap, zero outside the row) is staged in LDS first (span floats of dynamic
// LDS); span = 0: every sample is read from global memory.  The same values enter the same chain either way.
__global__ __launch_bounds__(256) void resample_block_lanes(const float* __restrict__ in, long long in_stride,
                                                            long long L, const float* __restrict__ hph, int n, int o,
                                                            int width, int T, long long nj, long long out_len,
                                                            float* __restrict__ out, long long out_stride, int span) {
    extern __shared__ float xs[];
    const long long jb = (long long)blockIdx.x * 256;
    const long long j = jb + threadIdx.x;
    const float* __restrict__ x = in + (long long)blockIdx.z * in_stride;
    if (span > 0) {
        const long long s0 = jb * o - width;
        for (int t = threadIdx.x; t < span; t += 256) xs[t] = rs_sample(x, s0 + t, L);
        __syncthreads();
    }
    if (j >= nj) return;
    float* __restrict__ y = out + (long long)blockIdx.z * out_stride;
    const long long base = j * o - width;
    const float* xl = xs + threadIdx.x * o;                       // this lane's taps in the staged span
    for (int i0 = 0; i0 < n; i0 += RS_P) {
        const int np = min(RS_P, n - i0);                         // uniform
        float acc[RS_P];
#pragma unroll
        for (int p = 0; p < RS_P; ++p) acc[p] = 0.f;
        const float* __restrict__ h = hph + (long long)i0 * T;
        if (span > 0) {
            for (int k = 0; k < T; ++k) {
                const float xv = xl[k];
#pragma unroll
                for (int p = 0; p < RS_P; ++p)
                    if (p < np) acc[p] = fmaf(h[p * T + k], xv, acc[p]);
            }
        } else {
            for (int k = 0; k < T; ++k) {
                const float xv = rs_sample(x, base + k, L);
#pragma unroll
                for (int p = 0; p < RS_P; ++p)
                    if (p < np) acc[p] = fmaf(h[(long long)p * T + k], xv, acc[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < RS_P; ++p) {
            const long long m = j * n + i0 + p;
            if (p < np && m < out_len) y[m] = acc[p];
        }
    }
}

}  // namespace

int dz_launch_resample(const float* in, long long in_stride, long long in_len, int rows, const float* table,
                       int tap_major, int n, int n_pad, int o, int width, int T, float* out, long long out_stride,
                       long long out_len, hipStream_t st) {
    const long long nj = (out_len + n - 1) / n;                   // input blocks with at least one output
    if (tap_major) {
        const long long gx = (nj + 4 * RS_J - 1) / (4 * RS_J);
        DZ_REQUIRE(gx <= 0x7fffffffLL && rows <= 65535, "resample: grid (%lld, %d) too large", gx, rows);
        DZ_LAUNCH(resample_phase_lanes, dim3((unsigned)gx, n_pad / 64, rows), dim3(256), 0, st, in, in_stride,
                  in_len, table, n, n_pad, o, width, T, nj, out_len, out, out_stride);
    } else {
        const long long gx = (nj + 255) / 256;
        DZ_REQUIRE(gx <= 0x7fffffffLL && rows <= 65535, "resample: grid (%lld, %d) too large", gx, rows);
        const long long span = 255ll * o + T;                     // staged when it fits in 32 KiB of LDS
        const int staged = span <= RS_SPAN_MAX ? (int)span : 0;
        DZ_LAUNCH(resample_block_lanes, dim3((unsigned)gx, 1, rows), dim3(256), staged * sizeof(float), st, in,
                  in_stride, in_len, table, n, o, width, T, nj, out_len, out, out_stride, staged);
    }
    DZ_HIP(hipGetLastError());
    return 0;
}
