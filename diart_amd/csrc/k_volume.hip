// dz_adjust_volume: the reference's AdjustVolume block (blocks/utils.py:92-137; DESIGN.md "Volume adjustment") for rows
// of interleaved float32 samples.  Independently for every (row, channel) signal x of n samples:
//     volume = 10 log10(mean(fl32(x x)))            squares in f32 (they underflow where the reference's do), summed in f64
//     gain   = fl32(10 ^ ((target_db - volume) / 20))   computed once, in f64
//     m      = max(fl32(gain max|x|), 1), NaN when that product is NaN   (rounding is monotone: the largest of the
//                                                                         rounded products is the rounded largest product)
//     out    = fl32(fl32(gain x) / m)
// The special rows follow from the arithmetic alone: zero energy -> gain = inf -> inf 0 = NaN; an Inf sample -> gain = 0
// -> 0 inf = NaN; a NaN sample -> NaN sum and NaN peak.  max|x| is taken on the bit patterns of |x| as unsigned
// integers: for non-negative floats that is the float order, with every NaN above +Inf, so a NaN is never dropped
// (fmaxf / v_max_f32 would drop it) and the order of the comparisons does not show.
//
// One workgroup per signal, two passes: the reduction, then the scale (the second pass reads what the first left in
// L2).  The work is dealt by SAMPLE INDEX, never by address: thread t owns the sample quads t, t + 1024, ... (and thread
// t < n % 4 the tail sample 4 (n / 4) + t after them), sums its squares in that order, and the partial sums meet in a
// fixed order (lanes by shuffle, waves through LDS).  So a signal's bits do not depend on its row's alignment, stride,
// place in the batch or the other rows of the call, and two calls agree.  No atomics, no scratch.
//
// Mono rows move one quad per lane as a 16-byte load / store.  A row may start at any float address (a 110 250-sample
// row at 44.1 kHz puts every other row 8 bytes off): global_load_dwordx4 / global_store_dwordx4 need dword alignment
// only, so the same instructions serve every base and there is no scalar head, only the tail above.  Interleaved rows
// (channels > 1) are read and written one float at a time, channels apart: in place, a workgroup touches nothing of
// its row's other channels.
#include "dz_common.h"

#include <math.h>

namespace {

constexpr int VOL_THREADS = 1024;   // 16 waves: 64 windows are 64 workgroups, each has to keep a CU's memory pipe busy alone
constexpr int VOL_UNROLL = 4;       // quads in flight per lane in the reduction

typedef float vol_quad __attribute__((ext_vector_type(4), aligned(4)));   // four samples at any float address

__device__ __forceinline__ unsigned vol_abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__device__ __forceinline__ void vol_take(float v, double& sum, unsigned& peak) {
    const float sq = v * v;             // fl32, as the reference squares
    sum += (double)sq;
    const unsigned a = vol_abs_bits(v);
    peak = a > peak ? a : peak;
}

// grid (rows * channels), VOL_THREADS threads
template <bool MONO>
__global__ __launch_bounds__(VOL_THREADS) void adjust_volume_kernel(const float* in, long long in_stride, float* out,
                                                                    long long out_stride,
                                                                    long long n, int channels, double target_db) {
    __shared__ double wsum[VOL_THREADS / 64];
    __shared__ unsigned wpeak[VOL_THREADS / 64];
    __shared__ float gm[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = MONO ? blockIdx.x : blockIdx.x / channels;
    const int ch = MONO ? 0 : blockIdx.x - row * channels;
    const float* x = in + (long long)row * in_stride + ch;
    float* y = out + (long long)row * out_stride + ch;
    const long long nq = MONO ? n >> 2 : 0;          // whole quads (mono); everything else one sample at a time
    const vol_quad* xq = reinterpret_cast<const vol_quad*>(x);

    // ---- pass 1: sum of squares and largest |x|, this thread's samples in ascending order
    double sum = 0.0;
    unsigned peak = 0u;
    if (MONO) {
        long long q = tid;
        for (; q + (VOL_UNROLL - 1) * VOL_THREADS < nq; q += VOL_UNROLL * VOL_THREADS) {
            vol_quad v[VOL_UNROLL];
#pragma unroll
            for (int u = 0; u < VOL_UNROLL; ++u) v[u] = xq[q + u * VOL_THREADS];
#pragma unroll
            for (int u = 0; u < VOL_UNROLL; ++u) {
                vol_take(v[u].x, sum, peak);
                vol_take(v[u].y, sum, peak);
                vol_take(v[u].z, sum, peak);
                vol_take(v[u].w, sum, peak);
            }
        }
        for (; q < nq; q += VOL_THREADS) {
            const vol_quad v = xq[q];
            vol_take(v.x, sum, peak);
            vol_take(v.y, sum, peak);
            vol_take(v.z, sum, peak);
            vol_take(v.w, sum, peak);
        }
        if (4 * nq + tid < n) vol_take(x[4 * nq + tid], sum, peak);
    } else {
        for (long long s = tid; s < n; s += VOL_THREADS) vol_take(x[s * channels], sum, peak);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {               // lanes: a fixed tree
        sum += __shfl_down(sum, d, 64);
        const unsigned o = __shfl_down(peak, d, 64);
        peak = o > peak ? o : peak;
    }
    if (lane == 0) {
        wsum[wave] = sum;
        wpeak[wave] = peak;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        unsigned pk = 0u;
        for (int w = 0; w < VOL_THREADS / 64; ++w) {  // waves: in order
            total += wsum[w];
            pk = wpeak[w] > pk ? wpeak[w] : pk;
        }
        const double volume = 10.0 * log10(total / (double)n);
        const float gain = (float)pow(10.0, (target_db - volume) / 20.0);
        const float top = gain * __uint_as_float(pk);             // fl32(gain max|x|); NaN for the special rows
        gm[0] = gain;
        gm[1] = (top > 1.f || top != top) ? top : 1.f;           // clamp(min=1) keeps a NaN
    }
    __syncthreads();
    const float gain = gm[0], m = gm[1];

    // ---- pass 2: fl32(fl32(gain x) / m); a thread rewrites only what it read (in place is safe)
    if (MONO) {
        vol_quad* yq = reinterpret_cast<vol_quad*>(y);
        for (long long q = tid; q < nq; q += VOL_THREADS) {
            const vol_quad v = xq[q];
            vol_quad r;
            r.x = (gain * v.x) / m;
            r.y = (gain * v.y) / m;
            r.z = (gain * v.z) / m;
            r.w = (gain * v.w) / m;
            yq[q] = r;
        }
        if (4 * nq + tid < n) y[4 * nq + tid] = (gain * x[4 * nq + tid]) / m;
    } else {
        for (long long s = tid; s < n; s += VOL_THREADS) y[s * channels] = (gain * x[s * channels]) / m;
    }
}

}  // namespace

extern "C" int dz_adjust_volume(dz_ctx* ctx, const float* d_in, long long in_row_stride, float* d_out,
                                long long out_row_stride, int rows, long long samples, int channels, double target_db,
                                void* stream) {
    DZ_REQUIRE(ctx && d_in && d_out, "dz_adjust_volume: NULL argument");
    DZ_REQUIRE((((uintptr_t)d_in | (uintptr_t)d_out) & 3) == 0, "dz_adjust_volume: %p / %p is not a float address",
               (const void*)d_in, (const void*)d_out);
    DZ_REQUIRE(rows >= 1 && samples >= 1 && samples <= (1ll << 40), "dz_adjust_volume: %d rows of %lld samples", rows,
               samples);
    DZ_REQUIRE(channels >= 1 && channels <= 8, "dz_adjust_volume: %d channels outside [1, 8]", channels);
    DZ_REQUIRE((long long)rows * channels <= 0x7fffffffLL, "dz_adjust_volume: %d rows x %d channels exceed the grid", rows,
               channels);
    const long long row = samples * channels;
    DZ_REQUIRE(in_row_stride >= row && out_row_stride >= row,
               "dz_adjust_volume: row strides %lld in / %lld out for rows of %lld x %d values", in_row_stride,
               out_row_stride, samples, channels);
    DZ_REQUIRE(isfinite(target_db), "dz_adjust_volume: target_db %g is not finite", target_db);
    // in place means the same rows: a thread rewrites what it read.  (Any other overlap of the two buffers is not checked.)
    DZ_REQUIRE(d_in != d_out || in_row_stride == out_row_stride,
               "dz_adjust_volume: in place needs equal strides (%lld in, %lld out)", in_row_stride, out_row_stride);
    DZ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)rows * (unsigned)channels;
    if (channels == 1)
        DZ_LAUNCH(adjust_volume_kernel<true>, dim3(grid), dim3(VOL_THREADS), 0, st, d_in, in_row_stride, d_out,
                  out_row_stride, samples, 1, target_db);
    else
        DZ_LAUNCH(adjust_volume_kernel<false>, dim3(grid), dim3(VOL_THREADS), 0, st, d_in, in_row_stride, d_out,
                  out_row_stride, samples, channels, target_db);
    DZ_HIP(hipGetLastError());
    return 0;
}
