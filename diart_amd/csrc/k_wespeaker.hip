// WeSpeaker ResNet34 (pyannote/wespeaker-voxceleb-resnet34-LM): everything but the 2-D convolutions of the trunk
// (k_conv2d.hip) — the kaldi fbank, its per-row mean normalisation, the 1-channel first convolution and the TSTP
// statistics pooling.  Host side: wespeaker_api.hip; definition: DESIGN.md "WeSpeaker ResNet34".
#include "dz_common.h"

namespace {

constexpr int WIN = 400, HOP = 160, NFFT = 512, NBIN = 257, NMEL = 80;
constexpr float EPS_F32 = 1.1920928955078125e-07f;       // torch.finfo(float32).eps: kaldi's log floor
// The waveform is scaled by 2^15 before the fbank; the power spectrum is then 2^30 times that of the unscaled
// frame.  log(max(eps, 2^30 E)) = 30 ln 2 + log(max(eps 2^-30, E)) exactly (a power of two), so the kernel keeps the
// unscaled samples and adds the constant.
constexpr float LOG_SCALE = 20.794415416798359f;          // 30 ln 2
constexpr float EPS_UNSCALED = EPS_F32 / 1073741824.f;

// Deterministic tree sum over 256 threads (red: 256 floats of LDS); every thread gets the total.
__device__ __forceinline__ float block_sum256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// One frame per workgroup: DC removal, pre-emphasis 0.97 (first sample replicated), symmetric Hamming window,
// 512-point power spectrum as a direct f32 DFT (bins k = thread, Nyquist by thread 0), kaldi mel bank, log floor.
__global__ __launch_bounds__(256) void wsp_fbank_kernel(const float* __restrict__ wave, long long stride, int T,
                                                        const float* __restrict__ mel, float* __restrict__ raw,
                                                        int* __restrict__ bad) {
    __shared__ float xs[WIN], ys[WIN], cs[NFFT], sn[NFFT], pw[NBIN], red[256];
    __shared__ int nbad;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* x = wave + (long long)b * stride + (long long)t * HOP;
    if (tid == 0) nbad = 0;
    for (int j = tid; j < NFFT; j += 256) {
        float s, c;
        sincospif((float)j / (NFFT / 2), &s, &c);      // e^{-2 pi i j / 512} = c - i s
        cs[j] = c;
        sn[j] = s;
    }
    __syncthreads();
    float part = 0.f;
    int lbad = 0;
    for (int n = tid; n < WIN; n += 256) {
        const float v = x[n];
        xs[n] = v;
        part += v;
        lbad |= !isfinite(v);
    }
    if (lbad) nbad = 1;
    const float mean = block_sum256(part, red) / (float)WIN;   // (the barrier also publishes xs and nbad)
    if (nbad) {          // a NaN / Inf sample: the row is flagged, its features are zeroed by the CMN pass
        if (tid == 0) bad[b] = 1;
        return;
    }
    for (int n = tid; n < WIN; n += 256) {
        const float cur = xs[n] - mean, prev = xs[n > 0 ? n - 1 : 0] - mean;
        const float win = 0.54f - 0.46f * cospif(2.f * (float)n / (float)(WIN - 1));
        ys[n] = (cur - 0.97f * prev) * win;
    }
    __syncthreads();
    {
        const int k = tid;
        float re = 0.f, im = 0.f;
        for (int n = 0; n < WIN; ++n) {
            const int j = (k * n) & (NFFT - 1);
            re = fmaf(ys[n], cs[j], re);
            im = fmaf(ys[n], sn[j], im);
        }
        pw[k] = re * re + im * im;
        if (tid == 0) {
            float ny = 0.f;
            for (int n = 0; n < WIN; ++n) ny += (n & 1) ? -ys[n] : ys[n];
            pw[NFFT / 2] = ny * ny;
        }
    }
    __syncthreads();
    if (tid < NMEL) {
        const float* mr = mel + tid * NBIN;
        float e = 0.f;
        for (int j = 0; j < NBIN; ++j) e = fmaf(pw[j], mr[j], e);
        raw[((long long)b * NMEL + tid) * T + t] = logf(fmaxf(e, EPS_UNSCALED)) + LOG_SCALE;
    }
}

// grid (80, N): mean over the T frames of one (row, bin), subtracted
__global__ __launch_bounds__(256) void wsp_cmn_kernel(const float* __restrict__ raw, int T, const int* __restrict__ bad,
                                                      float* __restrict__ feats) {
    __shared__ float red[256];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long long base = ((long long)b * NMEL + f) * T;
    if (bad[b]) {        // (block-uniform)
        for (int t = tid; t < T; t += 256) feats[base + t] = 0.f;
        return;
    }
    float part = 0.f;
    for (int t = tid; t < T; t += 256) part += raw[base + t];
    const float mean = block_sum256(part, red) / (float)T;
    for (int t = tid; t < T; t += 256) feats[base + t] = raw[base + t] - mean;
}

// one thread per (position, output channel): 9 taps in (kh, kw) order, zero padding 1
__global__ __launch_bounds__(256) void wsp_conv1_kernel(const float* __restrict__ feats, int T, long long total,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx & 31);
    const long long pos = idx >> 5;
    const int t = (int)(pos % T);
    const long long bf = pos / T;
    const int f = (int)(bf % NMEL);
    const float* xb = feats + (bf - f) * T;          // row b's [80][T]
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int fi = f + kh - 1;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ti = t + kw - 1;
            const float v = (fi >= 0 && fi < NMEL && ti >= 0 && ti < T) ? xb[(long long)fi * T + ti] : 0.f;
            acc = fmaf(v, w[c * 9 + kh * 3 + kw], acc);
        }
    }
    y[idx] = fmaxf(acc + bias[c], 0.f);
}

// grid (10, B K), thread = channel c: the statistics of pooled dimension c 10 + f of pool row r (trunk row r / K).
// Weights (pyannote.audio 3.1 StatsPool._pool): v1 = sum w + 1e-8, mean = sum w x / v1,
// var = sum w (x - mean)^2 / (v1 - sum w^2 / v1 + 1e-8); without weights mean and unbiased std.
__global__ __launch_bounds__(256) void wsp_pool_kernel(const float* __restrict__ x, int T4,
                                                       const float* __restrict__ weights, int Fw, int K,
                                                       const int* __restrict__ bad, float* __restrict__ out,
                                                       int* __restrict__ rflag) {
    extern __shared__ float ws[];
    const int f = blockIdx.x, r = blockIdx.y, c = threadIdx.x, b = r / K;
    const float* xr = x + ((long long)(b * 10 + f) * T4) * 256 + c;
    float mean, var;
    if (weights) {
        const float* wr = weights + (long long)r * Fw;
        for (int t = c; t < T4; t += 256) ws[t] = dz_pool_weight(wr, -Fw, T4, t);     // F.interpolate(mode="nearest")
        __syncthreads();
        float sw = 0.f, sw2 = 0.f, s = 0.f;
        for (int t = 0; t < T4; ++t) {
            const float wt = ws[t];
            sw += wt;
            sw2 += wt * wt;
            s += wt * xr[(long long)t * 256];
        }
        const float v1 = sw + 1e-8f;
        mean = s / v1;
        float d = 0.f;
        for (int t = 0; t < T4; ++t) {
            const float e = xr[(long long)t * 256] - mean;
            d += ws[t] * (e * e);
        }
        var = d / (v1 - sw2 / v1 + 1e-8f);
    } else {
        float s = 0.f;
        for (int t = 0; t < T4; ++t) s += xr[(long long)t * 256];
        mean = s / (float)T4;
        float d = 0.f;
        for (int t = 0; t < T4; ++t) {
            const float e = xr[(long long)t * 256] - mean;
            d += e * e;
        }
        var = d / (float)(T4 - 1);
    }
    float* o = out + (long long)r * 5120 + c * 10 + f;
    o[0] = mean;
    o[2560] = sqrtf(var);
    if (f == 0 && c == 0) rflag[r] = bad[b];
}

}  // namespace

int dz_launch_wsp_fbank(const float* wave, long long stride, int N, int T, const float* mel, float* raw, int* bad,
                        hipStream_t st) {
    DZ_REQUIRE(wave && mel && raw && bad && N >= 1 && T >= 1, "wsp_fbank: bad arguments");
    DZ_LAUNCH(wsp_fbank_kernel, dim3(T, N), dim3(256), 0, st, wave, stride, T, mel, raw, bad);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_wsp_cmn(const float* raw, int N, int T, const int* bad, float* feats, hipStream_t st) {
    DZ_LAUNCH(wsp_cmn_kernel, dim3(NMEL, N), dim3(256), 0, st, raw, T, bad, feats);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_wsp_conv1(const float* feats, int N, int T, const float* w, const float* b, float* y, hipStream_t st) {
    const long long total = (long long)N * NMEL * T * 32;
    DZ_LAUNCH(wsp_conv1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, feats, T, total, w, b, y);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_wsp_pool(const float* x, int B, int T4, const float* weights, int Fw, int K, const int* bad,
                       float* out, int* rflag, hipStream_t st) {
    DZ_REQUIRE(T4 >= 1 && T4 <= 8192, "wsp_pool: %d frames", T4);
    DZ_REQUIRE(weights == nullptr || Fw >= 1, "wsp_pool: %d weight frames", Fw);
    const size_t lds = weights ? sizeof(float) * T4 : 0;
    DZ_LAUNCH(wsp_pool_kernel, dim3(10, B * K), dim3(256), lds, st, x, T4, weights, Fw, K, bad, out, rflag);
    DZ_HIP(hipGetLastError());
    return 0;
}
