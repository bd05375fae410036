// Kernels around the NeMo TitaNet-L embedding (include/diart_amd.h: dz_ttn_*): everything that is not
// a GEMM.  The pointwise convolutions, the DFT, the mel bank and the pooling's attention run on the wide GEMMs
// (k_gemm_pre.hip / k_gemm_f32.hip / k_gemm_split.hip / k_convgemm.hip), the pooling itself and the power spectrum
// (power_kernel<257>) on k_ecapa.hip.
//   ttn_geometry   per-group geometry on the device: NaN flags, each row's valid frames and padded length
//   ttn_prep       pre-emphasis, masked at the row's length, + the centred STFT's padding (reflect | zeros)
//   ttn_norm       log(mel + 2^-24) -> per-feature mean / unbiased std over the row's valid frames, zeros past them
//   ttn_depthwise  masked depthwise convolution, written as the next pointwise GEMM's operand
//   ttn_se_fc      squeeze-excitation: Linear(C, C / 8) -> ReLU -> Linear(C / 8, C) -> sigmoid
//   ttn_apply      gate * y (+ residual) -> ReLU, written as f32 rows and as the residual GEMM's operand planes
// No reduction here depends on the row count or on a row's place in the batch: a row's sums run over its own
// frames in a fixed order.
#include "dz_common.h"

namespace {

constexpr int HOP = 160, LEAD = 200;     // samples per frame step; the compacted rows start LEAD samples into sig
constexpr float PREEMPH = 0.97f;

// ---------------------------------------------------------------------------
// ttn_geometry: one thread per group of K rows (the wrapper's rules).  lens[r]: kept samples,
// -(len + 1) for a row with a NaN / Inf sample.  A row shorter than min_samples is computed at the group's longest
// length and flagged; a group whose longest row is too short is flagged as a whole (and computed at full length:
// finite, read by no output).  frames = (len + 2 fpad - fnfft) / HOP + 1, clamped to [1, Tc].
// ---------------------------------------------------------------------------
__global__ void ttn_geometry_kernel(const int* __restrict__ lens, int G, int K, int Tc, int S, int min_samples, int fpad,
                                    int fnfft, int* __restrict__ tooshort, int* __restrict__ elen, int* __restrict__ plen,
                                    int* __restrict__ frames) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int r0 = g * K;
    int lmax = 0;
    for (int k = 0; k < K; ++k) {
        const int l = lens[r0 + k];
        lmax = max(lmax, l < 0 ? -l - 1 : l);
    }
    const bool all_short = lmax < min_samples;
    for (int k = 0; k < K; ++k) {
        const int r = r0 + k, l0 = lens[r];
        const bool bad = l0 < 0;
        int len = bad ? -l0 - 1 : l0;
        const bool too_short = len < min_samples;
        tooshort[r] = all_short || too_short || bad;
        if (too_short) len = all_short ? S : lmax;
        int f = (len + 2 * fpad - fnfft) / HOP + 1;
        f = f < 1 ? 1 : (f > Tc ? Tc : f);
        elen[r] = len;
        plen[r] = all_short ? S : lmax;
        frames[r] = f;
    }
}

// sig [row][LEAD + i] = sample i of the compacted row (zeros elsewhere) -> out [row][LEAD + i] = sample i of the
// pre-emphasised signal y(j) = x(j) - 0.97 x(j - 1), y(0) = x(0), y = 0 at and past the row's length, padded at
// i < 0 and i >= plen (the length the batch pads the row to) by reflection, or by zeros.
__global__ __launch_bounds__(256) void ttn_prep_kernel(const float* __restrict__ sig, long long stride,
                                                      const int* __restrict__ elen, const int* __restrict__ plen,
                                                      int reflect, float* __restrict__ out) {
    const int row = blockIdx.y;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= stride) return;
    const float* x = sig + (long long)row * stride + LEAD;
    const int len = elen[row], L = plen[row];
    int j = (int)p - LEAD;
    if (j < 0) j = reflect ? -j : -1;
    else if (j >= L) j = reflect ? 2 * (L - 1) - j : -1;
    float v = 0.f;
    if (j >= 0 && j < len) v = j > 0 ? x[j] - PREEMPH * x[j - 1] : x[0];
    out[(long long)row * stride + p] = v;
}

// mel power [row][T][80] -> features [row][T][80]: log(x + 2^-24), minus the feature's mean over the row's n valid
// frames, over (unbiased std + 1e-5); zeros at and past frame n.  The sums are float64 over the frames part, part + 3,
// ... of three thread groups, combined in the order 0, 1, 2 (exact for a constant feature: digital silence
// normalises to exactly 0, as it does in float64).
__global__ __launch_bounds__(256) void ttn_norm_kernel(const float* __restrict__ melp, int T,
                                                      const int* __restrict__ frames, float* __restrict__ feats) {
    __shared__ double part[3][80];
    __shared__ double mean_s[80], rstd_s[80];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* x = melp + (long long)row * T * 80;
    float* y = feats + (long long)row * T * 80;
    const int n = frames[row];
    const float guard = 5.9604644775390625e-08f;        // 2^-24
    const int m = tid % 80, pt = tid / 80;
    if (tid < 240) {
        double s = 0.0;
        for (int t = pt; t < n; t += 3) s += (double)logf(x[t * 80 + m] + guard);
        part[pt][m] = s;
    }
    __syncthreads();
    if (tid < 80) mean_s[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) / (double)n;
    __syncthreads();
    if (tid < 240) {
        const double mean = mean_s[m];
        double s = 0.0;
        for (int t = pt; t < n; t += 3) {
            const double d = (double)logf(x[t * 80 + m] + guard) - mean;
            s += d * d;
        }
        part[pt][m] = s;
    }
    __syncthreads();
    if (tid < 80)        // (n = 1: 0 / 0 = NaN, as torch.std)
        rstd_s[tid] = 1.0 / (sqrt(((part[0][tid] + part[1][tid]) + part[2][tid]) / (double)(n - 1)) + 1e-5);
    __syncthreads();
    for (int i = tid; i < T * 80; i += 256) {
        const int t = i / 80, c = i - t * 80;
        y[i] = t < n ? (float)(((double)logf(x[i] + guard) - mean_s[c]) * rstd_s[c]) : 0.f;
    }
}

// ---------------------------------------------------------------------------
// ttn_depthwise: y[row][t][c] = sum_j w[j][c] u[row][t + j - KT / 2][c], u = x (ReLU'd when relu) for frames in
// [0, frames[row]) and 0 outside — the length mask is applied on load.  Memory-bound: a workgroup stages the 32 +
// KT - 1 input frames x 128 channels it needs in LDS with coalesced 16-byte loads; wave w then owns the 32-channel
// strip 32 w .. 32 w + 31 (one k-block of the consumer's planes): lane = 8 * frame + channel quad, four passes of 8
// frames, the taps of the lane's four channels in registers.  A pass writes 8 rows x 128 bytes of f32 (the exact-f32
// GEMM's operand), or (PLANES) 512 contiguous bytes of each kb-major f16 plane (k_gemm_pre.hip's operand; dz_kb) —
// no f32 tensor in between.  LDS rows are 160 floats apart: the two frames of a 16-lane group sit in opposite halves
// of the banks.
// ---------------------------------------------------------------------------
typedef _Float16 ttn_f16x4 __attribute__((ext_vector_type(4)));
constexpr int DW_TF = 32, DW_LD = 160;

__device__ __forceinline__ void ttn_store_planes(unsigned short* planes, long long plane, long long idx, const f32x4& o,
                                                 float& amax) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        amax = fmaxf(amax, fabsf(o[e]));
        v[e] = __builtin_amdgcn_fmed3f(o[e], -65504.f, 65504.f);
    }
    const ttn_f16x4 hi = __builtin_convertvector(v, ttn_f16x4);
    const ttn_f16x4 lo = __builtin_convertvector((v - __builtin_convertvector(hi, f32x4)) * 2048.f, ttn_f16x4);
    *reinterpret_cast<ttn_f16x4*>(planes + idx) = hi;
    *reinterpret_cast<ttn_f16x4*>(planes + plane + idx) = lo;
}

template <int KT, bool PLANES>
__global__ __launch_bounds__(256) void ttn_depthwise_kernel(const float* __restrict__ x, int ldx, int Cin,
                                                           const float* __restrict__ taps,
                                                           const int* __restrict__ frames, int T, int C, int relu,
                                                           float* __restrict__ y, unsigned short* __restrict__ planes,
                                                           long long plane, long long R, int* __restrict__ oflag) {
    constexpr int HALO = KT / 2, ROWS = DW_TF + KT - 1;
    __shared__ __attribute__((aligned(16))) float tile[ROWS * DW_LD];
    const int tid = threadIdx.x, row = blockIdx.z, t0 = blockIdx.y * DW_TF, c0 = blockIdx.x * 128;
    const int n = frames[row];
    const float* xr = x + (long long)row * T * ldx;
    for (int i = tid; i < ROWS * 32; i += 256) {
        const int r = i >> 5, q = i & 31, t = t0 - HALO + r, c = c0 + q * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < n && c < Cin) {
            v = *reinterpret_cast<const f32x4*>(xr + (long long)t * ldx + c);
            if (relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
        }
        *reinterpret_cast<f32x4*>(tile + r * DW_LD + q * 4) = v;
    }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63, quad = lane & 7, fr = lane >> 3;
    const int cl = 32 * w + 4 * quad, c = c0 + cl;
    if (c >= C) return;
    f32x4 wt[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) wt[j] = *reinterpret_cast<const f32x4*>(taps + (long long)j * C + c);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < DW_TF / 8; ++i) {
        const int tl = 8 * i + fr, t = t0 + tl;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(tile + (tl + j) * DW_LD + cl);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wt[j][e], u[e], acc[e]);
        }
        if (t < T) {
            const long long rt = (long long)row * T + t;
            if (PLANES) ttn_store_planes(planes, plane, dz_kb(rt, c, R), acc, amax);
            else *reinterpret_cast<f32x4*>(y + rt * C + c) = acc;
        }
    }
    if (PLANES) dz_flag_range(oflag, amax);
}

// ---------------------------------------------------------------------------
// ttn_se_fc: gate[row][c] = sigmoid(sum_j w2t[j][c] relu(sum_c' w1[j][c'] s[row][c'])), H = C / 8 hidden units.  A
// workgroup takes two rows (the weights are read once for both).  Hidden unit j: the 64 lanes of a wave stride over
// the channels (float4), then a butterfly; output channel c: one thread walks the H hidden units in order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ttn_se_fc_kernel(const float* __restrict__ s, const float* __restrict__ w1,
                                                       const float* __restrict__ w2t, int N, int C, int H,
                                                       float* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* m0 = sm;                // [2][C] squeezed means
    float* h0 = sm + 2 * C;        // [2][H] hidden
    const int tid = threadIdx.x, r0 = blockIdx.x * 2;
    const bool two = r0 + 1 < N;
    for (int i = tid; i < C; i += 256) {
        m0[i] = s[(long long)r0 * C + i];
        m0[C + i] = two ? s[(long long)(r0 + 1) * C + i] : 0.f;
    }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63;
    for (int j = w; j < H; j += 4) {
        float a0 = 0.f, a1 = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w1 + (long long)j * C + c);
            const f32x4 u0 = *reinterpret_cast<const f32x4*>(m0 + c), u1 = *reinterpret_cast<const f32x4*>(m0 + C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0 = fmaf(wv[e], u0[e], a0);
                a1 = fmaf(wv[e], u1[e], a1);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o, 64);
            a1 += __shfl_xor(a1, o, 64);
        }
        if (lane == 0) {
            h0[j] = fmaxf(a0, 0.f);
            h0[H + j] = fmaxf(a1, 0.f);
        }
    }
    __syncthreads();
    for (int c = tid * 4; c < C; c += 1024) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < H; ++j) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w2t + (long long)j * C + c);
            const float g0 = h0[j], g1 = h0[H + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[e] = fmaf(wv[e], g0, a0[e]);
                a1[e] = fmaf(wv[e], g1, a1[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a0[e] = 1.f / (1.f + expf(-a0[e]));
            a1[e] = 1.f / (1.f + expf(-a1[e]));
        }
        *reinterpret_cast<f32x4*>(gate + (long long)r0 * C + c) = a0;
        if (two) *reinterpret_cast<f32x4*>(gate + (long long)(r0 + 1) * C + c) = a1;
    }
}

// out = relu(gate[row][c] * y (+ resid)) over [R = rows T][C]: f32 rows (the next block's depthwise input) and, when
// `planes` is set, the kb-major f16 planes the next block's residual GEMM reads.  Lane order of
// se_apply_planes_kernel (k_ecapa.hip): a wave owns 8 rows x 32 columns.
template <bool RES>
__global__ __launch_bounds__(256) void ttn_apply_kernel(const float* __restrict__ y, const float* __restrict__ gate,
                                                       const float* __restrict__ resid, float* __restrict__ out,
                                                       unsigned short* __restrict__ planes, long long plane,
                                                       long long R, int T, int C, int* __restrict__ oflag) {
    const int tid = threadIdx.x;
    const int c = blockIdx.x * 128 + (tid >> 6) * 32 + (tid & 7) * 4;
    const long long rt = (long long)blockIdx.y * 8 + ((tid >> 3) & 7);
    if (rt >= R || c >= C) return;
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + rt * C + c);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gate + (rt / T) * C + c);
    f32x4 o;
    if (RES) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(resid + rt * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(fmaf(g[e], v[e], r[e]), 0.f);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(g[e] * v[e], 0.f);
    }
    *reinterpret_cast<f32x4*>(out + rt * C + c) = o;
    if (planes) {
        float amax = 0.f;
        ttn_store_planes(planes, plane, dz_kb(rt, c, R), o, amax);
        dz_flag_range(oflag, amax);
    }
}

}  // namespace

int dz_launch_ttn_geometry(const int* lens, int G, int K, int Tc, int S, int min_samples, int fpad, int fnfft,
                           int* tooshort, int* elen, int* plen, int* frames, hipStream_t st) {
    DZ_REQUIRE(G >= 1 && K >= 1 && Tc >= 1 && min_samples > LEAD, "ttn_geometry: G %d, K %d, Tc %d, min_samples %d", G,
               K, Tc, min_samples);
    DZ_LAUNCH(ttn_geometry_kernel, dim3((G + 63) / 64), dim3(64), 0, st, lens, G, K, Tc, S, min_samples, fpad, fnfft,
              tooshort, elen, plen, frames);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_ttn_prep(const float* sig, long long stride, int rows, const int* elen, const int* plen, int reflect,
                       float* out, hipStream_t st) {
    DZ_LAUNCH(ttn_prep_kernel, dim3((unsigned)((stride + 255) / 256), rows), dim3(256), 0, st, sig, stride, elen, plen,
              reflect, out);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_ttn_norm(const float* melp, int T, int rows, const int* frames, float* feats, hipStream_t st) {
    DZ_LAUNCH(ttn_norm_kernel, dim3(rows), dim3(256), 0, st, melp, T, frames, feats);
    DZ_HIP(hipGetLastError());
    return 0;
}

// x [rows][T][ldx] (Cin channels read, the rest of the C output channels see zeros), taps [KT][C] -> y [rows T][C]
// f32, or (planes set) kb-major planes of rows T rows x C columns, lo plane `plane` elements after hi
int dz_launch_ttn_depthwise(const float* x, int ldx, int Cin, const float* taps, int ktaps, const int* frames, int rows,
                            int T, int C, int relu, float* y, void* planes, long long plane, hipStream_t st) {
    DZ_REQUIRE(x && taps && frames && (y || planes), "ttn_depthwise: NULL argument");
    DZ_REQUIRE(rows >= 1 && T >= 1 && C % 32 == 0 && Cin % 4 == 0 && Cin <= C && ldx % 4 == 0 && ldx >= Cin &&
                   ((uintptr_t)x & 15) == 0 && ((uintptr_t)taps & 15) == 0,
               "ttn_depthwise: rows %d, T %d, C %d (multiple of 32), Cin %d, ldx %d (multiples of 4)", rows, T, C, Cin,
               ldx);
    DZ_REQUIRE(planes == nullptr || (plane >= (long long)rows * T * C && plane % 4 == 0), "ttn_depthwise: plane distance");
    DZ_REQUIRE(((uintptr_t)y & 15) == 0 && ((uintptr_t)planes & 15) == 0, "ttn_depthwise: outputs must be 16-byte aligned");
    const dim3 grid((C + 127) / 128, (T + DW_TF - 1) / DW_TF, rows);
    const long long R = (long long)rows * T;
    unsigned short* pl = reinterpret_cast<unsigned short*>(planes);
#define DZ_DW(KT)                                                                                                     \
    case KT:                                                                                                          \
        if (planes)                                                                                                   \
            DZ_LAUNCH((ttn_depthwise_kernel<KT, true>), grid, dim3(256), 0, st, x, ldx, Cin, taps, frames, T, C, relu, y, \
                      pl, plane, R, dz_cur_oflag);                                                                    \
        else                                                                                                          \
            DZ_LAUNCH((ttn_depthwise_kernel<KT, false>), grid, dim3(256), 0, st, x, ldx, Cin, taps, frames, T, C, relu, \
                      y, pl, plane, R, dz_cur_oflag);                                                                 \
        break
    switch (ktaps) {
        DZ_DW(1);
        DZ_DW(3);
        DZ_DW(7);
        DZ_DW(11);
        DZ_DW(15);
        default:
            dz_set_error("ttn_depthwise: %d taps (built for 1, 3, 7, 11, 15)", ktaps);
            return 2;
    }
#undef DZ_DW
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_ttn_se_fc(const float* s, const float* w1, const float* w2t, int rows, int C, float* gate, hipStream_t st) {
    DZ_REQUIRE(C % 1024 == 0 && C <= 3072, "ttn_se_fc: %d channels (1024 or 3072)", C);
    const int H = C / 8;
    DZ_LAUNCH(ttn_se_fc_kernel, dim3((rows + 1) / 2), dim3(256), sizeof(float) * 2 * (C + H), st, s, w1, w2t, rows, C, H,
              gate);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_ttn_apply(const float* y, const float* gate, const float* resid, float* out, void* planes,
                        long long plane, int rows, int T, int C, hipStream_t st) {
    DZ_REQUIRE(y && gate && out && C % 32 == 0 && plane % 4 == 0, "ttn_apply: bad operands");
    DZ_REQUIRE((((uintptr_t)y | (uintptr_t)gate | (uintptr_t)resid | (uintptr_t)out | (uintptr_t)planes) & 15) == 0,
               "ttn_apply: operands must be 16-byte aligned");
    const long long R = (long long)rows * T;
    const dim3 grid((C + 127) / 128, (unsigned)((R + 7) / 8));
    unsigned short* pl = reinterpret_cast<unsigned short*>(planes);
    if (resid)
        DZ_LAUNCH(ttn_apply_kernel<true>, grid, dim3(256), 0, st, y, gate, resid, out, pl, plane, R, T, C, dz_cur_oflag);
    else
        DZ_LAUNCH(ttn_apply_kernel<false>, grid, dim3(256), 0, st, y, gate, resid, out, pl, plane, R, T, C, dz_cur_oflag);
    DZ_HIP(hipGetLastError());
    return 0;
}
