// Kernels of the speechbrain ResNet speaker embedding (speechbrain/spkrec-resnet-voxceleb, sbr_api.hip) that are not
// a convolution of the trunk (k_conv2d.hip's masked instances) or a GEMM of the head (k_convgemm.hip / k_gemm_split.hip).
//   sbr_extents    a row's live time steps at the stem and after each of the four layers
//   sbr_stem       Conv2d(1, C, 3, pad 1) + bias + folded BatchNorm + ReLU, zero padded at the row's own steps
//   sbr_se_sum     squeeze: sums over the row's live positions, in slices
//   sbr_se_fc      mean -> Linear -> ReLU -> Linear -> sigmoid
//   sbr_se_apply   ReLU(gate y + shortcut), zeros in the dead tail
//   sbr_att_pool   softmax over the row's frames per channel -> mean | std
// Activations are channels-last [row][t][f][c]: time is the slow spatial axis, so a row's dead frames (the buffer
// has Tb steps per row, the row's batch ext[row] of them) are one contiguous tail of zeros.  Every reduction runs in an
// order fixed by the row's own geometry: a row's result does not depend on the batch or on its place in it.
#include "dz_common.h"

namespace {

__global__ void sbr_extents_kernel(const int* __restrict__ tdev, int rows, int s0, int s1, int s2, int s3,
                                   int* __restrict__ ext) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int s[4] = {s0, s1, s2, s3};
    int e = tdev[r];
    ext[r] = e;
    for (int l = 0; l < 4; ++l) {
        e = (e - 1) / s[l] + 1;
        ext[(l + 1) * rows + r] = e;
    }
}

// thread = four channels of one output position; the taps in the order kt 3 + kf, bias last (wsp_conv1_kernel's order)
__global__ __launch_bounds__(256) void sbr_stem_kernel(const float* __restrict__ feats, int Tb, int F, int C,
                                                       long long total4, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const int* __restrict__ ext,
                                                       float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int q = C >> 2;
    const int c = (int)(idx % q) * 4;
    const long long pos = idx / q;
    const int f = (int)(pos % F);
    const long long bt = pos / F;
    const int t = (int)(bt % Tb);
    const int row = (int)(bt / Tb);
    const int e = ext[row];
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    if (t < e) {
        const float* xb = feats + (long long)row * Tb * F;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int ti = t + kt - 1;
#pragma unroll
            for (int kf = 0; kf < 3; ++kf) {
                const int fi = f + kf - 1;
                const float v = (ti >= 0 && ti < e && fi >= 0 && fi < F) ? xb[(long long)ti * F + fi] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(v, w[(c + j) * 9 + kt * 3 + kf], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = fmaxf(acc[j] + bias[c + j], 0.f);
    }
    *reinterpret_cast<f32x4*>(y + pos * C + c) = out;
}

// grid (slices, rows).  Slice s owns the live positions [s n / S, (s + 1) n / S) of the row's n = ext F; inside it,
// part p of 256 / (C / 4) walks positions p, p + parts, ... and the parts are added in ascending order.
__global__ __launch_bounds__(256) void sbr_se_sum_kernel(const float* __restrict__ y, int Tb, int F, int C,
                                                         const int* __restrict__ ext, float* __restrict__ part) {
    __shared__ f32x4 red[256];
    const int s = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
    const int q = C >> 2, parts = 256 / q;
    const int n = ext[row] * F;
    const int p0 = (int)((long long)s * n / DZ_SBR_SE_SLICES), p1 = (int)((long long)(s + 1) * n / DZ_SBR_SE_SLICES);
    const int cq = tid % q, pt = tid / q;
    const float* yr = y + (long long)row * Tb * F * C + cq * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (pt < parts)
        for (int p = p0 + pt; p < p1; p += parts) a += *reinterpret_cast<const f32x4*>(yr + (long long)p * C);
    red[tid] = a;
    __syncthreads();
    if (tid < q) {
        f32x4 t = red[tid];
        for (int k = 1; k < parts; ++k) t += red[k * q + tid];
        *reinterpret_cast<f32x4*>(part + ((long long)row * DZ_SBR_SE_SLICES + s) * C + tid * 4) = t;
    }
}

// one workgroup per row; the two matrices transposed, so consecutive threads read consecutive floats
__global__ __launch_bounds__(256) void sbr_se_fc_kernel(const float* __restrict__ part, int F, int C, int Cr,
                                                        const int* __restrict__ ext, const float* __restrict__ w1t,
                                                        const float* __restrict__ b1, const float* __restrict__ w2t,
                                                        const float* __restrict__ b2, float* __restrict__ gate) {
    __shared__ float mean[1024], h[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float n = (float)(ext[row] * F);
    const float* pr = part + (long long)row * DZ_SBR_SE_SLICES * C;
    for (int c = tid; c < C; c += 256) {
        float s = pr[c];
        for (int k = 1; k < DZ_SBR_SE_SLICES; ++k) s += pr[k * C + c];
        mean[c] = s / n;
    }
    __syncthreads();
    for (int j = tid; j < Cr; j += 256) {
        float a = 0.f;
        for (int c = 0; c < C; ++c) a = fmaf(w1t[c * Cr + j], mean[c], a);
        h[j] = fmaxf(a + b1[j], 0.f);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float a = 0.f;
        for (int j = 0; j < Cr; ++j) a = fmaf(w2t[j * C + c], h[j], a);
        gate[(long long)row * C + c] = 1.f / (1.f + expf(-(a + b2[c])));
    }
}

__global__ __launch_bounds__(256) void sbr_se_apply_kernel(const float* __restrict__ y, const float* __restrict__ gate,
                                                           const float* __restrict__ r, int Tb, int F, int C,
                                                           long long total4, const int* __restrict__ ext,
                                                           float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int q = C >> 2;
    const int c = (int)(idx % q) * 4;
    const long long pos = idx / q;
    const long long bt = pos / F;
    const int t = (int)(bt % Tb), row = (int)(bt / Tb);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (t < ext[row]) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + pos * C + c);
        const f32x4 s = *reinterpret_cast<const f32x4*>(r + pos * C + c);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gate + (long long)row * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaxf(fmaf(g[j], v[j], s[j]), 0.f);
    }
    *reinterpret_cast<f32x4*>(out + pos * C + c) = o;
}

// grid (C / 256, rows), thread = channel.  Three walks over the row's n frames in ascending order: the maximum, the
// softmax sums with the mean, the variance about that mean (sum w (x - mu)^2 = sum w x^2 - mu^2 without its
// cancellation), clamped at 1e-5 before the root.
__global__ __launch_bounds__(256) void sbr_att_pool_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                           int ldl, int Tb, int C, const int* __restrict__ ext,
                                                           float* __restrict__ pooled) {
    const int c = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (c >= C) return;
    const int n = ext[row];
    const float* xr = x + (long long)row * Tb * C + c;
    const float* lr = logits + (long long)row * Tb * ldl + c;
    float mx = -INFINITY;
    for (int t = 0; t < n; ++t) mx = fmaxf(mx, lr[(long long)t * ldl]);
    float s = 0.f, a = 0.f;
    for (int t = 0; t < n; ++t) {
        const float e = expf(lr[(long long)t * ldl] - mx);
        s += e;
        a = fmaf(e, xr[(long long)t * C], a);
    }
    const float mu = a / s;
    float v = 0.f;
    for (int t = 0; t < n; ++t) {
        const float e = expf(lr[(long long)t * ldl] - mx), d = xr[(long long)t * C] - mu;
        v = fmaf(e * d, d, v);
    }
    pooled[(long long)row * 2 * C + c] = mu;
    pooled[(long long)row * 2 * C + C + c] = sqrtf(fmaxf(v / s, 1e-5f));
}

}  // namespace

int dz_launch_sbr_extents(const int* tdev, int rows, int s0, int s1, int s2, int s3, int* ext, hipStream_t st) {
    DZ_REQUIRE(tdev && ext && rows >= 1, "sbr_extents: bad operands");
    DZ_REQUIRE(s0 >= 1 && s1 >= 1 && s2 >= 1 && s3 >= 1, "sbr_extents: strides %d %d %d %d", s0, s1, s2, s3);
    DZ_LAUNCH(sbr_extents_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, tdev, rows, s0, s1, s2, s3, ext);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_sbr_stem(const float* feats, int rows, int Tb, int F, int C, const float* w, const float* b,
                       const int* ext, float* y, hipStream_t st) {
    DZ_REQUIRE(feats && w && b && ext && y, "sbr_stem: NULL operand");
    DZ_REQUIRE(rows >= 1 && Tb >= 1 && F >= 1 && C >= 4 && C % 4 == 0, "sbr_stem: rows %d, Tb %d, F %d, C %d", rows, Tb,
               F, C);
    const long long total4 = (long long)rows * Tb * F * (C / 4);
    DZ_LAUNCH(sbr_stem_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, feats, Tb, F, C, total4, w, b,
              ext, y);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_sbr_se_sum(const float* y, int rows, int Tb, int F, int C, const int* ext, float* part, hipStream_t st) {
    DZ_REQUIRE(y && ext && part, "sbr_se_sum: NULL operand");
    DZ_REQUIRE(rows >= 1 && Tb >= 1 && F >= 1 && C >= 4 && C % 4 == 0 && C <= 1024, "sbr_se_sum: rows %d, Tb %d, F %d, C %d",
               rows, Tb, F, C);
    DZ_LAUNCH(sbr_se_sum_kernel, dim3(DZ_SBR_SE_SLICES, rows), dim3(256), 0, st, y, Tb, F, C, ext, part);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_sbr_se_fc(const float* part, int rows, int F, int C, int Cr, const int* ext, const float* w1t,
                        const float* b1, const float* w2t, const float* b2, float* gate, hipStream_t st) {
    DZ_REQUIRE(part && ext && w1t && b1 && w2t && b2 && gate, "sbr_se_fc: NULL operand");
    DZ_REQUIRE(rows >= 1 && F >= 1 && C >= 1 && C <= 1024 && Cr >= 1 && Cr <= 1024, "sbr_se_fc: rows %d, C %d, Cr %d", rows,
               C, Cr);
    DZ_LAUNCH(sbr_se_fc_kernel, dim3(rows), dim3(256), 0, st, part, F, C, Cr, ext, w1t, b1, w2t, b2, gate);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_sbr_se_apply(const float* y, const float* gate, const float* r, int rows, int Tb, int F, int C,
                           const int* ext, float* out, hipStream_t st) {
    DZ_REQUIRE(y && gate && r && ext && out, "sbr_se_apply: NULL operand");
    DZ_REQUIRE(rows >= 1 && Tb >= 1 && F >= 1 && C >= 4 && C % 4 == 0, "sbr_se_apply: rows %d, Tb %d, F %d, C %d", rows,
               Tb, F, C);
    const long long total4 = (long long)rows * Tb * F * (C / 4);
    DZ_LAUNCH(sbr_se_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, y, gate, r, Tb, F, C, total4,
              ext, out);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_sbr_att_pool(const float* x, const float* logits, int ldl, int rows, int Tb, int C, const int* ext,
                           float* pooled, hipStream_t st) {
    DZ_REQUIRE(x && logits && ext && pooled, "sbr_att_pool: NULL operand");
    DZ_REQUIRE(rows >= 1 && Tb >= 1 && C >= 1 && ldl >= C, "sbr_att_pool: rows %d, Tb %d, C %d, ldl %d", rows, Tb, C, ldl);
    DZ_LAUNCH(sbr_att_pool_kernel, dim3((C + 255) / 256, rows), dim3(256), 0, st, x, logits, ldl, Tb, C, ext, pooled);
    DZ_HIP(hipGetLastError());
    return 0;
}
