// Kernels of the mel-spectrogram ECAPA-TDNN's front end (speechbrain/spkrec-ecapa-voxceleb-mel-spec; ecm_api.hip,
// DESIGN.md 4.15): torchaudio's MelSpectrogram(n_fft = win_length = 1024, hop 256, centred, reflect padding, power 1,
// slaney bank) -> log(clamp(., 1e-5)) -> sentence mean.  The STFT and the mel bank are GEMM instances (DzGemm); here is
// what surrounds them:
//   ecm_prep       each row's centre-padded signal, reflected at its GROUP's longest row (the padded batch is what the
//                  STFT sees), laid out for the overlapping-rows STFT
//   ecm_magnitude  sqrt(re^2 + im^2) of the (re | im) GEMM output
//   ecm_post       log(max(x, 1e-5)) and the mean over each row's valid frames
// The batch geometry itself (frames, valid / mask frames, flags) is ecapa_geometry_kernel's (k_ecapa.hip) with hop 256.
// No reduction order depends on the batch or on a row's place in it.
#include "dz_common.h"

namespace {

enum { NFFT = 1024, HALF = 512, BINS = 513, LDS_SPEC = 1028, LDM = 544, NMEL = 80, SIG_LEAD = 200 };

// one workgroup per (column block of 1024, row)
__global__ __launch_bounds__(256) void ecm_prep_kernel(const float* __restrict__ sig, long long sig_stride,
                                                       const int* __restrict__ lens, int K, float* __restrict__ csig,
                                                       long long cstride, int* __restrict__ lmax_out) {
    const int row = blockIdx.y, r0 = row / K * K;
    int lmax = 0;
    for (int k = 0; k < K; ++k) {
        const int l = lens[r0 + k];
        lmax = max(lmax, l < 0 ? -l - 1 : l);
    }
    const int l0 = lens[row];
    const int len = l0 < 0 ? -l0 - 1 : l0;
    if (blockIdx.x == 0 && threadIdx.x == 0) lmax_out[row] = lmax;
    const float* x = sig + (long long)row * sig_stride + SIG_LEAD;
    float* o = csig + (long long)row * cstride;
    const bool live = lmax > HALF;             // (reflect padding of 512 needs more than 512 samples)
    const long long j0 = (long long)blockIdx.x * 1024;
    for (int q = threadIdx.x; q < 1024; q += 256) {
        const long long j = j0 + q;
        if (j >= cstride) break;
        float v = 0.f;
        if (live && j < (long long)lmax + NFFT) {
            int i = (int)j - HALF;
            i = i < 0 ? -i : i;
            i = i >= lmax ? 2 * (lmax - 1) - i : i;
            v = i < len ? x[i] : 0.f;          // (zeros behind the row's own length: pad_sequence)
        }
        o[j] = v;
    }
}

__global__ void ecm_magnitude_kernel(const float* __restrict__ spec, long long rows, float* __restrict__ mag) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * LDM) return;
    const long long r = idx / LDM;
    const int j = (int)(idx - r * LDM);
    float v = 0.f;
    if (j < BINS) {
        const float re = spec[r * LDS_SPEC + j], im = spec[r * LDS_SPEC + BINS + j];
        v = __fsqrt_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)));
    }
    mag[idx] = v;
}

// mel magnitudes [row][T][80] -> features [row][T][80]: x = log(max(x, 1e-5)), minus the per-mel mean over the first
// nvalid[row] frames (InputNormalization("sentence", std_norm = False)).  The sums are split over 3 thread groups
// (frames part, part + 3, ...) and combined in the fixed order (0 + 1) + 2, as fbank_post_mels_kernel<80> does.
__global__ __launch_bounds__(256) void ecm_post_kernel(const float* __restrict__ melp, int T,
                                                       const int* __restrict__ nvalid, float* __restrict__ feats) {
    __shared__ float msum[3][NMEL];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* x = melp + (long long)row * T * NMEL;
    float* y = feats + (long long)row * T * NMEL;
    const int nv = nvalid[row];
    if (tid < 3 * NMEL) {
        const int m = tid % NMEL, part = tid / NMEL;
        float s = 0.f;
        for (int t = part; t < nv; t += 3) s += logf(fmaxf(x[t * NMEL + m], 1e-5f));
        msum[part][m] = s;
    }
    __syncthreads();
    for (int i = tid; i < T * NMEL; i += 256) {
        const int m = i % NMEL;
        const float mean = ((msum[0][m] + msum[1][m]) + msum[2][m]) / (float)nv;
        y[i] = logf(fmaxf(x[i], 1e-5f)) - mean;
    }
}

}  // namespace

int dz_launch_ecm_prep(const float* sig, long long sig_stride, const int* lens, int rows, int K, float* csig,
                       long long cstride, int* lmax_out, hipStream_t st) {
    DZ_REQUIRE(sig && lens && csig && lmax_out, "ecm_prep: NULL argument");
    DZ_REQUIRE(rows >= 1 && K >= 1 && rows % K == 0 && cstride >= NFFT && sig_stride >= SIG_LEAD,
               "ecm_prep: %d rows in groups of %d, strides %lld / %lld", rows, K, sig_stride, cstride);
    DZ_LAUNCH(ecm_prep_kernel, dim3((unsigned)((cstride + 1023) / 1024), rows), dim3(256), 0, st, sig, sig_stride, lens,
              K, csig, cstride, lmax_out);
    DZ_HIP(hipGetLastError());
    return 0;
}
int dz_launch_ecm_magnitude(const float* spec, long long rows, float* mag, hipStream_t st) {
    const long long n = rows * LDM;
    DZ_LAUNCH(ecm_magnitude_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, spec, rows, mag);
    DZ_HIP(hipGetLastError());
    return 0;
}
int dz_launch_ecm_post(const float* melp, int T, int rows, const int* nvalid, float* feats, hipStream_t st) {
    DZ_LAUNCH(ecm_post_kernel, dim3(rows), dim3(256), 0, st, melp, T, nvalid, feats);
    DZ_HIP(hipGetLastError());
    return 0;
}
