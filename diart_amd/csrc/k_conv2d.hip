// Implicit-GEMM 2-D convolution (WeSpeaker ResNet34's 3x3 / 1x1 convolutions) on the matrix cores.
//
//   Y[m][n] = epi( sum_{kh,kw,c} X[b][fo*s + kh - pad][to*s + kw - pad][c] * W[n][(kh*3 + kw)*Cin + c] + bias[n] )
//   m = (b*Fo + fo)*To + to,   epi = (+ R[m][n]) -> (ReLU)
//
// Channels-last activations [row][f][t][c]: the output IS the [M][Cout] matrix the next layer reads, and each 8-wide
// (split) or 4-wide (f32) k chunk of an im2col row is a contiguous channel vector of one tap (Cin % 32 == 0), or
// zeros where the tap falls into the zero padding.  Rows of the GEMM are output positions of every row of the
// batch: a tile may hold the end of one row and the start of the next; nothing couples them (each output element
// is its own dot product in a fixed k order), so a row's result does not depend on its neighbours or on the batch.
//
// Two arithmetic modes, the two the project ships (k_gemm_split.hip / k_convgemm.hip):
//  * split-f16: activations split into (hi, lo * 2^11) f16 pairs on the way into LDS, weights pre-split on the host,
//    three v_mfma_f32_32x32x16_f16 per product into two f32 accumulators.  Tile (32 WM) x (32 WN NB) x 32 k,
//    WM x WN waves, wave tile 32 x 32 NB.  WM = 4 throughout; the N shape follows Cout: 128 x 32 (layer 1, Cout
//    32: 4 waves, no idle half-tile of weights), 128 x 64 (layer 2), 128 x 128 (layers 3 / 4).
//  * exact f32: v_mfma_f32_16x16x4_f32, tile 96 x BN x 32 k, 2 x 2 waves, BN = min(Cout, 128).
// Layer 1 has K = 288 = 9 k-tiles: both modes keep one k-tile in flight ahead of the MFMAs, so a short K
// does not pay for a deeper pipeline's prologue.
//
// One text, two instantiations (MASKED; DzConv2d.ext set selects true: the speechbrain ResNet, sbr_api.hip): the
// masked instances have the same tiles and arithmetic, and row b is live for its first ext[b] steps of the slow
// spatial axis (F: time there) only — every output at or past them is stored as exactly 0.0.  With zeros there the
// unchanged im2col load reads the zero padding a batch padded to ext[b] steps has, for stride 1 and stride 2.  A tile
// that lies wholly in one row's dead tail loads nothing.  Two places differ, both `if (!MASKED || ...)`: the k loop
// (dead_tile) and the epilogue (live_at); the plain instances compile to what they were without the parameter.
#include "dz_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int KT = 32;
constexpr float LO_SCALE = 2048.f, LO_UNSCALE = 1.f / 2048.f;
constexpr float F16_MAX = 65504.f;

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ int chunk_off(int row, int cidx) { return row * 64 + ((cidx ^ ((row >> 2) & 3)) << 4); }

__device__ __forceinline__ void split8(const float* v, u32x4& hi, u32x4& lo, float& amax) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        amax = fmaxf(amax, fmaxf(fabsf(v[2 * e]), fabsf(v[2 * e + 1])));
        const f32x2 x = {__builtin_amdgcn_fmed3f(v[2 * e], -F16_MAX, F16_MAX),
                         __builtin_amdgcn_fmed3f(v[2 * e + 1], -F16_MAX, F16_MAX)};
        const f16x2 h = __builtin_convertvector(x, f16x2);
        const f32x2 r = (x - __builtin_convertvector(h, f32x2)) * LO_SCALE;
        hi[e] = __builtin_bit_cast(unsigned, h);
        lo[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    }
}

// One im2col row of the GEMM: the output position it stands for, decoded once per thread.
struct Row {
    const float* xb;   // row b of X
    int f0, t0;        // top-left input coordinate of the receptive field (may be -1)
    bool ok;           // m < M
};
__device__ __forceinline__ Row decode_row(const DzConv2d& p, long long m) {
    Row r;
    const long long M = (long long)p.B * p.Fo * p.To;
    r.ok = m < M;
    if (!r.ok) m = 0;
    const int per = p.Fo * p.To;
    const int b = (int)(m / per);
    const int rem = (int)(m - (long long)b * per);
    const int fo = rem / p.To, to = rem - fo * p.To;
    const int pad = p.taps == 9 ? 1 : 0;
    r.xb = p.X + (long long)b * p.Fi * p.Ti * p.Cin;
    r.f0 = fo * p.stride - pad;
    r.t0 = to * p.stride - pad;
    return r;
}
// address of channel c of tap `tap` for this row, or NULL in the zero padding
__device__ __forceinline__ const float* tap_ptr(const DzConv2d& p, const Row& r, int tap, int c) {
    const int kh = tap / 3, kw = tap - kh * 3;
    const int fi = r.f0 + kh, ti = r.t0 + kw;
    if (!r.ok || fi < 0 || fi >= p.Fi || ti < 0 || ti >= p.Ti) return nullptr;
    return r.xb + ((long long)fi * p.Ti + ti) * p.Cin + c;
}

__device__ __forceinline__ float epilogue(const DzConv2d& p, long long m, int n, float v) {
    v += p.bias[n];
    if (p.R) v += p.R[m * p.Cout + n];
    return p.relu ? fmaxf(v, 0.f) : v;
}

// masked instances: is output position m inside its row's live steps?
__device__ __forceinline__ bool live_at(const DzConv2d& p, long long m) {
    const int per = p.Fo * p.To;
    const int b = (int)(m / per);
    return (int)(m - (long long)b * per) < p.ext[b] * p.To;
}
// does the tile [m0, m0 + BM) lie wholly in the dead tail of one row?  (uniform over the workgroup)
__device__ __forceinline__ bool dead_tile(const DzConv2d& p, long long m0, int BM) {
    const long long M = (long long)p.B * p.Fo * p.To;
    const int per = p.Fo * p.To;
    const long long m1 = (m0 + BM < M ? m0 + BM : M) - 1;
    const int b0 = (int)(m0 / per), b1 = (int)(m1 / per);
    return b0 == b1 && (int)(m0 - (long long)b0 * per) >= p.ext[b0] * p.To;
}

// ------------------------------------------------------------------------------------------------------------------
// split-f16
// ------------------------------------------------------------------------------------------------------------------
template <int WM, int WN, int NB>
struct SCfg {
    static constexpr int BM = 32 * WM, BN = 32 * WN * NB, T = 64 * WM * WN;
    static constexpr int RP = T / 4;                      // A rows staged per pass
    static constexpr int AP = BM / RP;                    // passes
    static constexpr int APLANE = BM * 64, BPLANE = BN * 64;
    static constexpr int STAGE = 2 * APLANE + 2 * BPLANE;
    static constexpr size_t LDS = 2 * STAGE;
    static_assert(BN * 4 <= T, "one B chunk per thread at most");
    static_assert(AP * RP == BM, "A rows must tile the passes");
};

template <int WM, int WN, int NB, bool MASKED>
__global__ __launch_bounds__(64 * WM * WN) void conv2d_split_kernel(DzConv2d p) {
    using C = SCfg<WM, WN, NB>;
    constexpr int BM = C::BM, BN = C::BN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int crow = tid >> 2, cidx = tid & 3;
    const bool has_b = tid < BN * 4;
    Row rows[C::AP];
#pragma unroll
    for (int a = 0; a < C::AP; ++a) rows[a] = decode_row(p, m0 + crow + a * C::RP);
    const int K = p.taps * p.Cin;
    const unsigned short* Whi = reinterpret_cast<const unsigned short*>(p.Wsplit);
    const unsigned short* Wlo = Whi + (long long)p.Cout * K;
    const long long wofs = (long long)(n0 + (has_b ? crow : 0)) * K + cidx * 8;

    float amax = 0.f;
    f32x4 ra[C::AP][2];
    u32x4 rbh, rbl;
    auto load_tile = [&](int kt) {
        const int k = kt * KT + cidx * 8;
        const int tap = k / p.Cin, c = k - tap * p.Cin;
#pragma unroll
        for (int a = 0; a < C::AP; ++a) {
            const float* x = tap_ptr(p, rows[a], tap, c);
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
            if (x) {
                v0 = *reinterpret_cast<const f32x4*>(x);
                v1 = *reinterpret_cast<const f32x4*>(x + 4);
            }
            ra[a][0] = v0;
            ra[a][1] = v1;
        }
        if (has_b) {
            const long long o = wofs + (long long)kt * KT;
            rbh = *reinterpret_cast<const u32x4*>(Whi + o);
            rbl = *reinterpret_cast<const u32x4*>(Wlo + o);
        }
    };
    auto store_tile = [&](int buf) {
        char* st = smem + buf * C::STAGE;
#pragma unroll
        for (int a = 0; a < C::AP; ++a) {
            const int off = chunk_off(crow + a * C::RP, cidx);
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = ra[a][0][e];
                v[4 + e] = ra[a][1][e];
            }
            u32x4 hi, lo;
            split8(v, hi, lo, amax);
            *reinterpret_cast<u32x4*>(st + off) = hi;
            *reinterpret_cast<u32x4*>(st + C::APLANE + off) = lo;
        }
        if (has_b) {
            const int off = chunk_off(crow, cidx);
            *reinterpret_cast<u32x4*>(st + 2 * C::APLANE + off) = rbh;
            *reinterpret_cast<u32x4*>(st + 2 * C::APLANE + C::BPLANE + off) = rbl;
        }
    };

    const int w = tid >> 6, l = tid & 63, li = l & 31, g = l >> 5;
    const int wm = w / WN, wn = w - wm * WN;
    f32x16 accm[NB], accx[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) accm[nb][r] = accx[nb][r] = 0.f;

    auto compute = [&](int buf) {
        const char* st = smem + buf * C::STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f16x8 ah, al, bh[NB], bl[NB];
            {
                const int off = chunk_off(wm * 32 + li, 2 * ks + g);
                ah = *reinterpret_cast<const f16x8*>(st + off);
                al = *reinterpret_cast<const f16x8*>(st + C::APLANE + off);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int off = chunk_off(wn * 32 * NB + nb * 32 + li, 2 * ks + g);
                bh[nb] = *reinterpret_cast<const f16x8*>(st + 2 * C::APLANE + off);
                bl[nb] = *reinterpret_cast<const f16x8*>(st + 2 * C::APLANE + C::BPLANE + off);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                accx[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[nb], accx[nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                accm[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[nb], accm[nb], 0, 0, 0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                accx[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[nb], accx[nb], 0, 0, 0);
        }
    };
    const int nk = K / KT;
    if (!MASKED || !dead_tile(p, m0, BM)) {
        load_tile(0);
        store_tile(0);
        lds_barrier();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) load_tile(kt + 1);
            compute(buf);
            if (kt + 1 < nk) store_tile(buf ^ 1);
            lds_barrier();
        }
    }
    dz_flag_range(p.oflag, amax);

    // C/D map of the 32x32 fragment: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const long long M = (long long)p.B * p.Fo * p.To;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = n0 + wn * 32 * NB + nb * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
            if (m < M) {
                float v = 0.f;
                if (!MASKED || live_at(p, m)) v = epilogue(p, m, n, accm[nb][r] + accx[nb][r] * LO_UNSCALE);
                p.Y[m * p.Cout + n] = v;
            }
        }
    }
}

template <int WM, int WN, int NB, bool MASKED>
int launch_split(const DzConv2d& p, hipStream_t st) {
    using C = SCfg<WM, WN, NB>;
    static DzAttrOnce attr_once;
    DZ_HIP(attr_once.raise((const void*)conv2d_split_kernel<WM, WN, NB, MASKED>, (int)C::LDS));
    const long long M = (long long)p.B * p.Fo * p.To;
    dim3 grid((unsigned)((M + C::BM - 1) / C::BM), p.Cout / C::BN);
    DZ_LAUNCH((conv2d_split_kernel<WM, WN, NB, MASKED>), grid, dim3(C::T), C::LDS, st, p);
    DZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// exact f32 (the tile and LDS image of k_convgemm.hip: [k/4][row ^ ((k/4)&3)][4], one ds_read_b128 per fragment)
// ------------------------------------------------------------------------------------------------------------------
constexpr int FBM = 96;
template <int BN>
struct FCfg {
    static constexpr int NT = BN / 32;
    static constexpr int A_F4 = FBM * 8 / 256;
    static constexpr int B_F4 = BN * 8 / 256;
    static constexpr int TILE = (FBM + BN) * KT;
    static constexpr size_t LDS = sizeof(float) * 2 * TILE;
};

template <int BN, bool MASKED>
__global__ __launch_bounds__(256) void conv2d_f32_kernel(DzConv2d p) {
    using C = FCfg<BN>;
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * FBM;
    const int n0 = blockIdx.y * BN;
    const int lrow = tid >> 3, lkq = tid & 7;
    Row rows[C::A_F4];
#pragma unroll
    for (int a = 0; a < C::A_F4; ++a) rows[a] = decode_row(p, m0 + lrow + 32 * a);
    const int K = p.taps * p.Cin;
    const float* Wt = p.W + (long long)(n0 + lrow) * K + lkq * 4;

    f32x4 ra[C::A_F4], rb[C::B_F4];
    auto load_tile = [&](int kt) {
        const int k = kt * KT + lkq * 4;
        const int tap = k / p.Cin, c = k - tap * p.Cin;
#pragma unroll
        for (int a = 0; a < C::A_F4; ++a) {
            const float* x = tap_ptr(p, rows[a], tap, c);
            ra[a] = x ? *reinterpret_cast<const f32x4*>(x) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int a = 0; a < C::B_F4; ++a)
            rb[a] = *reinterpret_cast<const f32x4*>(Wt + (long long)(32 * a) * K + kt * KT);
    };
    auto store_tile = [&](int buf) {
        float* As = fsm + buf * C::TILE;
        float* Bs = As + FBM * KT;
        const int sw = lkq & 3;
#pragma unroll
        for (int a = 0; a < C::A_F4; ++a)
            *reinterpret_cast<f32x4*>(As + (lkq * FBM + ((lrow + 32 * a) ^ sw)) * 4) = ra[a];
#pragma unroll
        for (int a = 0; a < C::B_F4; ++a)
            *reinterpret_cast<f32x4*>(Bs + (lkq * BN + ((lrow + 32 * a) ^ sw)) * 4) = rb[a];
    };

    const int w = tid >> 6, l = tid & 63, li = l & 15, q = l >> 4;
    const int wm = w >> 1, wn = w & 1;
    f32x4 acc[3][C::NT];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int nt = 0; nt < C::NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = K / KT;
    if (!MASKED || !dead_tile(p, m0, FBM)) {
        load_tile(0);
        store_tile(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) load_tile(kt + 1);
            const float* As = fsm + buf * C::TILE;
            const float* Bs = As + FBM * KT;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int kq = cc * 4 + q;
                f32x4 af[3], bf[C::NT];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt)
                    af[mt] = *reinterpret_cast<const f32x4*>(As + (kq * FBM + ((wm * 48 + mt * 16 + li) ^ q)) * 4);
#pragma unroll
                for (int nt = 0; nt < C::NT; ++nt)
                    bf[nt] = *reinterpret_cast<const f32x4*>(Bs + (kq * BN + ((wn * (BN / 2) + nt * 16 + li) ^ q)) * 4);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                        for (int nt = 0; nt < C::NT; ++nt) acc[mt][nt] = DZ_MFMA(af[mt][s], bf[nt][s], acc[mt][nt]);
            }
            if (kt + 1 < nk) store_tile(buf ^ 1);
            __syncthreads();
        }
    }

    const long long M = (long long)p.B * p.Fo * p.To;
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt) {
        const int n = n0 + wn * (BN / 2) + nt * 16 + li;
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm * 48 + mt * 16 + 4 * q + r;
                if (m < M) {
                    float v = 0.f;
                    if (!MASKED || live_at(p, m)) v = epilogue(p, m, n, acc[mt][nt][r]);
                    p.Y[m * p.Cout + n] = v;
                }
            }
    }
}

template <int BN, bool MASKED>
int launch_f32(const DzConv2d& p, hipStream_t st) {
    using C = FCfg<BN>;
    static DzAttrOnce attr_once;
    DZ_HIP(attr_once.raise((const void*)conv2d_f32_kernel<BN, MASKED>, (int)C::LDS));
    const long long M = (long long)p.B * p.Fo * p.To;
    dim3 grid((unsigned)((M + FBM - 1) / FBM), p.Cout / BN);
    DZ_LAUNCH((conv2d_f32_kernel<BN, MASKED>), grid, dim3(256), C::LDS, st, p);
    DZ_HIP(hipGetLastError());
    return 0;
}

template <bool MASKED>
int dispatch(const DzConv2d& p, hipStream_t st) {
    if (p.Wsplit) {
        if (p.Cout == 32) return launch_split<4, 1, 1, MASKED>(p, st);
        if (p.Cout == 64) return launch_split<4, 2, 1, MASKED>(p, st);
        return launch_split<4, 2, 2, MASKED>(p, st);
    }
    if (p.Cout == 32) return launch_f32<32, MASKED>(p, st);
    if (p.Cout == 64) return launch_f32<64, MASKED>(p, st);
    return launch_f32<128, MASKED>(p, st);
}

}  // namespace

int dz_launch_conv2d(const DzConv2d& p_in, hipStream_t st) {
    DzConv2d p = p_in;
    if (!p.oflag) p.oflag = dz_cur_oflag;
    DZ_REQUIRE(p.X && p.bias && p.Y && (p.W || p.Wsplit), "conv2d: NULL operand");
    DZ_REQUIRE(p.taps == 9 || p.taps == 1, "conv2d: %d taps (3x3 or 1x1 only)", p.taps);
    DZ_REQUIRE(p.Cin % KT == 0 && p.Cin >= KT, "conv2d: Cin %d must be a multiple of 32", p.Cin);
    DZ_REQUIRE(p.Cout == 32 || p.Cout == 64 || p.Cout % 128 == 0, "conv2d: Cout %d", p.Cout);
    DZ_REQUIRE(p.stride == 1 || p.stride == 2, "conv2d: stride %d", p.stride);
    DZ_REQUIRE(p.B >= 1 && p.Fi >= 1 && p.Ti >= 1, "conv2d: empty input");
    // output geometry of kernel 3 / pad 1 or kernel 1 / pad 0: (n - 1) / stride + 1 either way
    DZ_REQUIRE(p.Fo == (p.Fi - 1) / p.stride + 1 && p.To == (p.Ti - 1) / p.stride + 1, "conv2d: output geometry");
    return p.ext ? dispatch<true>(p, st) : dispatch<false>(p, st);
}
