// Adaptive s-norm of the gallery match: every distance expressed in standard deviations of the distances that its two
// sides get against their nearest impostors of a fixed COHORT.
//
//   cohort C (M, D) of UNIT-NORM rows (packed), 1 <= M <= 8192, 1 <= top_n <= M; for a vector v
//       d_v[m]        = 1 - (v . c_m) / |v|                                  (the gallery's distance, k_gallery.hip)
//       (mu_v, sd_v)  = mean and population deviation of the top_n SMALLEST d_v[m];  sd_v = max(sd_v, 1e-3)
//   and for an embedding row x and a voiceprint g_e, with d = 1 - (x . g_e) / |x|,
//       dn[r][e]      = 0.5 ((d - mu_g[e]) / sd_g[e] + (d - mu_x[r]) / sd_x[r])         (signed; lower is closer)
//   index / best / second are the gallery's fold over dn.  An unusable row (NaN / Inf element, zero norm) gets NaN
//   statistics and -1 / NaN / NaN.
//
// Kernels (the row norms and the final fold are k_gallery.hip's own norm and reduce kernels):
//
//   1. cohort_tile_kernel<VEC, false>   the 64 x 128 tile of k_gallery.hip's gallery_tile_kernel with the cohort in the
//                                       voiceprints' place: the SAME staging, swizzle and MFMA order, so a (row, member)
//                                       pair walks k exactly as a (row, voiceprint) pair does and keeps the bound
//                                       (D + 8) 2^-24.  The epilogue stores d to scratch, 16 bytes per lane and store.
//                                       Scratch: PASS = 256 rows x (M rounded up to 128) floats, at most 8 MiB per
//                                       handle; more rows go in passes of 256 on the one stream.
//   2. cohort_stats_kernel              one workgroup per row.  The row's M distances go to LDS as their
//                                       order-preserving integer image (32 KiB at M = 8192); four 8-bit radix passes
//                                       (LDS integer histograms, one wave scans the 256 bins) find t, the top_n-th
//                                       smallest, and c = top_n - #{d < t}.  Then
//                                           S1 = sum_{d < t} d + c t,   S2 = sum_{d < t} d^2 + c t^2     (float64)
//                                       thread i adds elements i, i + 256, ... in ascending order, then a fixed xor
//                                       butterfly per wave, then waves 0 + 1 + 2 + 3.
//                                           mean = S1 / top_n,  sd = sqrt(max(S2 / top_n - mean^2, 0))   (float64)
//                                       rounded to float32 once; sd then floored at 1e-3f; inv = 1.f / sd (float32).
//   3. cohort_tile_kernel<VEC, true>    the gallery tile with the normalising epilogue before the best-two fold.
//                                       Float32 operation order, no contraction (fp contract off in the epilogue):
//                                           d  = 1.f - acc / norm[r]
//                                           a  = (d - mu_g[e]) * inv_g[e]
//                                           b  = (d - mu_x[r]) * inv_x[r]
//                                           dn = 0.5f * (a + b)
//
// Determinism.  The distance bits of a (vector, member) pair depend on the two vectors only (k_gallery.hip's argument:
// one fixed k order, the accumulator starts at +0, the division is by the row's norm).  The selection is exact integer
// work: t and c are functions of the multiset of the row's distances.  The float64 sums add element m at a place fixed
// by m and M alone (thread m & 255, its (m >> 8)-th addition; a + b == b + a makes the butterfly's result the same in
// every lane), so (mean, sd, inv) depend on the vector, the stored cohort and top_n only: not on R, the row's place in
// its batch or pass, its alignment or stride, or the call.  dn is a fixed sequence of float32 operations on d and four
// such values; every later step is the gallery's associative and commutative fold.  No atomics on floats; the only
// atomics are integer adds on the LDS histogram, whose sums do not depend on their order.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): the table is in DESIGN.md 4.20.
#include "dz_common.h"
#include <math.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BR = 64;                       // embedding rows per tile
constexpr int BE = 128;                      // voiceprints / cohort members per tile
constexpr int KT = 32;                       // floats of a k-tile: 8 chunks of 16 bytes per row
constexpr int G_BYTES = BE * KT * 4;         // 16 KiB
constexpr int X_BYTES = BR * KT * 4;         //  8 KiB
constexpr int STAGE = G_BYTES + X_BYTES;
constexpr int INT_BIG = 0x7fffffff;
constexpr int MAX_COHORT = 8192;
constexpr float SIGMA_FLOOR = 1e-3f;

// the gallery's best-two fold (k_gallery.hip keeps its own copy: its kernels' text is pinned by its tests)
struct Best2 {
    float d, s;      // best and second-best distance
    int i;           // index of the best (INT_BIG: none yet)
};

// candidate (d, i) into b; NaN never enters (every comparison with it is false)
__device__ __forceinline__ void take(Best2& b, float d, int i) {
    if (d < b.d || (d == b.d && i < b.i)) {
        b.s = b.d;
        b.d = d;
        b.i = i;
    } else if (d < b.s) {
        b.s = d;
    }
}

// two folds over disjoint sets of voiceprints -> the fold over their union
__device__ __forceinline__ void merge(Best2& a, const Best2& o) {
    if (o.d < a.d || (o.d == a.d && o.i < a.i)) {
        a.s = fminf(a.d, o.s);
        a.d = o.d;
        a.i = o.i;
    } else {
        a.s = fminf(a.s, o.d);
    }
}

__device__ __forceinline__ Best2 shuffled(const Best2& b, int mask) {
    Best2 o;
    o.d = __shfl_xor(b.d, mask, 64);
    o.s = __shfl_xor(b.s, mask, 64);
    o.i = __shfl_xor(b.i, mask, 64);
    return o;
}

// VEC: the rows are 16-byte aligned at a stride that is a multiple of 4 floats
template <bool VEC>
__device__ __forceinline__ f32x4 load_chunk(const float* p) {
    if (VEC) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v;
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
    v[3] = p[3];
    return v;
}

// what the epilogue of a tile does with its distances
struct TileOut {
    // NORM == false: d -> dist[row * ld + member], ld a multiple of 128 (columns M .. ld - 1 are written, never read)
    float* dist;
    int ld;
    // NORM == true: the statistics of both sides and the (row, gallery tile) partial results
    const float *mu_g, *inv_g, *mu_x, *inv_x;
    int tiles;
    int* p_idx;
    float *p_best, *p_second;
};

// ---------------------------------------------------------------------------------------------------------------
// The main loop is gallery_tile_kernel's, statement for statement: the k order of a pair is the contract.
template <bool VEC, bool NORM>
__global__ __launch_bounds__(256) void cohort_tile_kernel(const float* __restrict__ X, long long stride, int R, int D,
                                                          const float* __restrict__ G, int E,
                                                          const float* __restrict__ norm, TileOut out) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int tid = threadIdx.x;
    const int w = tid >> 6, l = tid & 63, li = l & 31, h = l >> 5;
    const int r0 = blockIdx.x * BR, e0 = blockIdx.y * BE;

    // ---- staging.  A k-tile of a row is 8 chunks of 16 bytes; chunk c of tile row j sits in slot c ^ (j & 7) of its
    // 128-byte LDS row.  Thread t fetches chunk t & 7 of gallery rows (t >> 3) + 32 i, i < 4, and of embedding rows
    // (t >> 3) + 32 i, i < 2.  Rows beyond E / R are zeros and never read from memory.
    const int c = tid & 7, j0 = tid >> 3;
    const int slot = (c ^ (j0 & 7)) << 4;                         // (j0 + 32 i) & 7 == j0 & 7
    f32x4 gv[4], xv[2];
    auto fetch = [&](int kt) {
        const int k = kt * KT + c * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + j0 + 32 * i;
            gv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (e < E) gv[i] = *reinterpret_cast<const f32x4*>(G + (long long)e * D + k);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r0 + j0 + 32 * i;
            xv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < R) xv[i] = load_chunk<VEC>(X + (long long)r * stride + k);
        }
    };
    auto park = [&](int st) {
        char* s = smem + st * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(s + (j0 + 32 * i) * 128 + slot) = gv[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(s + G_BYTES + (j0 + 32 * i) * 128 + slot) = xv[i];
    };

    f32x16 acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;

    const int nk = D / KT;
    fetch(0);
    park(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) fetch(kt + 1);                            // in flight under this tile's MFMAs
        const char* s = smem + (kt & 1) * STAGE;
        const char* sg = s + (32 * w + li) * 128;                  // this lane's voiceprint
        const char* sx = s + G_BYTES + li * 128;                   // ... and its embedding row of block 0 (block 1: + 32 rows)
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) {
            const int off = ((2 * ss + h) ^ (li & 7)) << 4;        // chunk 2 ss + h: k = 8 ss + 4 h + u
            const f32x4 gf = *reinterpret_cast<const f32x4*>(sg + off);
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(sx + off);
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(sx + 32 * 128 + off);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[u], x0[u], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[u], x1[u], acc[1], 0, 0, 0);
            }
        }
        // the stage written now was last read in iteration kt - 1, which every wave has left (the barrier below)
        if (kt + 1 < nk) park((kt + 1) & 1);
        __syncthreads();
    }

    // ---- C/D map: column = lane & 31 = embedding row of the block, register q = voiceprint
    // (q & 3) + 8 (q >> 2) + 4 h of the wave's 32
    if constexpr (!NORM) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int r = r0 + 32 * b + li;
            if (r >= R) continue;
            const float n = norm[r];
            float* row = out.dist + (long long)r * out.ld + e0 + 32 * w + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {                          // members 8 j + 4 h .. + 3 of the wave's 32: 16 bytes
                f32x4 d;
#pragma unroll
                for (int u = 0; u < 4; ++u) d[u] = 1.f - acc[b][4 * j + u] / n;
                *reinterpret_cast<f32x4*>(row + 8 * j) = d;
            }
        }
    } else {
        __shared__ Best2 fold[4][BR];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma clang fp contract(off)
            const int r = r0 + 32 * b + li;
            const bool live = r < R;
            const float n = live ? norm[r] : __builtin_nanf("");
            const float mx = live ? out.mu_x[r] : 0.f, ix = live ? out.inv_x[r] : 0.f;
            Best2 best{INFINITY, INFINITY, INT_BIG};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = e0 + 32 * w + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (e < E) {
                    const float d = 1.f - acc[b][q] / n;
                    const float ga = (d - out.mu_g[e]) * out.inv_g[e];
                    const float xb = (d - mx) * ix;
                    take(best, 0.5f * (ga + xb), e);
                }
            }
            merge(best, shuffled(best, 32));
            if (h == 0) fold[w][32 * b + li] = best;
        }
        __syncthreads();
        if (tid < BR && r0 + tid < R) {
            Best2 best = fold[0][tid];
            merge(best, fold[1][tid]);
            merge(best, fold[2][tid]);
            merge(best, fold[3][tid]);
            const long long o = (long long)(r0 + tid) * out.tiles + blockIdx.y;
            out.p_idx[o] = best.i;
            out.p_best[o] = best.d;
            out.p_second[o] = best.s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// order-preserving image of a float: a < b  <=>  key(a) < key(b) (as unsigned), -0 just below +0
__device__ __forceinline__ unsigned to_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_key(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void cohort_stats_kernel(const float* __restrict__ dist, int ld, int M, int top_n,
                                                           const float* __restrict__ norm, float* __restrict__ mean,
                                                           float* __restrict__ sd, float* __restrict__ inv) {
    __shared__ unsigned keys[MAX_COHORT];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[2];                                    // the prefix found so far, the rank still wanted
    __shared__ double part[2][4];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (!(norm[r] == norm[r])) {                                   // an unusable row: the whole workgroup leaves
        if (tid == 0) {
            const float nan = __builtin_nanf("");
            mean[r] = nan;
            sd[r] = nan;
            if (inv) inv[r] = nan;
        }
        return;
    }
    const float* d = dist + (long long)r * ld;
    for (int i = tid; i < M; i += 256) keys[i] = to_key(d[i]);
    if (tid == 0) {
        sel[0] = 0u;
        sel[1] = (unsigned)top_n;
    }
    // ---- radix select, most significant byte first: after pass p the top 8 (p + 1) bits of t are known
    for (int p = 0; p < 4; ++p) {
        const int shift = 24 - 8 * p;
        hist[tid] = 0u;
        __syncthreads();
        const unsigned long long prefix = sel[0];
        const unsigned want = sel[1];
        for (int i = tid; i < M; i += 256) {
            const unsigned k = keys[i];
            if (((unsigned long long)k >> (shift + 8)) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                            // lane l: bins 4 l .. 4 l + 3
            unsigned b[4], s = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                b[j] = hist[4 * tid + j];
                s += b[j];
            }
            unsigned incl = s;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned o = __shfl_up(incl, m, 64);
                if (tid >= m) incl += o;
            }
            unsigned before = incl - s;                            // candidates in the bins below this lane's
            if (before < want && want <= incl) {                   // exactly one lane: the counts sum to >= want
                bool found = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (found) continue;
                    if (want <= before + b[j]) {
                        sel[0] = (unsigned)((prefix << 8) | (unsigned)(4 * tid + j));
                        sel[1] = want - before;
                        found = true;
                    } else {
                        before += b[j];
                    }
                }
            }
        }
        __syncthreads();
    }
    const unsigned tkey = sel[0];
    const double t = (double)from_key(tkey), c = (double)sel[1];   // c of the values equal to t are among the top_n
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < M; i += 256) {
        const unsigned k = keys[i];
        if (k < tkey) {
            const double v = (double)from_key(k);
            s1 += v;
            s2 = fma(v, v, s2);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {                            // a + b == b + a: every lane holds the same bits
        s1 += __shfl_xor(s1, m, 64);
        s2 += __shfl_xor(s2, m, 64);
    }
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = s1;
        part[1][tid >> 6] = s2;
    }
    __syncthreads();
    if (tid == 0) {
        const double S1 = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3] + c * t;
        const double S2 = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3] + c * (t * t);
        const double mu = S1 / (double)top_n;
        const double var = S2 / (double)top_n - mu * mu;
        const float s = fmaxf((float)sqrt(var > 0.0 ? var : 0.0), SIGMA_FLOOR);
        mean[r] = (float)mu;
        sd[r] = s;
        if (inv) inv[r] = 1.f / s;
    }
}

template <bool NORM>
void launch_tile(const float* X, long long stride, int R, int D, const float* G, int E, const float* norm,
                 const TileOut& out, hipStream_t st) {
    const dim3 grid((R + BR - 1) / BR, (E + BE - 1) / BE);
    if ((((uintptr_t)X & 15) == 0) && stride % 4 == 0) {
        DZ_LAUNCH((cohort_tile_kernel<true, NORM>), grid, dim3(256), 0, st, X, stride, R, D, G, E, norm, out);
    } else {
        DZ_LAUNCH((cohort_tile_kernel<false, NORM>), grid, dim3(256), 0, st, X, stride, R, D, G, E, norm, out);
    }
}

}  // namespace

int dz_cohort_ld(int M) { return (M + BE - 1) / BE * BE; }

// norm: the R row norms (dz_launch_gallery_norm); dist: DZ_COHORT_PASS x dz_cohort_ld(M) floats of scratch;
// mean / sd / inv (inv may be NULL): R each, device or mapped pinned memory.  The caller has checked the shapes.
int dz_launch_cohort_stats(const float* X, long long stride, int R, int D, const float* C, int M, int top_n,
                           const float* norm, float* dist, float* mean, float* sd, float* inv, hipStream_t st) {
    const int ld = dz_cohort_ld(M);
    for (int r0 = 0; r0 < R; r0 += DZ_COHORT_PASS) {
        const int n = R - r0 < DZ_COHORT_PASS ? R - r0 : DZ_COHORT_PASS;
        TileOut out{};
        out.dist = dist;
        out.ld = ld;
        launch_tile<false>(X + (long long)r0 * stride, stride, n, D, C, M, norm + r0, out, st);
        DZ_LAUNCH(cohort_stats_kernel, dim3(n), dim3(256), 0, st, dist, ld, M, top_n, norm + r0, mean + r0, sd + r0,
                  inv ? inv + r0 : nullptr);
    }
    DZ_HIP(hipGetLastError());
    return 0;
}

// the gallery's tile launch with the normalising epilogue; p_*: R x dz_gallery_tiles(E) each
int dz_launch_gallery_tile_norm(const float* X, long long stride, int R, int D, const float* G, int E,
                                const float* norm, const float* mu_g, const float* inv_g, const float* mu_x,
                                const float* inv_x, int* p_idx, float* p_best, float* p_second, hipStream_t st) {
    TileOut out{};
    out.mu_g = mu_g;
    out.inv_g = inv_g;
    out.mu_x = mu_x;
    out.inv_x = inv_x;
    out.tiles = dz_gallery_tiles(E);
    out.p_idx = p_idx;
    out.p_best = p_best;
    out.p_second = p_second;
    launch_tile<true>(X, stride, R, D, G, E, norm, out, st);
    DZ_HIP(hipGetLastError());
    return 0;
}
