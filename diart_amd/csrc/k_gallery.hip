// gallery_match: nearest enrolled voiceprint of every embedding row, on the EXACT-f32 matrix cores.
//
//   R rows x (D floats at any stride >= D)  against  a gallery G (E, D) of UNIT-NORM voiceprints (row-major, packed):
//       dist[r][e] = 1 - (x_r . g_e) / |x_r|                 (the clustering's cosine distance; |g_e| = 1 as stored)
//       index[r]   = argmin_e dist[r][e]  (lowest e among equal distances),  best[r] = its distance,
//       second[r]  = the smallest distance among the other voiceprints (+inf when E == 1)
//   A row with a NaN / Inf element, of zero norm, or whose norm is not a finite float gets -1 / NaN / NaN.
//
// Three launches on one stream, no atomics:
//
//   1. gallery_norm_kernel    one wave per row: sum of squares in float64 (lane l takes elements l, l + 64, ... in
//                             ascending order, then a fixed xor butterfly), norm[r] = (float) sqrt(sum); NaN marks an
//                             unusable row.  The order depends on the element's position IN THE ROW only.
//   2. gallery_tile_kernel    grid (ceil(R / 64), ceil(E / 128)): a 64-row x 128-voiceprint tile of dot products,
//                             k-tiles of 32 floats through two LDS stages (global -> registers -> LDS, the loads of
//                             tile kt + 1 in flight under the MFMAs of tile kt).  Four waves; wave w owns voiceprints
//                             32 w .. 32 w + 31 of the tile against both 32-row blocks: 2 accumulators of
//                             v_mfma_f32_32x32x2_f32, the VOICEPRINTS as the MFMA's row operand, so a lane ends with
//                             ONE embedding row (column = lane & 31) and 16 voiceprints in its registers: the best two
//                             of them are found in the lane, then lane ^ 32, then the four waves through LDS, and the
//                             tile's (index, best, second) of each row goes to scratch[row][gallery tile].
//   3. gallery_reduce_kernel  one wave per row: lane l folds gallery tiles l, l + 64, ..., then the butterfly; writes
//                             the three results (plain stores: device memory or pinned host memory mapped into the
//                             device).
//
// Determinism.  v_mfma_f32_32x32x2_f32 is bitwise an fmaf chain in k order (HIP guide, "FP32-input MFMA"), the
// accumulator starts at +0, and lane (row, h) of MFMA u of sub-step s of k-tile kt carries k = 32 kt + 8 s + 4 h + u for
// BOTH operands: every (row, voiceprint) pair walks k in the SAME fixed order (32 kt + 8 s + u, then + 4), whatever R,
// E, the voiceprint's place in the gallery, the row's place in the batch or its alignment (the aligned and the
// single-float loads fetch the same values).  The division is by norm[r] alone.  Hence the distance bits of a pair
// depend on the two vectors only; every later step is a comparison (d, index) -> lowest d, then lowest index, which
// is associative and commutative, so the order of the folds does not matter either.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): tile kernel 68 VGPRs + 32 AGPRs, 52 224 bytes
// of LDS, no scratch, 3 waves per SIMD; the table is in DESIGN.md 4.18.
#include "dz_common.h"
#include <math.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BR = 64;                       // embedding rows per tile
constexpr int BE = 128;                      // voiceprints per tile
constexpr int KT = 32;                       // floats of a k-tile: 8 chunks of 16 bytes per row
constexpr int G_BYTES = BE * KT * 4;         // 16 KiB
constexpr int X_BYTES = BR * KT * 4;         //  8 KiB
constexpr int STAGE = G_BYTES + X_BYTES;
constexpr int INT_BIG = 0x7fffffff;

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

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gallery_norm_kernel(const float* __restrict__ X, long long stride, int R, int D,
                                                           float* __restrict__ norm) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (r >= R) return;                                            // whole waves leave: no barrier below
    const float* x = X + (long long)r * stride;
    double acc = 0.0;
    bool finite = true;
    for (int k = l; k < D; k += 64) {
        const float v = x[k];
        finite = finite && (fabsf(v) <= 3.402823466e38f);           // false for NaN and Inf
        acc = fma((double)v, (double)v, acc);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);   // a + b == b + a: every lane holds the same bits
    const bool all_finite = __all(finite);
    const float n = (float)sqrt(acc);
    if (l == 0) norm[r] = (all_finite && n > 0.f && n <= 3.402823466e38f) ? n : __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------------------
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

template <bool VEC>
__global__ __launch_bounds__(256) void gallery_tile_kernel(const float* __restrict__ X, long long stride, int R, int D,
                                                           const float* __restrict__ G, int E,
                                                           const float* __restrict__ norm, int tiles,
                                                           int* __restrict__ p_idx, float* __restrict__ p_best,
                                                           float* __restrict__ p_second) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    __shared__ Best2 fold[4][BR];
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
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int r = r0 + 32 * b + li;
        const float n = r < R ? norm[r] : __builtin_nanf("");
        Best2 best{INFINITY, INFINITY, INT_BIG};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = e0 + 32 * w + (q & 3) + 8 * (q >> 2) + 4 * h;
            const float d = 1.f - acc[b][q] / n;
            if (e < E) take(best, d, e);
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
        const long long o = (long long)(r0 + tid) * tiles + blockIdx.y;
        p_idx[o] = best.i;
        p_best[o] = best.d;
        p_second[o] = best.s;
    }
}

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gallery_reduce_kernel(const float* __restrict__ norm, int R, int tiles,
                                                             const int* __restrict__ p_idx,
                                                             const float* __restrict__ p_best,
                                                             const float* __restrict__ p_second,
                                                             int* __restrict__ index, float* __restrict__ dist,
                                                             float* __restrict__ second) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (r >= R) return;
    Best2 best{INFINITY, INFINITY, INT_BIG};
    for (int t = l; t < tiles; t += 64) {
        const long long o = (long long)r * tiles + t;
        Best2 part{p_best[o], p_second[o], p_idx[o]};
        merge(best, part);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) merge(best, shuffled(best, m));
    if (l == 0) {
        const bool usable = norm[r] == norm[r] && best.i != INT_BIG;
        index[r] = usable ? best.i : -1;
        dist[r] = usable ? best.d : __builtin_nanf("");
        second[r] = usable ? best.s : __builtin_nanf("");
    }
}

}  // namespace

int dz_gallery_tiles(int E) { return (E + BE - 1) / BE; }

// scratch: norm (max_rows floats) | p_idx | p_best | p_second (max_rows * tiles each); the caller has checked the shapes
int dz_launch_gallery_match(const float* X, long long stride, int R, int D, const float* G, int E, float* norm,
                            int* p_idx, float* p_best, float* p_second, int* index, float* dist, float* second,
                            hipStream_t st) {
    const int tiles = dz_gallery_tiles(E);
    DZ_LAUNCH(gallery_norm_kernel, dim3((R + 3) / 4), dim3(256), 0, st, X, stride, R, D, norm);
    const dim3 grid((R + BR - 1) / BR, tiles);
    if ((((uintptr_t)X & 15) == 0) && stride % 4 == 0) {
        DZ_LAUNCH(gallery_tile_kernel<true>, grid, dim3(256), 0, st, X, stride, R, D, G, E, norm, tiles, p_idx, p_best,
                  p_second);
    } else {
        DZ_LAUNCH(gallery_tile_kernel<false>, grid, dim3(256), 0, st, X, stride, R, D, G, E, norm, tiles, p_idx, p_best,
                  p_second);
    }
    DZ_LAUNCH(gallery_reduce_kernel, dim3((R + 3) / 4), dim3(256), 0, st, norm, R, tiles, p_idx, p_best, p_second, index,
              dist, second);
    DZ_HIP(hipGetLastError());
    return 0;
}

// the first and the last launch alone, for the normalised match (k_cohort.hip), whose tile kernel lies between them
int dz_launch_gallery_norm(const float* X, long long stride, int R, int D, float* norm, hipStream_t st) {
    DZ_LAUNCH(gallery_norm_kernel, dim3((R + 3) / 4), dim3(256), 0, st, X, stride, R, D, norm);
    DZ_HIP(hipGetLastError());
    return 0;
}

int dz_launch_gallery_reduce(const float* norm, int R, int E, const int* p_idx, const float* p_best,
                             const float* p_second, int* index, float* dist, float* second, hipStream_t st) {
    DZ_LAUNCH(gallery_reduce_kernel, dim3((R + 3) / 4), dim3(256), 0, st, norm, R, dz_gallery_tiles(E), p_idx, p_best,
              p_second, index, dist, second);
    DZ_HIP(hipGetLastError());
    return 0;
}
