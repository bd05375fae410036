// Device-resident rolling window of N audio streams.
//
// Replaces, for the N-stream driver, rearrange_audio_stream
// (/root/reference/src/diart/operators.py:44-100: accumulate blocks until `duration` seconds are
// buffered, then emit the last `duration` seconds every `step` seconds) and the per-step upload
// of the whole window that follows it (blocks/segmentation.py:47 / blocks/embedding.py:52: the
// reference moves 320 KB per chunk to the device although only 32 KB of it are new).
//
// Layout: one row of 2*P floats per stream, P = W + slack*hop (W = window samples).  A new
// block of `hop` samples is written at positions p and p + P (p advances modulo P), so the newest
// W samples are ALWAYS one contiguous span [q, q + W) of the row, q = (p + slack*hop) mod P: the
// segmentation / embedding kernels read the rolling window in place through (base pointer +
// offset, row stride 2*P) with their usual coalesced 16-byte loads — no wrap-around logic in any
// kernel, nothing is copied or repeated.  The slack keeps a push from overwriting samples a forward
// pass of the previous `slack` windows may still be reading: block t+1 lands on the slot of
// block t+1-W/hop-slack, which belongs to windows <= t-slack only.
//
// ONE push path (ring_push) behind the three entry points.  dz_ring_push (lock step: every row at the
// common position, one launch whatever n), dz_ring_push_rows (float rows, each listed row at its own
// position: StreamServer, where every stream has its own pace) and dz_ring_push_rows_pcm (the same
// for raw client audio) check their arguments and call it.  It resolves the source once — pinned
// host memory read in place over PCIe, device memory, or ONE asynchronous H2D copy of the new samples
// into one of two landing blocks used alternately (the 2-D runtime copies into the ring this replaced
// cost the step ~0.3 ms of host and queue time) — launches ONE kernel template
// (ring_scatter_kernel<T, C>: load, convert, average the channels, store at both positions;
// <float, 1> copies bits) and does the position bookkeeping.  Only the new samples cross PCIe.
//
// dz_ring_gather copies the current windows of the listed rows, device to device, into the dense
// (k, W) batch the forward passes take — 320 KB per window at HBM speed instead of 320 KB per window
// over PCIe — with ONE kernel, 16 bytes per lane wherever that lane's piece allows it.
#include "dz_common.h"

#include <new>
#include <type_traits>
#include <utility>
#include <vector>

struct dz_ring {
    dz_ctx* ctx;
    int n, W, hop, P;
    long long pitch;   // floats between the rows of two streams: 2P rounded up to an ODD multiple of
                       // 256 bytes (2P itself is a large power-of-two multiple for the usual
                       // geometries: every stream's window then starts on the same HBM channel / L2
                       // set and the front-end kernels ran 25 % slower reading the ring than a
                       // dense stream array)
    float* buf;        // [n][2P]
    char* land;        // two landing blocks of `land_cap` bytes each for the H2D copies of pageable blocks, used
    size_t land_cap;   // alternately; a mono float32 block of all n rows fits from create on, wider formats grow it
    long long pushed;  // push calls so far, lock-step and per-row alike (dz_ring_window's `filled`, the landing blocks' turn)
    int pos;           // write position of the NEXT block, in [0, P)
    // per-row state (the per-row pushes / dz_ring_gather); a lock-step dz_ring_push moves every row
    std::vector<int> rpos;
    std::vector<long long> rpushed;
    bool aligned;      // hop % 4 == 0: every block and every window starts on a 16-byte boundary
};

// up to 64 (row, offset) pairs per launch, passed in the kernel-argument segment
struct DzRowList {
    int row[64];
    int off[64];
};

static long long round16(long long bytes) { return (bytes + 15) & ~15LL; }

extern "C" int dz_ring_create(dz_ctx* ctx, int n_streams, int window, int hop, int slack_blocks,
                              dz_ring** out) {
    DZ_REQUIRE(ctx && out, "dz_ring_create: NULL argument");
    DZ_REQUIRE(n_streams >= 1 && window >= 1 && hop >= 1 && slack_blocks >= 0,
               "dz_ring_create: empty geometry");
    // hop % 4 != 0 (44.1 kHz: 22 050 samples per 500 ms): blocks and windows start on 4-byte boundaries only; the
    // per-row entry points then move 4-byte pieces where a piece is not 16-byte aligned, dz_ring_window refuses
    DZ_REQUIRE(window % hop == 0, "dz_ring_create: window (%d) must be a multiple of hop (%d)", window, hop);
    DZ_HIP(hipSetDevice(ctx->device));
    dz_ring* r = new (std::nothrow) dz_ring;
    DZ_REQUIRE(r != nullptr, "dz_ring_create: out of memory");
    r->ctx = ctx; r->n = n_streams; r->W = window; r->hop = hop; r->buf = nullptr;
    r->aligned = hop % 4 == 0; r->land = nullptr;
    r->P = window + slack_blocks * hop;
    r->pushed = 0; r->pos = 0;
    r->rpos.assign(n_streams, 0);
    r->rpushed.assign(n_streams, 0);
    r->pitch = ((2LL * r->P + 63) / 64) * 64;
    if (((r->pitch / 64) & 1) == 0) r->pitch += 64;
    const size_t bytes = (size_t)n_streams * r->pitch * sizeof(float);
    hipError_t e = hipMalloc((void**)&r->buf, bytes);
    if (e != hipSuccess) {
        dz_set_error("dz_ring_create: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        delete r;
        return 1;
    }
    DZ_HIP(hipMemset(r->buf, 0, bytes));
    r->land_cap = (size_t)n_streams * round16((long long)hop * sizeof(float));
    e = hipMalloc((void**)&r->land, 2 * r->land_cap);
    if (e != hipSuccess) {
        dz_set_error("dz_ring_create: hipMalloc(landing blocks) failed: %s", hipGetErrorString(e));
        (void)hipFree(r->buf);
        delete r;
        return 1;
    }
    *out = r;
    return 0;
}

// ---------------------------------------------------------------------------
// Blocks -> ring (every push): load, convert, average the channels and store at `off` and
// `off + P` in ONE kernel.  Replaces, for live streams, the channel average of the reference's loader
// (reference audio.py:32-34, waveform.mean(dim=0)) and the int16 -> float conversion its clients
// do before they send.  The arithmetic is the header's definition, operation for operation: nothing is
// contracted (the sum is a chain of adds, the average one division), and one float channel is copied as bits.
// ---------------------------------------------------------------------------
// the three 1-byte formats share a storage type: a tag type each selects the conversion
struct pcm_u8 { unsigned char v; };
struct pcm_ulaw { unsigned char v; };
struct pcm_alaw { unsigned char v; };

__device__ __forceinline__ float pcm_to_f32(float v) { return v; }
__device__ __forceinline__ float pcm_to_f32(short v) { return (float)v * (1.0f / 32768.0f); }
__device__ __forceinline__ float pcm_to_f32(int v) { return (float)v * (1.0f / 2147483648.0f); }   // the conversion rounds
__device__ __forceinline__ float pcm_to_f32(pcm_u8 b) { return ((float)b.v - 128.0f) * (1.0f / 128.0f); }
// G.711 expansion in integer ALU (a dozen operations per byte, selects instead of branches: no table to stage, no
// LDS, nothing a wave could diverge on), then one exact int -> float conversion and one exact scaling
__device__ __forceinline__ float pcm_to_f32(pcm_ulaw b) {
    const int u = ~(int)b.v & 0xFF;
    const int t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7);
    const int L = (u & 0x80) ? 0x84 - t : t - 0x84;
    return (float)L * (1.0f / 32768.0f);
}
__device__ __forceinline__ float pcm_to_f32(pcm_alaw b) {
    const int a = (int)b.v ^ 0x55;
    const int m = (a & 0x0F) << 4;
    const int s = (a >> 4) & 7;
    const int t = (s == 0) ? m + 8 : (m + 0x108) << ((s - 1) & 7);     // (& 7: the shift of the unselected side stays defined)
    const int L = (a & 0x80) ? t : -t;
    return (float)L * (1.0f / 32768.0f);
}

// e: the C values of one frame
template <typename T, int C>
__device__ __forceinline__ float pcm_frame(const T* e) {
#pragma clang fp contract(off)
    float s = pcm_to_f32(e[0]);
    if (C == 1) return s;
#pragma unroll
    for (int c = 1; c < C; ++c) s = s + pcm_to_f32(e[c]);
    return s / (float)C;
}

// one frame at `src` (aligned to one value)
template <typename T, int C>
__device__ __forceinline__ float pcm_one_frame(const T* src) {
    T e[C];
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = src[c];
    return pcm_frame<T, C>(e);
}

// One lane's share of a row: the F = 16 / sizeof(T) frames at `src`, of which `left` lie inside the row, to o0 and,
// with TWICE, to o1.  With `vec` (all three 16-byte aligned) and left >= F: C 16-byte loads whatever the format, F / 4
// 16-byte stores per destination.  Otherwise (unaligned, or the lane that holds the ragged end of the row) the
// min(left, F) frames one by one.  The same arithmetic per frame either way.
template <typename T, int C, bool TWICE>
__device__ __forceinline__ void pcm_lane(const T* src, float* o0, float* o1, long long left, bool vec) {
    constexpr int F = 16 / sizeof(T);
    if (__builtin_expect(vec && left >= F, 1)) {      // (laid out first: the instructions of the usual lane are contiguous)
        union {
            f32x4 v[C];
            T e[F * C];
        } u;
        const f32x4* s = reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int c = 0; c < C; ++c) u.v[c] = s[c];
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = pcm_frame<T, C>(u.e + (4 * q + i) * C);
            *reinterpret_cast<f32x4*>(o0 + 4 * q) = o;
            if (TWICE) *reinterpret_cast<f32x4*>(o1 + 4 * q) = o;
        }
    } else {
#pragma nounroll
        for (int g = 0; g < F && g < left; ++g) {
            const float o = pcm_one_frame<T, C>(src + g * C);
            o0[g] = o;
            if (TWICE) o1[g] = o;
        }
    }
}

// lanes of a block of the push kernel: a 1-byte format's lane takes 16 frames, so one wave already covers 1 024
template <typename T>
constexpr int pcm_block_lanes() { return sizeof(T) == 1 ? 64 : 256; }

// THE push kernel.  Row j of `block` (rows `bstride` values apart): hop frames of C interleaved values of type T ->
// ring row rows.row[j] at rows.off[j] and rows.off[j] + P; with uni >= 0 (a lock-step push: one launch for any number
// of rows) -> ring row j at `uni`.  A block of L lanes covers L F frames, F = 16 / sizeof(T).  Where the input rows
// (in_vec) and this row's ring position (off and P multiples of 4) allow 16-byte access each LANE decides
// (pcm_lane): its F frames lie inside the row -> C 16-byte loads and 16-byte stores, and only the lane that holds
// the ragged end (hop % F frames) takes those one by one.  So the telephone hop of 4 000 one-byte frames is 250
// vector lanes per row, and the 832 frames behind the last full block of a float32 hop of 8 000 are read 16 bytes
// at a time (over PCIe when the block is mapped pinned memory).  Where they do not (a ring with hop % 4 != 0, input
// rows off the 16-byte boundary) the lanes of the block take single frames, L apart: 4-byte stores, a wave's stores
// one contiguous span.  Every path does the same arithmetic per frame; <float, 1> copies bits.
template <typename T, int C>
__global__ __launch_bounds__(256) void ring_scatter_kernel(const T* __restrict__ block, long long bstride,
                                                           float* __restrict__ buf, long long pitch, int hop, int P,
                                                           int in_vec, int uni, DzRowList rows) {
    constexpr int F = 16 / sizeof(T);
    constexpr int L = pcm_block_lanes<T>();
    const int jrow = blockIdx.y;
    // (the list is read whatever the mode, so that every kernel argument is fetched in one round trip)
    const int lrow = rows.row[jrow & 63], loff = rows.off[jrow & 63];
    const int off = uni >= 0 ? uni : loff;
    const T* in = block + (long long)jrow * bstride;
    float* row = buf + (long long)(uni >= 0 ? jrow : lrow) * pitch + off;
    const int f0 = blockIdx.x * (F * L);
    if (__builtin_expect(in_vec && ((off | P) & 3) == 0, 1)) {
        const int f = f0 + F * threadIdx.x;
        pcm_lane<T, C, true>(in + (long long)f * C, row + f, row + P + f, hop - f, true);
        return;
    }
#pragma unroll
    for (int t = 0; t < F; ++t) {
        const int f = f0 + t * L + threadIdx.x;
        if (f < hop) {
            const float o = pcm_one_frame<T, C>(in + (long long)f * C);
            row[f] = o;
            row[P + f] = o;
        }
    }
}

static long long pcm_value_bytes(int format) {
    return format == DZ_PCM_F32 || format == DZ_PCM_S32 ? 4 : format == DZ_PCM_S16 ? 2 : 1;
}

static bool pcm_format_known(int format) { return format >= DZ_PCM_F32 && format <= DZ_PCM_ALAW; }

// f(T(), integral_constant<int, C>()) for the value type of `format` and C = channels (both checked by the caller):
// the one format x channel dispatch, of the push and of dz_pcm_decode
template <typename T, typename Fn, int... I>
static void pcm_with_channels(int channels, Fn& f, std::integer_sequence<int, I...>) {
    ((channels == I + 1 ? f(T(), std::integral_constant<int, I + 1>()) : void()), ...);
}

template <typename Fn>
static void pcm_dispatch(int format, int channels, Fn f) {
    const std::make_integer_sequence<int, 8> c8;
    switch (format) {
        case DZ_PCM_F32: pcm_with_channels<float>(channels, f, c8); break;
        case DZ_PCM_S16: pcm_with_channels<short>(channels, f, c8); break;
        case DZ_PCM_U8: pcm_with_channels<pcm_u8>(channels, f, c8); break;
        case DZ_PCM_S32: pcm_with_channels<int>(channels, f, c8); break;
        case DZ_PCM_ULAW: pcm_with_channels<pcm_ulaw>(channels, f, c8); break;
        default: pcm_with_channels<pcm_alaw>(channels, f, c8); break;
    }
}

// ---------------------------------------------------------------------------
// dz_pcm_decode: the push kernel's lane (pcm_lane) over ONE contiguous device buffer, without a ring (files, tests,
// functional.decode_pcm): F frames with 16-byte loads and stores where both buffers are 16-byte aligned and the
// frames lie inside the buffer, single frames otherwise: the same bits either way.
// ---------------------------------------------------------------------------
template <typename T, int C>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const T* __restrict__ src, float* __restrict__ dst,
                                                         long long n, int vec) {
    const long long f = ((long long)blockIdx.x * 256 + threadIdx.x) * (16 / sizeof(T));
    pcm_lane<T, C, false>(src + f * C, dst + f, nullptr, n - f, vec);
}

extern "C" int dz_pcm_decode(dz_ctx* ctx, const void* d_src, long long n_frames, int format, int channels,
                             float* d_dst, void* stream) {
    DZ_REQUIRE(ctx && d_src && d_dst, "dz_pcm_decode: NULL argument");
    DZ_REQUIRE(pcm_format_known(format), "dz_pcm_decode: unknown format %d", format);
    DZ_REQUIRE(channels >= 1 && channels <= 8, "dz_pcm_decode: %d channels (1 .. 8)", channels);
    DZ_REQUIRE(n_frames >= 1 && n_frames <= (1LL << 40), "dz_pcm_decode: %lld frames", n_frames);
    const long long esz = pcm_value_bytes(format);
    DZ_REQUIRE((uintptr_t)d_src % esz == 0 && ((uintptr_t)d_dst & 3) == 0,
               "dz_pcm_decode: buffers must be aligned to one value");
    DZ_HIP(hipSetDevice(ctx->device));
    const int vec = (((uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0;
    pcm_dispatch(format, channels, [&](auto tag, auto c) {
        using T = decltype(tag);
        constexpr long long per_block = 256 * (16 / sizeof(T));
        hipLaunchKernelGGL((pcm_decode_kernel<T, decltype(c)::value>), dim3((unsigned)((n_frames + per_block - 1) / per_block)),
                           dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const T*>(d_src), d_dst, n_frames, vec);
    });
    DZ_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// A step's results -> pinned host memory with ONE kernel (stores over the host link; pinned memory is mapped at
// its own address).  Why not hipMemcpyAsync: on this runtime a device-to-host copy call now and then blocks its
// caller until everything queued on that stream has run — measured in `StreamBatch`: about once per 150 steps
// the D2H copy at the end of a step's launch sat 6 - 13 ms in the call (a whole step's latency under load; the
// segmentation copy or the embedding copy, never the kernel launches or the event calls around them), the
// host fed nothing meanwhile and the eight steps in flight drained: -3 to -7 % on a 200-step run, 8 ms of a 19 ms
// driver-form region (profiles/r06z_launch_stalls.json).  A kernel launch does not take that path.
// Replaces the two `.cpu()` of /root/reference/src/diart/blocks/segmentation.py:47 and blocks/embedding.py:68.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void results_to_host_kernel(const float* __restrict__ a, float* __restrict__ ha,
                                                              long long na, const float* __restrict__ b,
                                                              float* __restrict__ hb, long long nb) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // 16-byte piece of (a | b)
    const long long pa = (na + 3) / 4;
    const float* src = a;
    float* dst = ha;
    long long n = na;
    if (i >= pa) { i -= pa; src = b; dst = hb; n = nb; }
    if (4 * i + 3 < n) {
        reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
    } else {
        for (long long j = 4 * i; j < n; ++j) dst[j] = src[j];
    }
}

extern "C" int dz_results_to_host(dz_ctx* ctx, const float* d_a, float* h_a, long long n_a, const float* d_b,
                                  float* h_b, long long n_b, void* stream) {
    DZ_REQUIRE(ctx && d_a && h_a && n_a >= 1, "dz_results_to_host: NULL / empty first buffer");
    DZ_REQUIRE(n_b >= 0 && (n_b == 0 || (d_b && h_b)), "dz_results_to_host: NULL second buffer");
    DZ_REQUIRE((((uintptr_t)d_a | (uintptr_t)h_a | (uintptr_t)d_b | (uintptr_t)h_b) & 15) == 0,
               "dz_results_to_host: buffers must be 16-byte aligned");
    DZ_HIP(hipSetDevice(ctx->device));
    const long long pieces = (n_a + 3) / 4 + (n_b + 3) / 4;
    DZ_LAUNCH(results_to_host_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
              d_a, h_a, n_a, d_b, h_b, n_b);
    DZ_HIP(hipGetLastError());
    return 0;
}

extern "C" int dz_ring_destroy(dz_ring* r) {
    if (r) {
        if (r->buf) (void)hipFree(r->buf);
        if (r->land) (void)hipFree(r->land);
        delete r;
    }
    return 0;
}

extern "C" int dz_ring_reset(dz_ring* r) {
    DZ_REQUIRE(r, "dz_ring_reset: NULL argument");
    r->pushed = 0;
    r->pos = 0;
    r->rpos.assign(r->n, 0);
    r->rpushed.assign(r->n, 0);
    return 0;
}

extern "C" int dz_ring_reset_row(dz_ring* r, int row) {
    DZ_REQUIRE(r && row >= 0 && row < r->n, "dz_ring_reset_row: bad row");
    r->rpos[row] = 0;
    r->rpushed[row] = 0;
    return 0;
}

// The push path.  k rows of `block` (stride_bytes apart; hop frames of `channels` interleaved values of `format`
// each): row j -> ring row rows[j] at THAT row's own write position (the caller has checked `rows`), 64 rows per
// launch; or, rows == nullptr and k == n, the lock-step push: row j -> ring row j at the common position, one launch.
static int ring_push(dz_ring* r, const void* block, long long stride_bytes, int format, int channels, int on_device,
                     const int* rows, int k, hipStream_t st) {
    const long long esz = pcm_value_bytes(format);
    const long long row_bytes = (long long)r->hop * channels * esz;
    DZ_REQUIRE(stride_bytes >= row_bytes && stride_bytes % esz == 0 && (uintptr_t)block % esz == 0,
               "ring push: rows of the block must be >= hop * channels values apart and aligned to one value");
    DZ_HIP(hipSetDevice(r->ctx->device));
    const char* src = reinterpret_cast<const char*>(block);
    long long sstride = stride_bytes;
    if (on_device == 2) {
        // pinned host memory: ask the runtime for its device-side address and let the scatter kernel
        // read it in place over PCIe (32 KB per stream).  That keeps the upload off the copy queues,
        // where it was seen to wait behind the D2H copy of a step whose results were not ready yet
        // (-17 % with one embedding stream per lane).  Not mappable -> staged copy below.
        void* dptr = nullptr;
        if (hipHostGetDevicePointer(&dptr, (void*)block, 0) == hipSuccess && dptr) {
            src = reinterpret_cast<const char*>(dptr);
        } else {
            (void)hipGetLastError();
            on_device = 0;
        }
    }
    if (!on_device) {
        // landing rows start on 16-byte boundaries whatever the caller's stride.  Pushes of one ring are issued in
        // stream order, so two landing blocks used alternately are never overwritten before the scatter that reads
        // them has run.  They grow to the largest format seen (hipFree waits for the kernels still reading them)
        const long long spitch = round16(row_bytes);
        const size_t full = (size_t)r->n * spitch;
        if (r->land_cap < full) {
            DZ_HIP(hipFree(r->land));
            r->land = nullptr; r->land_cap = 0;
            DZ_HIP(hipMalloc((void**)&r->land, 2 * full));
            r->land_cap = full;
        }
        char* land = r->land + (size_t)(r->pushed & 1) * r->land_cap;
        if (stride_bytes == row_bytes && row_bytes == spitch) {
            DZ_HIP(hipMemcpyAsync(land, block, (size_t)k * row_bytes, hipMemcpyHostToDevice, st));
        } else {
            DZ_HIP(hipMemcpy2DAsync(land, (size_t)spitch, block, (size_t)stride_bytes, (size_t)row_bytes, k,
                                    hipMemcpyHostToDevice, st));
        }
        src = land;
        sstride = spitch;
    }
    const int in_vec = ((uintptr_t)src & 15) == 0 && (sstride & 15) == 0;
    const int per_launch = rows ? 64 : k;
    for (int j0 = 0; j0 < k; j0 += per_launch) {
        const int m = k - j0 < per_launch ? k - j0 : per_launch;
        DzRowList rl = {};
        for (int j = 0; rows && j < m; ++j) {
            rl.row[j] = rows[j0 + j];
            rl.off[j] = r->rpos[rows[j0 + j]];
        }
        pcm_dispatch(format, channels, [&](auto tag, auto c) {
            using T = decltype(tag);
            constexpr int L = pcm_block_lanes<T>(), per_block = L * (int)(16 / sizeof(T));
            hipLaunchKernelGGL((ring_scatter_kernel<T, decltype(c)::value>), dim3((r->hop + per_block - 1) / per_block, m),
                               dim3(L), 0, st, reinterpret_cast<const T*>(src + (long long)j0 * sstride), sstride / esz,
                               r->buf, r->pitch, r->hop, r->P, in_vec, rows ? -1 : r->pos, rl);
        });
        DZ_HIP(hipGetLastError());
    }
    if (!rows) r->pos = (r->pos + r->hop) % r->P;
    for (int j = 0; j < k; ++j) {
        const int i = rows ? rows[j] : j;
        r->rpos[i] = rows ? (r->rpos[i] + r->hop) % r->P : r->pos;
        r->rpushed[i] += 1;
    }
    r->pushed += 1;        // also alternates the landing blocks
    return 0;
}

static int ring_check_rows(const dz_ring* r, const int* rows, int k, const char* who) {
    DZ_REQUIRE(k >= 1 && k <= r->n, "%s: %d rows for %d streams", who, k, r->n);
    std::vector<char> seen(r->n, 0);
    for (int j = 0; j < k; ++j) {
        DZ_REQUIRE(rows[j] >= 0 && rows[j] < r->n && !seen[rows[j]], "%s: bad / repeated row %d", who, rows[j]);
        seen[rows[j]] = 1;
    }
    return 0;
}

extern "C" int dz_ring_push_rows_pcm(dz_ring* r, const void* block, long long block_stride_bytes, int format,
                                     int channels, int on_device, const int* rows, int k, void* stream) {
    DZ_REQUIRE(r && block && rows, "dz_ring_push_rows_pcm: NULL argument");
    DZ_REQUIRE(pcm_format_known(format), "dz_ring_push_rows_pcm: unknown format %d", format);
    DZ_REQUIRE(channels >= 1 && channels <= 8, "dz_ring_push_rows_pcm: %d channels (1 .. 8)", channels);
    int rc = ring_check_rows(r, rows, k, "dz_ring_push_rows_pcm");
    if (rc) return rc;
    return ring_push(r, block, block_stride_bytes, format, channels, on_device, rows, k, (hipStream_t)stream);
}

// block: [n][hop] floats with `block_stride` floats between rows; on the host (pinned memory makes
// the copy asynchronous) when on_device == 0, in device memory otherwise.  Every row at the common position.
extern "C" int dz_ring_push(dz_ring* r, const float* block, long long block_stride, int on_device,
                            void* stream) {
    DZ_REQUIRE(r && block, "dz_ring_push: NULL argument");
    DZ_REQUIRE(block_stride >= r->hop, "dz_ring_push: block_stride %lld < hop %d", block_stride,
               r->hop);
    DZ_REQUIRE(!r->aligned || (((uintptr_t)block & 15) == 0 && (block_stride & 3) == 0),
               "dz_ring_push: block rows must be 16-byte aligned");
    return ring_push(r, block, block_stride * (long long)sizeof(float), DZ_PCM_F32, 1, on_device, nullptr, r->n,
                     (hipStream_t)stream);
}

// One new block for each of the `k` listed streams: row j of `block` (k, hop) goes to ring row
// rows[j], at THAT row's own write position.  Rows must be distinct.
extern "C" int dz_ring_push_rows(dz_ring* r, const float* block, long long block_stride, int on_device,
                                 const int* rows, int k, void* stream) {
    DZ_REQUIRE(r && block && rows, "dz_ring_push_rows: NULL argument");
    DZ_REQUIRE(!r->aligned || (block_stride >= r->hop && ((uintptr_t)block & 15) == 0 && (block_stride & 3) == 0),
               "dz_ring_push_rows: rows of the block must be >= hop floats apart and 16-byte aligned");
    int rc = ring_check_rows(r, rows, k, "dz_ring_push_rows");
    if (rc) return rc;
    return ring_push(r, block, block_stride * (long long)sizeof(float), DZ_PCM_F32, 1, on_device, rows, k,
                     (hipStream_t)stream);
}

// samples received by one row so far, capped at the window
extern "C" int dz_ring_filled_row(const dz_ring* r, int row, int* filled) {
    DZ_REQUIRE(r && filled && row >= 0 && row < r->n, "dz_ring_filled_row: bad argument");
    const long long got = r->rpushed[row] * r->hop;
    *filled = got >= r->W ? r->W : (int)got;
    return 0;
}

// out row j <- the W samples of ring row rows.row[j] starting at rows.off[j].  A block of 256 lanes moves 1024
// samples.  Where this row's source and destination are 16-byte aligned each lane moves its 4 samples with one
// 16-byte load and store (the lane at the end of a W that is no multiple of 4: what is left, one by one); else (a ring
// with hop % 4 != 0) four 4-byte pieces per lane, 256 samples apart (every load and store of a wave is then one
// contiguous 256-byte span).
__global__ __launch_bounds__(256) void ring_gather_kernel(const float* __restrict__ buf, long long pitch,
                                                          float* __restrict__ out, long long ostride, int W,
                                                          int out_vec, DzRowList rows) {
    const int jrow = blockIdx.y;
    const int off = rows.off[jrow];
    const float* src = buf + (long long)rows.row[jrow] * pitch + off;
    float* dst = out + (long long)jrow * ostride;
    const int e0 = blockIdx.x * 1024;
    if (out_vec && (off & 3) == 0) {
        const int e = e0 + 4 * threadIdx.x;
        if (e + 4 <= W) {
            *reinterpret_cast<f32x4*>(dst + e) = *reinterpret_cast<const f32x4*>(src + e);
        } else {
            for (int g = e; g < W; ++g) dst[g] = src[g];
        }
    } else {
        for (int t = 0; t < 4; ++t) {
            const int e = e0 + t * 256 + threadIdx.x;
            if (e < W) dst[e] = src[e];
        }
    }
}

// d_out row j (out_stride floats apart) <- the current window of ring row rows[j]; every listed row
// must hold a complete window
extern "C" int dz_ring_gather(const dz_ring* r, const int* rows, int k, float* d_out, long long out_stride,
                              void* stream) {
    DZ_REQUIRE(r && rows && d_out, "dz_ring_gather: NULL argument");
    const bool out_vec = (out_stride & 3) == 0 && ((uintptr_t)d_out & 15) == 0;
    DZ_REQUIRE(k >= 1 && out_stride >= r->W && (out_vec || !r->aligned) && ((uintptr_t)d_out & 3) == 0,
               "dz_ring_gather: output rows must be >= window floats apart and 16-byte aligned (4-byte aligned "
               "for a ring whose hop is not a multiple of 4)");
    for (int j = 0; j < k; ++j) {
        DZ_REQUIRE(rows[j] >= 0 && rows[j] < r->n, "dz_ring_gather: bad row %d", rows[j]);
        DZ_REQUIRE(r->rpushed[rows[j]] * r->hop >= r->W, "dz_ring_gather: the window of row %d is not complete",
                   rows[j]);
    }
    DZ_HIP(hipSetDevice(r->ctx->device));
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int m = k - j0 < 64 ? k - j0 : 64;
        DzRowList rl;
        for (int j = 0; j < m; ++j) {
            rl.row[j] = rows[j0 + j];
            rl.off[j] = (r->rpos[rows[j0 + j]] + r->P - r->W) % r->P;
        }
        hipLaunchKernelGGL(ring_gather_kernel, dim3((r->W + 1023) / 1024, m), dim3(256), 0, (hipStream_t)stream, r->buf,
                           r->pitch, d_out + (long long)j0 * out_stride, out_stride, r->W, (int)out_vec, rl);
        DZ_HIP(hipGetLastError());
    }
    return 0;
}

// The rolling window as the forward passes take it: *d_wave + i * *stride is the window of stream
// i.  *filled = samples received so far, capped at W: the window is complete (what
// rearrange_audio_stream would emit) once *filled == W.
extern "C" int dz_ring_window(const dz_ring* r, const float** d_wave, long long* stride,
                              int* filled) {
    DZ_REQUIRE(r && d_wave && stride, "dz_ring_window: NULL argument");
    DZ_REQUIRE(r->aligned, "dz_ring_window: the windows of a ring with hop %d (not a multiple of 4 samples) do not "
               "start on 16-byte boundaries and cannot be read in place: use dz_ring_gather / dz_ring_read", r->hop);
    *d_wave = r->buf + (r->pos + r->P - r->W) % r->P;
    *stride = r->pitch;
    if (filled) {
        const long long got = r->pushed * r->hop;
        *filled = got >= r->W ? r->W : (int)got;
    }
    return 0;
}

// contiguous copy (n, W) of the current window (tests; a consumer that wants the window the way
// rearrange_audio_stream emits it).  The forward passes do not need it.
extern "C" int dz_ring_read(const dz_ring* r, float* d_out, void* stream) {
    DZ_REQUIRE(r && d_out, "dz_ring_read: NULL argument");
    DZ_HIP(hipSetDevice(r->ctx->device));
    const float* src = r->buf + (r->pos + r->P - r->W) % r->P;
    DZ_HIP(hipMemcpy2DAsync(d_out, (size_t)r->W * sizeof(float), src,
                            (size_t)r->pitch * sizeof(float), (size_t)r->W * sizeof(float), r->n,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
