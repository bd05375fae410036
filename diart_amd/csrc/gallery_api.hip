// dz_gallery_*: a gallery of enrolled voiceprints on the device and the nearest-voiceprint search of embedding rows
// against it (include/diart_amd.h; kernels: k_gallery.hip; definition: DESIGN.md 4.18).  Host code.
#include "dz_common.h"

#include <math.h>
#include <new>
#include <vector>

namespace {
constexpr int MAX_ROWS = 4096, MAX_ENTRIES = 65536, MIN_DIM = 64, MAX_DIM = 512;
}

struct dz_gallery {
    int device;
    int E, D, tiles;
    float* G;          // (E, D) unit-norm voiceprints
    float* norm;       // scratch of ONE match at a time: MAX_ROWS row norms ...
    int* p_idx;        // ... and the (row, gallery tile) partial results, MAX_ROWS x tiles each
    float* p_best;
    float* p_second;
};

extern "C" int dz_gallery_create(dz_ctx* ctx, const float* voiceprints, int E, int D, dz_gallery** out) {
    DZ_REQUIRE(voiceprints && out, "dz_gallery_create: NULL argument");
    DZ_REQUIRE(E >= 1 && E <= MAX_ENTRIES, "dz_gallery_create: %d voiceprints (1 .. %d)", E, MAX_ENTRIES);
    DZ_REQUIRE(D >= MIN_DIM && D <= MAX_DIM && D % 64 == 0,
               "dz_gallery_create: dimension %d (a multiple of 64 from %d to %d)", D, MIN_DIM, MAX_DIM);
    // stored form: each voiceprint divided by its float64 norm, rounded to float32 once
    std::vector<float> unit((size_t)E * D);
    for (int e = 0; e < E; ++e) {
        const float* v = voiceprints + (size_t)e * D;
        double ss = 0.0;
        bool finite = true;
        for (int k = 0; k < D; ++k) {
            finite = finite && isfinite(v[k]);
            ss += (double)v[k] * (double)v[k];
        }
        const double n = sqrt(ss);
        DZ_REQUIRE(finite && n > 0.0 && isfinite(n), "dz_gallery_create: voiceprint %d is %s", e,
                   finite ? "of zero norm" : "not finite");
        for (int k = 0; k < D; ++k) unit[(size_t)e * D + k] = (float)((double)v[k] / n);
    }
    DZ_REQUIRE(ctx, "dz_gallery_create: NULL context");
    DZ_HIP(hipSetDevice(ctx->device));
    dz_gallery* g = new (std::nothrow) dz_gallery;
    DZ_REQUIRE(g != nullptr, "dz_gallery_create: out of memory");
    g->device = ctx->device;
    g->E = E;
    g->D = D;
    g->tiles = dz_gallery_tiles(E);
    g->G = nullptr;
    g->norm = nullptr;
    const size_t gbytes = unit.size() * sizeof(float), part = (size_t)MAX_ROWS * g->tiles * 4;
    char* scratch = nullptr;
    hipError_t err = hipMalloc((void**)&g->G, gbytes);
    if (err == hipSuccess) err = hipMemcpy(g->G, unit.data(), gbytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc((void**)&scratch, MAX_ROWS * 4 + 3 * part);
    if (err != hipSuccess) {
        dz_set_error("dz_gallery_create: %zu-byte gallery + %zu bytes of scratch: %s", gbytes, MAX_ROWS * 4 + 3 * part,
                     hipGetErrorString(err));
        if (g->G) (void)hipFree(g->G);
        delete g;
        return 1;
    }
    g->norm = reinterpret_cast<float*>(scratch);
    g->p_idx = reinterpret_cast<int*>(scratch + MAX_ROWS * 4);
    g->p_best = reinterpret_cast<float*>(scratch + MAX_ROWS * 4 + part);
    g->p_second = reinterpret_cast<float*>(scratch + MAX_ROWS * 4 + 2 * part);
    *out = g;
    return 0;
}

extern "C" int dz_gallery_destroy(dz_gallery* g) {
    if (g) {
        (void)hipSetDevice(g->device);
        if (g->G) (void)hipFree(g->G);
        if (g->norm) (void)hipFree(g->norm);
        delete g;
    }
    return 0;
}

extern "C" int dz_gallery_size(dz_gallery* g) { return g ? g->E : 0; }
extern "C" int dz_gallery_dim(dz_gallery* g) { return g ? g->D : 0; }

extern "C" int dz_gallery_match(dz_gallery* g, const float* d_rows, long long row_stride, int R, int* index_out,
                                float* dist_out, float* second_out, void* stream) {
    DZ_REQUIRE(g, "dz_gallery_match: NULL handle");
    DZ_REQUIRE(d_rows && index_out && dist_out && second_out, "dz_gallery_match: NULL rows or output");
    DZ_REQUIRE(R >= 1 && R <= MAX_ROWS, "dz_gallery_match: %d rows (1 .. %d)", R, MAX_ROWS);
    DZ_REQUIRE(row_stride >= g->D, "dz_gallery_match: row stride %lld below the dimension %d", row_stride, g->D);
    DZ_REQUIRE((((uintptr_t)d_rows | (uintptr_t)index_out | (uintptr_t)dist_out | (uintptr_t)second_out) & 3) == 0,
               "dz_gallery_match: rows and outputs must be aligned to one value");
    DZ_HIP(hipSetDevice(g->device));
    return dz_launch_gallery_match(d_rows, row_stride, R, g->D, g->G, g->E, g->norm, g->p_idx, g->p_best, g->p_second,
                                   index_out, dist_out, second_out, (hipStream_t)stream);
}
