// dz_gallery_*: a gallery of enrolled voiceprints on the device and the nearest-voiceprint search of embedding rows
// against it (include/diart_amd.h; kernels: k_gallery.hip; definition: DESIGN.md 4.18), raw or normalised against a
// cohort of impostors (kernels: k_cohort.hip; definition: DESIGN.md 4.20).  Host code.
#include "dz_common.h"

#include <math.h>
#include <new>
#include <vector>

namespace {
constexpr int MAX_ROWS = 4096, MAX_ENTRIES = 65536, MIN_DIM = 64, MAX_DIM = 512, MAX_COHORT = 8192;

// rows (n, D) -> each divided by its float64 norm, rounded to float32 once; -1, or the first row that is not finite
// (*finite = false) or of zero norm
int unit_rows(const float* rows, int n, int D, std::vector<float>& unit, bool* finite_out) {
    unit.resize((size_t)n * D);
    for (int e = 0; e < n; ++e) {
        const float* v = rows + (size_t)e * D;
        double ss = 0.0;
        bool finite = true;
        for (int k = 0; k < D; ++k) {
            finite = finite && isfinite(v[k]);
            ss += (double)v[k] * (double)v[k];
        }
        const double nrm = sqrt(ss);
        if (!(finite && nrm > 0.0 && isfinite(nrm))) {
            *finite_out = finite;
            return e;
        }
        for (int k = 0; k < D; ++k) unit[(size_t)e * D + k] = (float)((double)v[k] / nrm);
    }
    return -1;
}
}  // namespace

struct dz_gallery {
    int device;
    int E, D, tiles;
    float* G;          // (E, D) unit-norm voiceprints
    float* norm;       // scratch of ONE match at a time: MAX_ROWS row norms ...
    int* p_idx;        // ... and the (row, gallery tile) partial results, MAX_ROWS x tiles each
    float* p_best;
    float* p_second;
    // the cohort (dz_gallery_set_cohort), one allocation; M == 0: none
    int M, top_n;
    float* C;          // (M, D) unit-norm cohort rows
    float* c_dist;     // DZ_COHORT_PASS x dz_cohort_ld(M) distances of one pass of rows: at most 8 MiB
    float *mu_g, *sd_g, *inv_g;     // E each: the voiceprints' statistics, computed when the cohort is set
    float *mu_x, *sd_x, *inv_x;     // MAX_ROWS each: the rows' statistics of ONE normalised match
};

extern "C" int dz_gallery_create(dz_ctx* ctx, const float* voiceprints, int E, int D, dz_gallery** out) {
    DZ_REQUIRE(voiceprints && out, "dz_gallery_create: NULL argument");
    DZ_REQUIRE(E >= 1 && E <= MAX_ENTRIES, "dz_gallery_create: %d voiceprints (1 .. %d)", E, MAX_ENTRIES);
    DZ_REQUIRE(D >= MIN_DIM && D <= MAX_DIM && D % 64 == 0,
               "dz_gallery_create: dimension %d (a multiple of 64 from %d to %d)", D, MIN_DIM, MAX_DIM);
    // stored form: each voiceprint divided by its float64 norm, rounded to float32 once
    std::vector<float> unit;
    bool finite = true;
    const int bad = unit_rows(voiceprints, E, D, unit, &finite);
    DZ_REQUIRE(bad < 0, "dz_gallery_create: voiceprint %d is %s", bad, finite ? "of zero norm" : "not finite");
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
    g->M = g->top_n = 0;
    g->C = nullptr;
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
        if (g->C) (void)hipFree(g->C);
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

// ---------------------------------------------------------------------------------------------------------------
// the cohort: adaptive s-norm of the match (k_cohort.hip)

extern "C" int dz_gallery_set_cohort(dz_gallery* g, const float* rows, int M, int top_n) {
    DZ_REQUIRE(g, "dz_gallery_set_cohort: NULL handle");
    std::vector<float> unit;
    if (rows != nullptr && M != 0) {
        DZ_REQUIRE(M >= 1 && M <= MAX_COHORT, "dz_gallery_set_cohort: a cohort of %d rows (1 .. %d)", M, MAX_COHORT);
        DZ_REQUIRE(top_n >= 1 && top_n <= M, "dz_gallery_set_cohort: top_n = %d (1 .. the cohort's %d rows)", top_n, M);
        bool finite = true;
        const int bad = unit_rows(rows, M, g->D, unit, &finite);
        DZ_REQUIRE(bad < 0, "dz_gallery_set_cohort: cohort row %d is %s", bad, finite ? "of zero norm" : "not finite");
    } else {
        M = 0;                                          // NULL or no rows: the cohort is removed
    }
    DZ_HIP(hipSetDevice(g->device));
    if (g->C) {
        DZ_HIP(hipDeviceSynchronize());                 // no match of an older cohort is still running
        (void)hipFree(g->C);
    }
    g->C = nullptr;
    g->M = g->top_n = 0;
    if (M == 0) return 0;
    const size_t cfl = (size_t)M * g->D, dfl = (size_t)DZ_COHORT_PASS * dz_cohort_ld(M);
    const size_t floats = cfl + dfl + 3 * (size_t)g->E + 3 * (size_t)MAX_ROWS;
    float* base = nullptr;
    hipError_t err = hipMalloc((void**)&base, floats * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(base, unit.data(), cfl * sizeof(float), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        dz_set_error("dz_gallery_set_cohort: %zu bytes of cohort and scratch: %s", floats * sizeof(float),
                     hipGetErrorString(err));
        if (base) (void)hipFree(base);
        return 1;
    }
    g->C = base;
    g->c_dist = base + cfl;
    g->mu_g = g->c_dist + dfl;
    g->sd_g = g->mu_g + g->E;
    g->inv_g = g->sd_g + g->E;
    g->mu_x = g->inv_g + g->E;
    g->sd_x = g->mu_x + MAX_ROWS;
    g->inv_x = g->sd_x + MAX_ROWS;
    // the voiceprints' statistics, once: the stored unit voiceprints as the rows, MAX_ROWS (the norm scratch) at a time
    int rc = 0;
    for (int e0 = 0; e0 < g->E && rc == 0; e0 += MAX_ROWS) {
        const int n = g->E - e0 < MAX_ROWS ? g->E - e0 : MAX_ROWS;
        const float* X = g->G + (size_t)e0 * g->D;
        rc = dz_launch_gallery_norm(X, g->D, n, g->D, g->norm, nullptr);
        if (rc == 0)
            rc = dz_launch_cohort_stats(X, g->D, n, g->D, g->C, M, top_n, g->norm, g->c_dist, g->mu_g + e0, g->sd_g + e0,
                                        g->inv_g + e0, nullptr);
    }
    if (rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess) {
        dz_set_error("dz_gallery_set_cohort: the voiceprints' statistics failed on the device");
        rc = 1;
    }
    if (rc != 0) {
        (void)hipFree(base);
        g->C = nullptr;
        return rc;
    }
    g->M = M;
    g->top_n = top_n;
    return 0;
}

extern "C" int dz_gallery_cohort_size(dz_gallery* g) { return g ? g->M : 0; }

// the checks that dz_gallery_match makes, under another function's name
static int check_rows(const dz_gallery* g, const char* who, const void* d_rows, long long row_stride, int R,
                      const void* a, const void* b, const void* c) {
    DZ_REQUIRE(g, "%s: NULL handle", who);
    DZ_REQUIRE(d_rows && a && b && c, "%s: NULL rows or output", who);
    DZ_REQUIRE(g->M > 0, "%s: the gallery has no cohort (dz_gallery_set_cohort)", who);
    DZ_REQUIRE(R >= 1 && R <= MAX_ROWS, "%s: %d rows (1 .. %d)", who, R, MAX_ROWS);
    DZ_REQUIRE(row_stride >= g->D, "%s: row stride %lld below the dimension %d", who, row_stride, g->D);
    DZ_REQUIRE((((uintptr_t)d_rows | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0,
               "%s: rows and outputs must be aligned to one value", who);
    return 0;
}

extern "C" int dz_gallery_cohort_stats(dz_gallery* g, const float* d_rows, long long row_stride, int R, float* mean_out,
                                       float* std_out, void* stream) {
    if (int rc = check_rows(g, "dz_gallery_cohort_stats", d_rows, row_stride, R, mean_out, std_out, std_out)) return rc;
    DZ_HIP(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dz_launch_gallery_norm(d_rows, row_stride, R, g->D, g->norm, st)) return rc;
    return dz_launch_cohort_stats(d_rows, row_stride, R, g->D, g->C, g->M, g->top_n, g->norm, g->c_dist, mean_out,
                                  std_out, nullptr, st);
}

extern "C" int dz_gallery_entry_stats(dz_gallery* g, float* mean_host, float* std_host) {
    DZ_REQUIRE(g, "dz_gallery_entry_stats: NULL handle");
    DZ_REQUIRE(mean_host && std_host, "dz_gallery_entry_stats: NULL output");
    DZ_REQUIRE(g->M > 0, "dz_gallery_entry_stats: the gallery has no cohort (dz_gallery_set_cohort)");
    DZ_HIP(hipSetDevice(g->device));
    DZ_HIP(hipMemcpy(mean_host, g->mu_g, (size_t)g->E * sizeof(float), hipMemcpyDeviceToHost));
    DZ_HIP(hipMemcpy(std_host, g->sd_g, (size_t)g->E * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dz_gallery_match_norm(dz_gallery* g, const float* d_rows, long long row_stride, int R, int* index_out,
                                     float* dist_out, float* second_out, void* stream) {
    if (int rc = check_rows(g, "dz_gallery_match_norm", d_rows, row_stride, R, index_out, dist_out, second_out)) return rc;
    DZ_HIP(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dz_launch_gallery_norm(d_rows, row_stride, R, g->D, g->norm, st)) return rc;
    if (int rc = dz_launch_cohort_stats(d_rows, row_stride, R, g->D, g->C, g->M, g->top_n, g->norm, g->c_dist, g->mu_x,
                                        g->sd_x, g->inv_x, st))
        return rc;
    if (int rc = dz_launch_gallery_tile_norm(d_rows, row_stride, R, g->D, g->G, g->E, g->norm, g->mu_g, g->inv_g,
                                             g->mu_x, g->inv_x, g->p_idx, g->p_best, g->p_second, st))
        return rc;
    return dz_launch_gallery_reduce(g->norm, R, g->E, g->p_idx, g->p_best, g->p_second, index_out, dist_out,
                                    second_out, st);
}
