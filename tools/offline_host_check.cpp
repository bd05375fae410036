// A stand-alone check of the whole-file mode's host entry points for sanitizer builds:
// dz_agglo_linkage_host over three files (one with duplicate rows, one of a single row) on two threads, dz_agglo_cut,
// dz_offline_assign and dz_offline_reconstruct on what it returns, and the refusals.  No GPU, no Python.  Build it with
// the host sources it needs, for example
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Idiart_amd/csrc \
//       tools/offline_host_check.cpp diart_amd/csrc/agglo.cpp diart_amd/csrc/hostpool.cpp -lpthread -o offline_host_check
//
// and run it: it returns 0 when every check holds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/diart_amd.h"

// the library's error text lives in api.hip, which needs the HIP runtime: this program brings its own
static thread_local char g_err[512];
void dz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" const char* dz_last_error(void) { return g_err; }

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s failed (%s)\n", __LINE__, #cond, g_err); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    const int D = 24, counts[3] = {37, 1, 90};
    const int rows_off[4] = {0, 37, 38, 128};
    std::mt19937 rng(7);
    std::normal_distribution<double> gauss;
    std::vector<double> x((size_t)128 * D);
    for (int r = 0; r < 128; ++r) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
            x[(size_t)r * D + k] = gauss(rng) + (k == r % 3 ? 4.0 : 0.0);       // three voices
            s += x[(size_t)r * D + k] * x[(size_t)r * D + k];
        }
        for (int k = 0; k < D; ++k) x[(size_t)r * D + k] /= std::sqrt(s);
    }
    for (int k = 0; k < D; ++k) x[(size_t)5 * D + k] = x[(size_t)9 * D + k] = x[(size_t)2 * D + k];     // duplicates
    std::vector<double> Z((size_t)(36 + 0 + 89) * 4);
    int status[3] = {0, 0, 0};
    CHECK(dz_agglo_linkage_host(3, rows_off, x.data(), D, Z.data(), status, 2) == 0);
    CHECK(status[0] == -1 && status[1] == -1 && status[2] == -1);
    CHECK(Z[2] == 0.0 && Z[4 + 2] == 0.0 && Z[8 + 2] > 0.0);
    const double* Zf[3] = {Z.data(), Z.data() + 36 * 4, Z.data() + 36 * 4};
    for (int f = 0; f < 3; ++f) {
        const int n = counts[f];
        std::vector<int> labels(n), train(n), assign(n);
        int G = 0;
        CHECK(dz_agglo_cut(Zf[f], n, 0.9, 3, 4, labels.data(), &G) == 0);
        CHECK(G >= 1 && G <= 4);
        for (int r = 0; r < n; ++r) train[r] = r;
        std::vector<double> centroids((size_t)G * D);
        CHECK(dz_offline_assign(x.data() + (size_t)rows_off[f] * D, n, D, train.data(), labels.data(), n, G, assign.data(),
                                centroids.data()) == 0);
        for (int r = 0; r < n; ++r) CHECK(assign[r] >= 0 && assign[r] < G && (labels[r] < 0 || labels[r] == assign[r]));
        std::printf("file %d: %d rows, %d clusters kept\n", f, n, G);
    }
    CHECK(dz_agglo_cut(Z.data(), 37, NAN, 1, 4, nullptr, nullptr) == 2);
    int G = 0, one = 0;
    CHECK(dz_agglo_cut(nullptr, 1, 0.5, 12, 4, &one, &G) == 0 && G == 1 && one == 0);
    CHECK(dz_agglo_cut(nullptr, 0, 0.5, 12, 4, nullptr, &G) == 0 && G == 0);
    // reconstruction: 2 files, 6 and 1 chunks of 10 frames and 2 local speakers, 3 output frames per step
    const int F = 10, K = 2, chunks[2] = {6, 1}, kept[2] = {2, 0}, frames[2] = {5 * 3 + F, F};
    std::vector<float> seg0((size_t)6 * F * K), seg1((size_t)F * K, 0.1f);
    for (size_t e = 0; e < seg0.size(); ++e) seg0[e] = (float)((rng() % 100) / 100.0);
    for (int e = 0; e < F * K; ++e) seg0[(size_t)2 * F * K + e] = NAN;                  // an invalid chunk
    const int assign0[12] = {0, 1, 1, 0, -1, -1, 0, 0, 1, -1, 0, 1}, assign1[2] = {-1, -1};
    const int offset0[6] = {0, 3, 6, 9, 12, 15}, offset1[1] = {0};
    std::vector<unsigned char> act0((size_t)frames[0] * 2, 7);
    const float* segs[2] = {seg0.data(), seg1.data()};
    const int* assigns[2] = {assign0, assign1};
    const int* offsets[2] = {offset0, offset1};
    unsigned char* acts[2] = {act0.data(), nullptr};
    CHECK(dz_offline_reconstruct(2, segs, assigns, offsets, chunks, F, K, kept, 0.5, frames, acts, 2) == 0);
    for (unsigned char v : act0) CHECK(v <= 1);
    const int bad_offset[6] = {0, 3, 6, 9, 12, 16};
    offsets[0] = bad_offset;
    CHECK(dz_offline_reconstruct(2, segs, assigns, offsets, chunks, F, K, kept, 0.5, frames, acts, 2) == 2);
    std::printf("offline_host_check ok\n");
    return 0;
}
