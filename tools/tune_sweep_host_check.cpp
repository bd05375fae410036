// A stand-alone check of the sweep's host entry points for sanitizer builds: dz_tune_name_host and
// dz_tune_ident_score_core at several points on a seeded case, each against the loop of its own points = 1 calls, and
// the components against dz_tune_ident_score, the sequential text, within 1e-9 x the pair's total.
// No GPU, no Python.  Build it with the host sources it needs, for example
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Idiart_amd/csrc \
//       tools/tune_sweep_host_check.cpp diart_amd/csrc/tune_score.cpp diart_amd/csrc/cluster.cpp \
//       diart_amd/csrc/tail.cpp diart_amd/csrc/hostpool.cpp -lpthread -o tune_sweep_host_check
//
// and run it: it prints what it compared and returns 0 when every comparison holds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
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

int main() {
    // two files of 7 and 1 steps, R rows each on a grid of 0.1 s cells; 3 local and 5 global speakers; 4 voiceprints;
    // 3 trials (a chain of trial 1 stops at its step 4); 2 planes x 3 thresholds
    const int N = 2, K = 3, G = 5, V = 4, T = 3, P = 2, Q = 3, J = P * Q, R = 4, lanes = 256, blocks = 2;
    const int chunk_off[N + 1] = {0, 7, 8};
    const int total = chunk_off[N], rows = total * R;
    std::mt19937 rng(20260);
    auto draw = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    std::vector<signed char> assign((size_t)T * total * K);
    for (auto& a : assign) a = (signed char)draw(-1, G - 1);
    std::vector<int> status((size_t)T * N, -1);
    status[1 * N + 0] = 4;
    std::vector<int> index((size_t)P * total * K);
    std::vector<float> dist((size_t)P * total * K);
    for (size_t i = 0; i < index.size(); ++i) {
        index[i] = draw(-1, V - 1);
        dist[i] = index[i] < 0 ? NAN : (float)(draw(-120, 20) / 10.0);
    }
    std::vector<signed char> vp_ref((size_t)N * V);
    for (auto& b : vp_ref) b = (signed char)draw(-1, 2);
    const double thresholds[Q] = {-13.0, -3.0, 0.5};
    std::vector<double> thr((size_t)T * J);
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < J; ++j) thr[(size_t)t * J + j] = thresholds[j % Q];

    // ---- the names
    const size_t plane = (size_t)total * G;
    std::vector<signed char> ident((size_t)T * J * plane, 99), ident1((size_t)T * plane);
    std::vector<int> hold((size_t)T * J * plane, 99), hold1((size_t)T * plane);
    if (dz_tune_name_host(T, J, P, N, total, K, G, V, chunk_off, assign.data(), status.data(), index.data(), dist.data(),
                          vp_ref.data(), thr.data(), ident.data(), hold.data(), 3)) {
        std::printf("dz_tune_name_host at %d points failed: %s\n", J, dz_last_error());
        return 1;
    }
    int named = 0;
    for (int j = 0; j < J; ++j) {
        std::vector<double> d1(T, thresholds[j % Q]);
        const size_t off = (size_t)(j / Q) * total * K;
        if (dz_tune_name_host(T, 1, 1, N, total, K, G, V, chunk_off, assign.data(), status.data(), index.data() + off,
                              dist.data() + off, vp_ref.data(), d1.data(), ident1.data(), hold1.data(), 1)) {
            std::printf("dz_tune_name_host at one point failed: %s\n", dz_last_error());
            return 1;
        }
        for (int t = 0; t < T; ++t)
            for (size_t i = 0; i < plane; ++i) {
                const size_t s = ((size_t)t * J + j) * plane + i;
                if (ident[s] != ident1[t * plane + i] || hold[s] != hold1[t * plane + i]) {
                    std::printf("names differ at trial %d point %d slot %zu\n", t, j, i);
                    return 1;
                }
                named += hold[s] >= 0;
            }
    }

    // ---- the score: steps that follow each other, cell i of a file is [0.1 i, 0.1 (i + 1))
    std::vector<int> row_off(total + 1), step_rows(total, R), mid_cell, file_cell_off(N + 1, 0), cell_step;
    std::vector<double> mids, cell_dur;
    std::vector<unsigned long long> cell_ref;
    for (int c = 0; c <= total; ++c) row_off[c] = c * R;
    for (int n = 0; n < N; ++n) {
        for (int c = chunk_off[n]; c < chunk_off[n + 1]; ++c)
            for (int i = 0; i <= R; ++i) {
                const int cell = (c - chunk_off[n]) * R + i;
                mids.push_back(0.1 * cell);
                mid_cell.push_back(cell);
            }
        const int ncell = (chunk_off[n + 1] - chunk_off[n]) * R;
        file_cell_off[n + 1] = file_cell_off[n] + ncell;
        for (int i = 0; i < ncell; ++i) {
            cell_dur.push_back(0.1);
            cell_ref.push_back((unsigned long long)draw(0, 7));
            cell_step.push_back(chunk_off[n] + i / R);
        }
    }
    const int max_cells = 7 * R;
    std::vector<unsigned> bits((size_t)T * rows);
    for (auto& b : bits) b = (unsigned)draw(0, 31) & (unsigned)draw(0, 31);
    std::vector<double> out((size_t)T * J * N * 5, -1.0), out1((size_t)T * N * 5), seq((size_t)T * N * 5);
    const int file_row_off[N + 1] = {0, chunk_off[1] * R, rows};
    dz_tune_cells cells = {};   // (the track tuners' prefix sums stay NULL: nothing here reads them)
    cells.file_chunk_off = chunk_off;
    cells.file_row_off = file_row_off;
    cells.row_off = row_off.data();
    cells.step_rows = step_rows.data();
    cells.mids = mids.data();
    cells.mid_cell = mid_cell.data();
    cells.file_cell_off = file_cell_off.data();
    cells.cell_dur = cell_dur.data();
    cells.cell_ref = cell_ref.data();
    cells.cell_step = cell_step.data();
    cells.n_files = N, cells.total_rows = rows, cells.total_chunks = total, cells.max_cells = max_cells;
    cells.max_speakers = G, cells.collar = 0.15;
    if (dz_tune_ident_score_core(&cells, T, J, bits.data(), ident.data(), lanes, blocks, out.data(), 2)) {
        std::printf("dz_tune_ident_score_core at %d points failed: %s\n", J, dz_last_error());
        return 1;
    }
    double correct = 0.0;
    for (int j = 0; j < J; ++j) {
        for (int t = 0; t < T; ++t)
            std::memcpy(ident1.data() + t * plane, ident.data() + ((size_t)t * J + j) * plane, plane);
        if (dz_tune_ident_score_core(&cells, T, 1, bits.data(), ident1.data(), lanes, blocks, out1.data(), 1) ||
            dz_tune_ident_score(&cells, T, bits.data(), ident1.data(), seq.data(), 2)) {
            std::printf("dz_tune_ident_score_core at one point or dz_tune_ident_score failed: %s\n", dz_last_error());
            return 1;
        }
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < N * 5; ++i) {
                const double a = out[((size_t)t * J + j) * N * 5 + i], b = out1[(size_t)t * N * 5 + i];
                if (std::memcmp(&a, &b, sizeof a)) {
                    std::printf("components differ at trial %d point %d entry %d: %.17g, %.17g\n", t, j, i, a, b);
                    return 1;
                }
                const double total_s = seq[(size_t)t * N * 5 + i / 5 * 5], c = seq[(size_t)t * N * 5 + i];
                if (!(std::fabs(a - c) <= 1e-9 * (total_s > 1.0 ? total_s : 1.0))) {
                    std::printf("the sequential text differs at trial %d point %d entry %d: %.17g, %.17g\n", t, j, i, a, c);
                    return 1;
                }
                if (i % 5 == 1) correct += a;
            }
    }
    // ---- the refusals touch nothing
    const int refused = dz_tune_name_host(T, 257, P, N, total, K, G, V, chunk_off, assign.data(), status.data(), index.data(),
                                          dist.data(), vp_ref.data(), thr.data(), ident.data(), nullptr, 1) +
                        dz_tune_name_host(T, J, 4, N, total, K, G, V, chunk_off, assign.data(), status.data(), index.data(),
                                          dist.data(), vp_ref.data(), thr.data(), ident.data(), nullptr, 1) +
                        dz_tune_ident_score_core(&cells, T, 0, bits.data(), ident.data(), lanes, blocks, out.data(), 1);
    if (refused != 6 || named == 0 || !(correct > 0.0)) {
        std::printf("refusals %d (6 expected), %d named slots, correct %.3f s\n", refused, named, correct);
        return 1;
    }
    std::printf("%d trials x %d points: names and components of the sweep equal the one-point calls' (%d named slots, "
                "%.1f s correct); 3 refusals\n", T, J, named, correct);
    return 0;
}
