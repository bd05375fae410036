// What the output tail of one step costs on the host: a loop over dz_tail_step_batch alone, no GPU.
// 64 streams, 293 frames, 20 global speakers (three of them with runs of activity), step 0.5 s, latency 5 s, Hamming
// aggregation with "loose" cropping: the shipped shape.  Built from two host files, so that two trees can be timed
// in turn:
//   g++ -O3 -std=c++17 tools/tail_step_bench.cpp diart_amd/csrc/tail.cpp diart_amd/csrc/hostpool.cpp -o tail_step_bench -lpthread
//   ./tail_step_bench <threads> <steps>
// Prints microseconds per step and a check value (the same for two trees that compute the same).
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/diart_amd.h"

static thread_local char g_err[512];
void dz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* dz_last_error(void) { return g_err; }

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 1, steps = argc > 2 ? atoi(argv[2]) : 3000;
    const int N = 64, F = 293, G = 20, max_turns = G * ((F + 2) / 2 + 1);
    std::vector<double> ham(F);
    for (int i = 0; i < F; ++i) ham[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * i / (F - 1));
    std::vector<dz_tail*> tails(N);
    for (int i = 0; i < N; ++i)
        if (dz_tail_create(F, G, 0.5, 5.0, 0.5, DZ_AGG_HAMMING, DZ_CROP_LOOSE, ham.data(), &tails[i])) return 2;
    std::mt19937 rng(1);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    // a few score sets, cycled: three "speakers" with runs of activity, the others silent
    const int sets = 4;
    std::vector<std::vector<double>> scores(sets, std::vector<double>((size_t)N * F * G, 0.0));
    for (auto& s : scores)
        for (int i = 0; i < N; ++i)
            for (int f = 0; f < F; ++f)
                for (int g = 0; g < 3; ++g) s[((size_t)i * F + f) * G + g] = ((f / 40 + g + i) % 3 == 0) ? 0.6 + 0.4 * u(rng) : 0.3 * u(rng);
    std::vector<double> start(N), res(N, 5.0 / F), agg((size_t)N * (F + 2) * G), t0(N), rout(N), turns((size_t)N * max_turns * 3);
    std::vector<int> rows(N), nturns(N);
    double check = 0.0;
    const auto a = std::chrono::steady_clock::now();
    for (int t = 0; t < steps; ++t) {
        for (int i = 0; i < N; ++i) start[i] = 0.5 * t;
        if (dz_tail_step_batch(tails.data(), N, scores[t % sets].data(), start.data(), res.data(), agg.data(), rows.data(), t0.data(),
                               rout.data(), turns.data(), max_turns, nturns.data(), threads)) {
            fprintf(stderr, "failed: %s\n", g_err);
            return 3;
        }
        check += agg[(size_t)(t % N) * (F + 2) * G + 1] + nturns[t % N];
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count() / steps;
    printf("%.1f us/step threads %d (check %.6f)\n", us, threads, check);
    return 0;
}
