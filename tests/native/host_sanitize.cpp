// Sanitizer harness for the host half of the path (csrc/cluster.cpp, tail.cpp, hostpool.cpp, filebatch.cpp): the fp64
// OnlineSpeakerClustering, DelayedAggregation + Binarize and the worker pool that runs them for N streams.  Built by
// tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined and with -fsanitize=thread (the GPU build cannot
// carry sanitizers on this pool) and run on random inputs — NaN embeddings, silent chunks, more local speakers than free
// centroids, varying thread counts, two callers at once.  It checks only what must hold whatever the data (finite
// scores, assignments in range, batch == one-by-one, the tuner's plan (csrc/tune_score.cpp dz_tune_plan, built with
// them) == the rows and the output grid dz_tail_step returned, the track tuners' host entry points on 1, 3 and 256
// lanes); the reference's results are pinned by
// tests/test_clustering.py and tests/test_tail.py.  Exit code 0 = nothing reported.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../../include/diart_amd.h"

// the two symbols the HIP translation units provide in the product library
static thread_local char g_err[512];
void dz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* dz_last_error(void) { return g_err; }

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "host_sanitize: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            exit(3);                                                                  \
        }                                                                             \
    } while (0)

constexpr int F = 293, K = 3, D = 64, G = 20;
namespace {

struct Streams {
    int n;
    std::vector<dz_clu*> clu;
    std::vector<dz_tail*> tail;
    explicit Streams(int n_, int g = G) : n(n_), clu(n_), tail(n_) {
        std::vector<double> ham(F);
        for (int i = 0; i < F; ++i) ham[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * i / (F - 1));
        for (int i = 0; i < n; ++i) {
            CHECK(dz_clu_create(0.5, 0.3, 1.0, g, &clu[i]) == 0);
            CHECK(dz_tail_create(F, g, 0.5, 2.5, 0.5, DZ_AGG_HAMMING, DZ_CROP_LOOSE, ham.data(), &tail[i]) == 0);
        }
    }
    ~Streams() {
        for (int i = 0; i < n; ++i) {
            dz_clu_destroy(clu[i]);
            dz_tail_destroy(tail[i]);
        }
    }
};

void fill(std::mt19937& rng, int n, int step, std::vector<float>& seg, std::vector<float>& emb, int K = ::K, int G = ::G) {
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::normal_distribution<float> g(0.f, 1.f);
    seg.resize((size_t)n * F * K);
    emb.resize((size_t)n * K * D);
    for (int i = 0; i < n; ++i) {
        const int kind = (int)(rng() % 8);               // 0: silent chunk, 1: a NaN embedding, else speech
        for (int f = 0; f < F; ++f)
            for (int k = 0; k < K; ++k) {
                float v = u(rng);
                if (kind == 0) v *= 0.05f;
                else if ((f / 40 + k + step) % 3 == 0) v = 0.6f + 0.4f * v;      // active runs
                seg[((size_t)i * F + f) * K + k] = v;
            }
        for (int k = 0; k < K; ++k) {
            const int spk = (int)(rng() % (G + 10));     // ten identities more than centroids
            for (int d = 0; d < D; ++d)
                emb[((size_t)i * K + k) * D + d] = std::sin(0.37f * (float)(spk + 1) * (float)(d + 1)) + 0.05f * g(rng);
        }
        if (kind == 1) emb[((size_t)i * K + 1) * D + 7] = NAN;
    }
}

// K, G: beyond 8 local and 32 global speakers only the heap-backed store of the decision core runs
void run_streams(unsigned seed, int n, int steps, int threads, int K = ::K, int G = ::G) {
    std::mt19937 rng(seed);
    const int max_turns = 64 * G;
    Streams s(n, G), one(n, G);
    std::vector<float> seg, emb;
    std::vector<double> scores((size_t)n * F * G), scores1((size_t)F * G), agg((size_t)n * (F + 2) * G), turns((size_t)n * max_turns * 3);
    std::vector<double> start(n), res(n, 5.0 / F), t0(n), rout(n);
    std::vector<int> assign((size_t)n * K), assign1(K), rows(n), nturns(n);
    // what dz_tail_step returned at every step of a stream since it (re)started, against the tuner's plan of the same
    // starts: the two callers of the shared step geometry (csrc/tail_core.h) must agree
    struct Chain {
        std::vector<double> start, res, t0, rout;
        std::vector<int> rows;
    };
    std::vector<Chain> chain(n);
    auto check_plan = [&](Chain& c) {
        const int chunks = (int)c.start.size(), nwin = 5;   // Streams: latency 2.5 / step 0.5
        if (!chunks) return;
        std::vector<int> plan((size_t)chunks * (4 + nwin));
        std::vector<double> pt0(chunks), pres(chunks);
        CHECK(dz_tune_plan(chunks, F, 0.5, 2.5, c.start.data(), c.res.data(), plan.data(), pt0.data(), pres.data()) == 0);
        for (int s = 0; s < chunks; ++s) {
            const int* p = &plan[(size_t)s * (4 + nwin)];
            CHECK(p[0] + p[1] == c.rows[s] && pt0[s] == c.t0[s] && pres[s] == c.rout[s]);
            CHECK(p[3] == (s + 1 < nwin ? s + 1 : nwin));
        }
        c = Chain();
    };
    for (int t = 0; t < steps; ++t) {
        fill(rng, n, t, seg, emb, K, G);
        CHECK(dz_clu_step_batch(s.clu.data(), n, seg.data(), F, K, emb.data(), D, scores.data(), assign.data(), threads) == 0);
        for (int i = 0; i < n; ++i) {                    // the batch on the pool == one stream at a time on this thread
            CHECK(dz_clu_step(one.clu[i], &seg[(size_t)i * F * K], F, K, &emb[(size_t)i * K * D], D, scores1.data(), assign1.data()) == 0);
            CHECK(memcmp(scores1.data(), &scores[(size_t)i * F * G], sizeof(double) * F * G) == 0);
            CHECK(memcmp(assign1.data(), &assign[(size_t)i * K], sizeof(int) * K) == 0);
            for (int k = 0; k < K; ++k) CHECK(assign[(size_t)i * K + k] >= -1 && assign[(size_t)i * K + k] < G);
            start[i] = 0.5 * t;
        }
        for (double v : scores) CHECK(std::isfinite(v));
        CHECK(dz_tail_step_batch(s.tail.data(), n, scores.data(), start.data(), res.data(), agg.data(), rows.data(), t0.data(),
                                 rout.data(), turns.data(), max_turns, nturns.data(), threads) == 0);
        for (int i = 0; i < n; ++i) {
            CHECK(rows[i] >= 0 && rows[i] <= F + 2 && nturns[i] >= 0 && nturns[i] <= max_turns);
            Chain& c = chain[i];
            c.start.push_back(start[i]); c.res.push_back(res[i]); c.t0.push_back(t0[i]); c.rout.push_back(rout[i]);
            c.rows.push_back(rows[i]);
        }
        if (t % 17 == 16) {                              // a stream that ends and starts again
            CHECK(dz_clu_reset(s.clu[t % n]) == 0 && dz_clu_reset(one.clu[t % n]) == 0);
            CHECK(dz_tail_reset(s.tail[t % n]) == 0);
            check_plan(chain[t % n]);
        }
    }
    for (Chain& c : chain) check_plan(c);
    std::vector<double> centers((size_t)G * D);
    std::vector<int> mask(G);
    for (int i = 0; i < n; ++i) {
        const int rc = dz_clu_get_centers(s.clu[i], centers.data(), D);
        CHECK(rc == 0 || rc == 1);
        CHECK(dz_clu_get_active(s.clu[i], mask.data()) == 0);
    }
}

void run_files(unsigned seed, int files, int steps, int threads) {
    std::mt19937 rng(seed);
    Streams s(files);
    const int per = 4, rows = files * per;
    std::vector<float> seg, emb;
    std::vector<int> row0(files), count(files), nturns(rows), assign((size_t)rows * K);
    std::vector<double> start(rows), turns((size_t)rows * 256 * 3);
    for (int t = 0; t < steps; ++t) {
        fill(rng, rows, t, seg, emb);
        for (int i = 0; i < files; ++i) {
            row0[i] = i * per;
            count[i] = 1 + (int)(rng() % per);
            for (int j = 0; j < per; ++j) start[(size_t)i * per + j] = 0.5 * (t * per + j);
        }
        CHECK(dz_file_step_batch(s.clu.data(), s.tail.data(), files, row0.data(), count.data(), seg.data(), F, K, emb.data(), D, G,
                                 start.data(), 5.0 / F, turns.data(), 256, nturns.data(), assign.data(), threads) == 0);
    }
}

// The track tuners' host entry points (csrc/tune_score.cpp: one implementation under two row rules): files of 7 and 2
// steps on 1, 3 and 256 lanes — fewer lanes than steps, and more — with and without the masks and the components.
// Whatever the lanes: masks of 0 / 1, finite components, and (T, 2) taus with equal columns give what (T,) taus give.
void run_track(unsigned seed, int threads) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    constexpr int Ft = 16, nwin = 5, N = 2, T = 3, ncell = 40;
    const int chunk_off[N + 1] = {0, 7, 9}, chunks = chunk_off[N];
    std::vector<float> seg((size_t)chunks * Ft);
    for (float& v : seg) v = u(rng);
    seg[3 * Ft + 5] = NAN;
    std::vector<double> ham(Ft), start(chunks), res(chunks, 5.0 / Ft), t0(chunks), rout(chunks);
    for (int i = 0; i < Ft; ++i) ham[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * i / (Ft - 1));
    std::vector<int> plan((size_t)chunks * (4 + nwin)), row_off(chunks + 1, 0), row_chunk;
    for (int n = 0; n < N; ++n) {
        const int c0 = chunk_off[n], count = chunk_off[n + 1] - c0;
        for (int c = 0; c < count; ++c) start[c0 + c] = 0.5 * c;
        CHECK(dz_tune_plan(count, Ft, 0.5, 2.5, &start[c0], &res[c0], &plan[(size_t)c0 * (4 + nwin)], &t0[c0], &rout[c0]) == 0);
    }
    for (int c = 0; c < chunks; ++c) {
        const int rows = plan[(size_t)c * (4 + nwin)] + plan[(size_t)c * (4 + nwin) + 1];
        row_off[c + 1] = row_off[c] + rows;
        row_chunk.insert(row_chunk.end(), rows, c);
    }
    const int total_rows = row_off[chunks];
    // rows + 1 frame middles per step and the scoring cell each lies in: cells of 0.25 s, the reference on in every third
    std::vector<double> mids((size_t)total_rows + chunks), dur_prefix(N * (ncell + 1)), ref_prefix(N * (ncell + 1));
    std::vector<int> mid_cell(mids.size()), file_cell_off = {0, ncell, 2 * ncell};
    for (int c = 0; c < chunks; ++c)
        for (int i = 0; i <= row_off[c + 1] - row_off[c]; ++i) {
            const double m = t0[c] + (i + 0.5) * rout[c];
            mids[(size_t)row_off[c] + c + i] = m;
            mid_cell[(size_t)row_off[c] + c + i] = m < 0.0 ? 0 : (m / 0.25 > ncell ? ncell : (int)(m / 0.25));
        }
    for (int n = 0; n < N; ++n)
        for (int i = 0; i <= ncell; ++i) {
            dur_prefix[(size_t)n * (ncell + 1) + i] = 0.25 * i;
            ref_prefix[(size_t)n * (ncell + 1) + i] = 0.25 * ((i + 2) / 3);
        }
    dz_tune_desc d = {};
    d.seg = seg.data();
    d.chunk_off = chunk_off;
    d.plan = plan.data();
    d.row_off = row_off.data();
    d.row_chunk = row_chunk.data();
    d.hamming = ham.data();
    d.N = N, d.F = Ft, d.K = d.D = d.G = 1, d.nwin = nwin, d.total_chunks = chunks, d.total_rows = total_rows;
    const double taus[T] = {0.3, 0.5, 0.8};
    double pairs[T][2];
    for (int t = 0; t < T; ++t) pairs[t][0] = pairs[t][1] = taus[t];
    std::vector<double> agg(total_rows), agg2(total_rows), out((size_t)T * N * 5), out2(out.size());
    std::vector<unsigned> bits((size_t)T * total_rows), bits2(bits.size());
    dz_tune_cells cells = {};   // what the track entry reads; the rest stays NULL
    cells.mids = mids.data();
    cells.mid_cell = mid_cell.data();
    cells.file_cell_off = file_cell_off.data();
    cells.dur_prefix = dur_prefix.data();
    cells.ref_prefix = ref_prefix.data();
    cells.collar = 0.05;
    for (int lanes : {1, 3, 256}) {
        CHECK(dz_tune_vad_host(&d, &cells, 1, taus, T, agg.data(), bits.data(), lanes, out.data(), threads) == 0);
        CHECK(dz_tune_vad_host(&d, &cells, 2, &pairs[0][0], T, agg2.data(), bits2.data(), lanes, out2.data(), threads) == 0);
        CHECK(memcmp(agg.data(), agg2.data(), sizeof(double) * agg.size()) == 0);
        CHECK(memcmp(bits.data(), bits2.data(), sizeof(unsigned) * bits.size()) == 0);
        CHECK(memcmp(out.data(), out2.data(), sizeof(double) * out.size()) == 0);
        for (unsigned b : bits) CHECK(b <= 1u);
        for (double v : out) CHECK(std::isfinite(v));
        // the masks alone, the components alone (the stateless masks need no scoring geometry at all)
        CHECK(dz_tune_vad_host(&d, nullptr, 1, taus, T, agg.data(), bits.data(), lanes, nullptr, threads) == 0);
        CHECK(dz_tune_vad_host(&d, &cells, 2, &pairs[0][0], T, agg2.data(), bits2.data(), lanes, nullptr, threads) == 0);
        CHECK(memcmp(bits.data(), bits2.data(), sizeof(unsigned) * bits.size()) == 0);
        CHECK(dz_tune_vad_host(&d, &cells, 2, &pairs[0][0], T, agg2.data(), nullptr, lanes, out2.data(), threads) == 0);
        CHECK(memcmp(out.data(), out2.data(), sizeof(double) * out.size()) == 0);
    }
    CHECK(dz_tune_vad_host(&d, &cells, 1, taus, T, agg.data(), bits.data(), 257, out.data(), threads) == 2);
    CHECK(dz_tune_vad_host(&d, &cells, 3, taus, T, agg.data(), bits.data(), 256, out.data(), threads) == 2);
}

void run_lsap(unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 2.0);
    for (int it = 0; it < 300; ++it) {
        const int nr = 1 + (int)(rng() % 12), nc = 1 + (int)(rng() % 40);
        std::vector<double> cost((size_t)nr * nc);
        for (double& c : cost) c = rng() % 5 == 0 ? 1e10 : u(rng);
        std::vector<int> col(nr, -2);
        CHECK(dz_lsap(cost.data(), nr, nc, col.data()) == 0);
        for (int r = 0; r < nr; ++r) CHECK(col[r] >= -1 && col[r] < nc);
    }
}
}  // namespace

int main(int argc, char** argv) {
    const int steps = argc > 1 ? atoi(argv[1]) : 60;
    run_lsap(1);
    run_streams(5, 4, steps, 2, 10, 40);
    for (int threads : {1, 3, 8}) {
        run_streams(10u + threads, 16, steps, threads);
        run_files(20u + threads, 5, steps / 2, threads);
        run_track(60u + threads, threads);
    }
    // two engines' host halves at once (two StreamBatch objects on two Python threads share the process-wide pool)
    dz_host_pool_set_spin(40);
    std::thread a([&] { run_streams(31, 12, steps, 4); }), b([&] { run_streams(32, 9, steps, 4); });
    std::thread c([&] { run_files(33, 4, steps / 2, 3); });
    a.join();
    b.join();
    c.join();
    dz_host_pool_set_spin(0);
    run_streams(40, 8, steps / 2, 6);
    // fewer items than workers, one item, and the spin setting changing between parallel-fors
    for (int n : {1, 2, 3, 5}) {
        dz_host_pool_set_spin(n % 2 ? 40 : 0);
        run_streams(50u + n, n, 20, 8);
    }
    printf("host_sanitize ok\n");
    return 0;
}
