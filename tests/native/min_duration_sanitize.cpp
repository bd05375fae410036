// The minimum-duration scoring of the track tuners on the host (csrc/tune_score.cpp: dz_tune_vad_host with four columns,
// the text of tune_vad_score_kernel<TcDurRule> with its lanes played in order, and dz_tune_track_score_dur, the
// sequential text)
// on a generated cache, for AddressSanitizer + UBSan (tests/test_min_duration_host.py compiles this file with g++
// together with the host sources and runs it).  Files of 1, 9, 70 and 300 chunks: at 256 lanes one step per lane with
// empty lanes behind, and two steps per lane; tracks of slow waves with flat stretches, so that spans cross many lanes;
// trials with both durations zero, small, around a second and above the file.  The two texts must agree within
// 1e-9 x total per component, and the kernel's text must give the same components at 1, 7 and 256 lanes within that.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <cstdarg>

#include "../../include/diart_amd.h"

// the error string lives in api.hip, which needs hipcc: the host sources get their own here
static thread_local char g_err[512];
void dz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* dz_last_error(void) { return g_err; }

namespace {

struct Rng {
    unsigned long long s;
    double next() {   // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0;
    }
};

int fail(const char* what, int a = 0, int b = 0) {
    std::printf("min_duration_sanitize FAILED: %s (%d, %d): %s\n", what, a, b, dz_last_error());
    return 1;
}

}  // namespace

int main() {
    const int F = 16, N = 4, counts[N] = {1, 9, 70, 300};
    const double step = 0.5, latency = 2.5, duration = 5.0, collar = 0.05;
    const int nwin = 5;
    Rng rng{12345};
    std::vector<int> chunk_off(1, 0);
    for (int n = 0; n < N; ++n) chunk_off.push_back(chunk_off.back() + counts[n]);
    const int chunks = chunk_off.back();
    std::vector<float> seg((size_t)chunks * F);
    std::vector<double> starts(chunks), res(chunks, duration / F), t0(chunks), out_res(chunks), hamming(F);
    for (int i = 0; i < F; ++i) hamming[i] = 0.54 - 0.46 * std::cos(2.0 * M_PI * i / (F - 1));
    std::vector<int> plan((size_t)chunks * (4 + nwin));
    for (int n = 0; n < N; ++n) {
        const int c0 = chunk_off[n];
        for (int c = 0; c < counts[n]; ++c) {
            starts[c0 + c] = step * c;
            const bool flat = (c / 40) % 2 == 1;   // forty steps high, in a row: a span across many lanes
            for (int i = 0; i < F; ++i) {
                const double t = starts[c0 + c] + (i + 0.5) * duration / F;
                seg[(size_t)(c0 + c) * F + i] = (float)(flat ? 0.9 : 0.5 + 0.35 * std::sin(t * (1.3 + n)) + 0.1 * (rng.next() - 0.5));
            }
        }
        if (dz_tune_plan(counts[n], F, step, latency, starts.data() + c0, res.data() + c0, plan.data() + (size_t)c0 * (4 + nwin),
                         t0.data() + c0, out_res.data() + c0))
            return fail("dz_tune_plan", n);
    }
    std::vector<int> row_off(1, 0), row_chunk;
    for (int c = 0; c < chunks; ++c) {
        const int rows = plan[(size_t)c * (4 + nwin)] + plan[(size_t)c * (4 + nwin) + 1];
        row_off.push_back(row_off.back() + rows);
        row_chunk.insert(row_chunk.end(), rows, c);
    }
    const int total_rows = row_off.back();
    // frame middles (rows + 1 per step), the files' cells (the sorted middles), a random reference, the prefix sums
    std::vector<double> mids((size_t)total_rows + chunks), dur_prefix, ref_prefix, cell_dur;
    std::vector<int> mid_cell(mids.size()), file_cell_off(1, 0);
    std::vector<unsigned long long> cell_ref;
    for (int n = 0; n < N; ++n) {
        std::vector<double> bounds;
        for (int c = chunk_off[n]; c < chunk_off[n + 1]; ++c)
            for (int i = 0; i <= row_off[c + 1] - row_off[c]; ++i) {
                const double s = t0[c] + i * out_res[c];
                mids[(size_t)row_off[c] + c + i] = 0.5 * (s + (s + out_res[c])) - 0.25 * n;
                bounds.push_back(mids[(size_t)row_off[c] + c + i]);
            }
        std::sort(bounds.begin(), bounds.end());
        bounds.erase(std::unique(bounds.begin(), bounds.end()), bounds.end());
        for (int c = chunk_off[n]; c < chunk_off[n + 1]; ++c)
            for (int i = 0; i <= row_off[c + 1] - row_off[c]; ++i) {
                const size_t at = (size_t)row_off[c] + c + i;
                mid_cell[at] = (int)(std::lower_bound(bounds.begin(), bounds.end(), mids[at]) - bounds.begin());
            }
        const int ncell = (int)bounds.size() - 1;
        dur_prefix.push_back(0.0);
        ref_prefix.push_back(0.0);
        bool active = false;
        for (int i = 0; i < ncell; ++i) {
            if (rng.next() < 0.05) active = !active;
            const double d = bounds[i + 1] - bounds[i];
            cell_dur.push_back(d);
            cell_ref.push_back(active ? 1ull : 0ull);
            dur_prefix.push_back(dur_prefix.back() + d);
            ref_prefix.push_back(ref_prefix.back() + (active ? d : 0.0));
        }
        file_cell_off.push_back(file_cell_off.back() + ncell);
    }
    dz_tune_desc d = {};
    d.seg = seg.data();
    d.chunk_off = chunk_off.data();
    d.plan = plan.data();
    d.row_off = row_off.data();
    d.row_chunk = row_chunk.data();
    d.hamming = hamming.data();
    d.N = N, d.F = F, d.K = 1, d.D = 1, d.G = 1, d.nwin = nwin, d.total_chunks = chunks, d.total_rows = total_rows;
    dz_tune_cells cells = {};   // (the members neither entry reads stay NULL)
    cells.file_chunk_off = chunk_off.data();
    cells.row_off = row_off.data();
    cells.mids = mids.data();
    cells.mid_cell = mid_cell.data();
    cells.file_cell_off = file_cell_off.data();
    cells.cell_dur = cell_dur.data();
    cells.cell_ref = cell_ref.data();
    cells.dur_prefix = dur_prefix.data();
    cells.ref_prefix = ref_prefix.data();
    cells.n_files = N, cells.total_rows = total_rows, cells.total_chunks = chunks, cells.max_speakers = 1, cells.collar = collar;

    const double durations[][2] = {{0.0, 0.0}, {0.2, 0.0}, {0.0, 0.3}, {1.1, 0.9}, {2.4, 0.07}, {1e4, 0.0}, {0.0, 1e4}, {0.4, 3.3}};
    const int T = (int)(sizeof(durations) / sizeof(durations[0]));
    std::vector<double> taus;
    for (int t = 0; t < T; ++t) {
        const double on = 0.45 + 0.03 * t;
        taus.insert(taus.end(), {on, t % 3 == 0 ? on : on - 0.2, durations[t][0], durations[t][1]});
    }
    std::vector<double> agg(total_rows), first((size_t)T * N * 5), out((size_t)T * N * 5), seq((size_t)T * N * 5);
    std::vector<unsigned> bits((size_t)T * total_rows), bits0;
    const int lanes[] = {256, 7, 1};
    for (int li = 0; li < 3; ++li) {
        std::fill(out.begin(), out.end(), -1.0);
        if (dz_tune_vad_host(&d, &cells, 4, taus.data(), T, agg.data(), bits.data(), lanes[li], out.data(), li == 0 ? 3 : 1))
            return fail("dz_tune_vad_host, four columns", lanes[li]);
        if (li == 0) {
            first = out;
            bits0 = bits;
        }
        if (bits != bits0) return fail("masks differ between lane counts", lanes[li]);
        for (size_t i = 0; i < out.size(); ++i) {
            const double bar = 1e-9 * std::max(first[i / 5 * 5], 1.0);
            if (!(std::fabs(out[i] - first[i]) <= bar)) return fail("components differ between lane counts", lanes[li], (int)i);
        }
    }
    if (dz_tune_track_score_dur(&cells, T, bits0.data(), taus.data(), seq.data(), 3))
        return fail("dz_tune_track_score_dur");
    double hyp = 0.0;
    for (size_t i = 0; i < seq.size(); ++i) {
        const double bar = 1e-9 * std::max(seq[i / 5 * 5], 1.0);
        if (!(std::fabs(seq[i] - first[i]) <= bar)) return fail("the two texts differ", (int)(i / 5), (int)(i % 5));
        if (i % 5 == 1 || i % 5 == 2) hyp += seq[i];
    }
    if (!(hyp > 10.0)) return fail("no hypothesis to speak of");
    // the refusals: status 2 before anything is read
    std::vector<double> bad = taus;
    bad[2] = -0.1;
    if (dz_tune_vad_host(&d, &cells, 4, bad.data(), T, agg.data(), bits.data(), 256, out.data(), 1) != 2)
        return fail("a negative duration passed");
    bad[2] = 0.0, bad[7] = NAN;
    if (dz_tune_track_score_dur(&cells, T, bits0.data(), bad.data(), seq.data(), 1) != 2)
        return fail("a NaN duration passed");
    if (dz_tune_vad_host(&d, &cells, 4, taus.data(), T, agg.data(), bits.data(), 257, out.data(), 1) != 2)
        return fail("257 lanes passed");
    if (dz_tune_vad_host(&d, &cells, 4, nullptr, T, agg.data(), bits.data(), 256, out.data(), 1) != 2 ||
        dz_tune_track_score_dur(&cells, 0, bits0.data(), taus.data(), seq.data(), 1) != 2)
        return fail("NULL or T < 1 passed");
    std::printf("min_duration_sanitize ok: %d trials x %d files, %d rows, hypothesis %.1f s\n", T, N, total_rows, hyp);
    return 0;
}
