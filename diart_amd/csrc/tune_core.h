// The replay of the hyper-parameter tuner over cached model outputs: tc_chain walks one (trial, file)
// chain of clustering steps, tc_row_mask turns the assignments into one packed output row of the tail.  The
// decisions of a step are clu_core.h's, the text dz_clu_step runs too, here on its fixed store (K <= TC_KMAX,
// G <= TC_GMAX, the whole state in LDS); what this file adds is how the lanes of a wavefront share the arithmetic that
// feeds them (each norm and each of the K x G distances summed by ONE lane in the core's order).  Host and device
// compile this text: k_tune.hip for the kernels, tune_score.cpp for backend="core", which tests/test_tune_host.py
// holds against dz_clu_step + dz_tail_step.  The VoiceActivityDetection half (tc_vad_*, at the end) is k_tune_vad.hip's
// and dz_tune_vad_host's in the same way.
#pragma once
#include "../../include/diart_amd.h"
#include "clu_core.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------------------
// One (trial, file) chain: the file's chunks in order.  `lane` of `nl` lanes share the work that has no order
// (the norms, the K x G distances, the centroid rows); lane 0 takes the decisions; `sync` is the workgroup
// barrier (nothing on the host, where nl = 1).  The centroids are ctr[d * G + g] (lanes with neighbouring g read
// neighbouring doubles).  Returns -1, or the index of the first chunk at which dz_clu_step would return non-zero;
// the chunks from there on keep the -1 their assign rows were filled with.
// ---------------------------------------------------------------------------------------------------------
template <typename Sync>
TC_HD int tc_chain(const dz_tune_desc& d, int n, double tau, double rho, double delta, signed char* assign /* this trial's */,
                   double* ctr, TcStep<CluFixed>& s, int lane, int nl, Sync sync) {
    const int K = d.K, G = d.G, D = d.D;
    const float tau32 = (float)tau, rho32 = (float)rho;
    const int c0 = d.chunk_off[n], c1 = d.chunk_off[n + 1];
    bool has_centers = false;
    for (int c = c0; c < c1; ++c) {
        const float* e = d.emb + (long)c * K * D;
        sync();
        for (int k = lane; k < K; k += nl) {
            const unsigned fl = d.pre_flags[(long)c * K + k];
            const bool act = !(fl & 1u) && d.pre_max[(long)c * K + k] >= tau32;
            s.is_long[k] = d.pre_mean[(long)c * K + k] >= rho32 ? 1 : 0;
            s.is_active[k] = (act && !(fl & 2u)) ? 1 : 0;
        }
        sync();
        if (!has_centers) {
            if (lane == 0) s.rc = tc_decide_first(s, K, G);
            has_centers = true;
        } else {
            for (int i = lane; i < G + K; i += nl) {
                if (i < G) {
                    if (s.active.test(i)) s.cn[i] = tc_sqrt(tc_dot2_vv(ctr + i, G, D));
                } else if (s.is_active[i - G]) {
                    s.un[i - G] = tc_sqrt(tc_dot2_ff(e + (long)(i - G) * D, D));
                }
            }
            sync();
            for (int i = lane; i < K * G; i += nl) {
                const int k = i / G, g = i - k * G;
                double v = TC_INVALID;
                if (s.is_active[k] && s.active.test(g))
                    v = tc_cosine(tc_dot2_fv(e + (long)k * D, ctr + g, G, D), s.un[k], s.cn[g]);
                s.dist.m[i] = v;
            }
            if (lane == 0) {   // a fresh map: nothing solved, no column list (tc_map_copy copies nraw of them)
                s.dist.K = K;
                s.dist.G = G;
                s.dist.solved = 0;
                s.dist.rc = 0;
                s.dist.nraw = 0;
            }
            sync();
            if (lane == 0) s.rc = tc_decide(s, K, G, delta);
        }
        sync();
        if (s.rc) return c - c0;
        for (int k = 0; k < K; ++k) {
            const int gu = s.upd[k], ga = s.add[k];
            if (gu >= 0)
                for (int i = lane; i < D; i += nl) ctr[(long)i * G + gu] += (double)e[(long)k * D + i];
            if (ga >= 0)
                for (int i = lane; i < D; i += nl) ctr[(long)i * G + ga] = (double)e[(long)k * D + i];
        }
        for (int k = lane; k < K; k += nl) assign[(long)c * K + k] = (signed char)s.assign[k];
    }
    return -1;
}

TC_HD int tc_clip(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The hypothesis of packed output row p under one trial: bit g = the aggregated score of global speaker g is
// > tau (tail.cpp: Hamming-weighted sum over the step's buffers in order, divided by the sum of the weights; the
// first chunk's prepended rows are that chunk's own scores).  A buffer in which g has no local speaker adds
// h * 0.0 on the host: leaving that addition out changes at most the sign of a zero, which no comparison sees.
TC_HD unsigned tc_row_mask(const dz_tune_desc& d, int p, double tau, const signed char* assign /* this trial's */) {
    const int K = d.K, F = d.F, G = d.G;
    const int c = d.row_chunk[p], r = p - d.row_off[c];
    const int* plan = d.plan + (long)c * (4 + d.nwin);
    const int pre = plan[1], nbuf = plan[3];
    const unsigned all = G >= 32 ? 0xffffffffu : ((1u << G) - 1u);
    unsigned out = 0, seen = 0;
    if (r < pre) {
        const int row = tc_clip(plan[2] + r, F - 1);
        for (int k = 0; k < K; ++k) {
            const int g = assign[(long)c * K + k];
            if (g < 0) continue;
            seen |= 1u << g;
            if ((double)d.seg[((long)c * F + row) * K + k] > tau) out |= 1u << g;
        }
    } else {
        const int ra = r - pre, cb0 = c - nbuf + 1;
        double den = 0.0;
        for (int b = 0; b < nbuf; ++b) {
            const double h = d.hamming[tc_clip(plan[4 + b] + ra, F - 1)];
            den = b == 0 ? h : den + h;
            for (int k = 0; k < K; ++k) {
                const int g = assign[(long)(cb0 + b) * K + k];
                if (g >= 0) seen |= 1u << g;
            }
        }
        for (unsigned m = seen; m; m &= m - 1) {
            const int g = __builtin_ctz(m);
            double num = 0.0;
            bool first = true;
            for (int b = 0; b < nbuf; ++b) {
                const long cb = cb0 + b;
                int ks = -1;
                for (int k = 0; k < K; ++k)
                    if (assign[cb * K + k] == g) ks = k;
                if (ks < 0) continue;
                const int row = tc_clip(plan[4 + b] + ra, F - 1);
                const double term = d.hamming[row] * (double)d.seg[(cb * F + row) * K + ks];
                num = first ? term : num + term;
                first = false;
            }
            if (tc_div(num, den) > tau) out |= 1u << g;
        }
    }
    if (0.0 > tau) out |= all & ~seen;   // a speaker nobody was mapped to scores 0.0
    return out;
}

// ---------------------------------------------------------------------------------------------------------
// VoiceActivityDetection (one track per chunk: K = G = 1, seg is (chunks, F), no clustering).
//
// tc_vad_row: the aggregated speech score of packed output row p, the value tc_row_mask compares with tau when
// the one local speaker of every buffer is mapped.  It does not depend on tau: computed once per cache.
// ---------------------------------------------------------------------------------------------------------
TC_HD double tc_vad_row(const dz_tune_desc& d, int p) {
    const int F = d.F;
    const int c = d.row_chunk[p], r = p - d.row_off[c];
    const int* plan = d.plan + (long)c * (4 + d.nwin);
    const int pre = plan[1], nbuf = plan[3];
    if (r < pre) return (double)d.seg[(long)c * F + tc_clip(plan[2] + r, F - 1)];
    const int ra = r - pre;
    const long cb0 = c - nbuf + 1;
    double den = 0.0, num = 0.0;
    for (int b = 0; b < nbuf; ++b) {
        const int row = tc_clip(plan[4 + b] + ra, F - 1);
        const double h = d.hamming[row];
        const double term = h * (double)d.seg[(cb0 + b) * F + row];
        den = b == 0 ? h : den + h;
        num = b == 0 ? term : num + term;
    }
    return tc_div(num, den);
}

// What the detection error rate of one (trial, file) needs besides the file's constants: the duration the merged
// speech turns cover, and the part of it in which the reference is active.
struct TcVadSum {
    double hyp, both;
};
// The end of the latest-ending turn so far and the scoring cell that starts there (-infinity: no turn yet).
struct TcVadEnd {
    double e;
    int cell;
};

// Steps [c_lo, c_hi) of one file under one tau, in order.  Row r of a step is speech when agg > tau; a turn runs
// from mid[onset] to mid[first inactive row] (the row after the step's last closes an open turn; mids holds rows + 1
// values per step), turns no longer than 1e-6 are dropped (Segment.__bool__).  Turns arrive sorted by start (the
// cache checks that the steps' grids are), so Annotation.support(collar) is a running maximum: a turn whose gap to
// `end` is <= 1e-6 or < collar extends the covered span from `end` to its own end (if that is later), any other
// turn opens a new span.  Every turn therefore adds the cells [from, its end cell) with from = the cell of `end`
// or its own start cell: nothing is covered twice.  Durations are differences of the file's prefix sums
// (dur_prefix / ref_prefix: ncell + 1 values, cell_dur and cell_dur where the reference is active, summed in order).
TC_HD TcVadEnd tc_vad_walk(const double* agg, const int* row_off, const double* mids, const int* mid_cell,
                           const double* dur_prefix, const double* ref_prefix, double tau, double collar, int c_lo,
                           int c_hi, TcVadEnd end, TcVadSum* sum) {
    for (int c = c_lo; c < c_hi; ++c) {
        const int p = row_off[c], rows = row_off[c + 1] - p;
        const double* mid = mids + (long)p + c;
        const int* cell = mid_cell + (long)p + c;
        int onset = -1;
        for (int r = 0; r <= rows; ++r) {
            const bool on = r < rows && agg[p + r] > tau;
            if (on && onset < 0) onset = r;
            if (!on && onset >= 0) {
                const double s = mid[onset], e = mid[r];
                if (e - s > 1e-6) {
                    const double gap = s - end.e;
                    int from = cell[onset];
                    bool adds = true;
                    if (gap <= 1e-6 || gap < collar) {
                        from = end.cell;
                        adds = e > end.e;
                    }
                    if (adds) {
                        const int to = cell[r];
                        sum->hyp += dur_prefix[to] - dur_prefix[from];
                        sum->both += ref_prefix[to] - ref_prefix[from];
                        end.e = e;
                        end.cell = to;
                    }
                }
                onset = -1;
            }
        }
    }
    return end;
}

// The five components (metrics.COMPONENTS) of DetectionErrorRate as dz_tune_score builds them for one hypothesis
// label and one reference label: the confusion is 0.
TC_HD void tc_vad_components(double total, TcVadSum s, double* o) {
    const double fa = s.hyp - s.both, missed = total - s.both;
    o[0] = total;
    o[1] = s.both;
    o[2] = fa > 0.0 ? fa : 0.0;
    o[3] = missed > 0.0 ? missed : 0.0;
    o[4] = 0.0;
}

// How a workgroup of nl lanes shares a file of `chunks` steps: lane i walks steps [i * per, (i + 1) * per).
TC_HD int tc_vad_steps_per_lane(int chunks, int nl) { return (chunks + nl - 1) / nl; }
