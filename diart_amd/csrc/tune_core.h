// The replay of the hyper-parameter tuner over cached model outputs: tc_chain walks one (trial, file)
// chain of clustering steps, tc_row_mask turns the assignments into one packed output row of the tail.  The
// decisions of a step are clu_core.h's, the text dz_clu_step runs too, here on its fixed store (K <= TC_KMAX,
// G <= TC_GMAX, the whole state in LDS); what this file adds is how the lanes of a wavefront share the arithmetic that
// feeds them (each norm and each of the K x G distances summed by ONE lane in the core's order).  Host and device
// compile this text: k_tune.hip for the kernels, tune_score.cpp for backend="core", which tests/test_tune_host.py
// holds against dz_clu_step + dz_tail_step.
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
