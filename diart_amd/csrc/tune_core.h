// The decisions of one clustering step (cluster.cpp identify + step) with fixed-capacity arrays, so that one
// lane of a wavefront can take them: the replay kernel of the hyper-parameter tuner (k_tune.hip)
// walks thousands of (trial, file) chains, one wavefront each, and must take the SAME decisions as dz_clu_step
// or assignments flip at ties.  Everything here restates cluster.cpp line by line: the LSAP is lsap_solve
// (transposed when there are fewer columns than rows, columns scanned in reverse, ties towards unassigned
// columns), the map algebra is SpeakerMap's (1e10 sentinels, `source_mapped`'s NaN rule, `valid` enumerating the
// solver's column list), the missed-speaker rule sorts the active centroids stably by distance.  The arithmetic
// that feeds it (dot2's two interleaved partial sums, sqrt and division correctly rounded, no contraction) is in
// tc_dot2 / tc_cosine.  Host and device compile this text; the host side is what tests/test_tune_host.py holds
// against dz_clu_step (dz_tune_core_replay).
#pragma once
#include <math.h>

#include "../../include/diart_amd.h"

#pragma clang fp contract(off)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TC_HD __host__ __device__ inline
#else
#define TC_HD inline
#endif

constexpr int TC_KMAX = 8;    // local speakers of a chunk
constexpr int TC_GMAX = 32;   // global speakers: the hypothesis of a frame is one 32-bit mask
constexpr double TC_INVALID = 1e10;   // MinimizationObjective.invalid_value

TC_HD double tc_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}
TC_HD double tc_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

// cluster.cpp dot2 with u read as float32 (the embedding, exact in fp64) at stride 1 and v at stride vs
TC_HD double tc_dot2_fv(const float* u, const double* v, long vs, int n) {
    double s0 = 0.0, s1 = 0.0;
    const int m = n & ~1;
    for (int i = 0; i < m; i += 2) {
        s0 += (double)u[i] * v[(long)i * vs];
        s1 += (double)u[i + 1] * v[(long)(i + 1) * vs];
    }
    double s = s0 + s1;
    for (int i = m; i < n; ++i) s += (double)u[i] * v[(long)i * vs];
    return s;
}
TC_HD double tc_dot2_ff(const float* u, int n) {
    double s0 = 0.0, s1 = 0.0;
    const int m = n & ~1;
    for (int i = 0; i < m; i += 2) {
        s0 += (double)u[i] * (double)u[i];
        s1 += (double)u[i + 1] * (double)u[i + 1];
    }
    double s = s0 + s1;
    for (int i = m; i < n; ++i) s += (double)u[i] * (double)u[i];
    return s;
}
TC_HD double tc_dot2_vv(const double* v, long vs, int n) {
    double s0 = 0.0, s1 = 0.0;
    const int m = n & ~1;
    for (int i = 0; i < m; i += 2) {
        s0 += v[(long)i * vs] * v[(long)i * vs];
        s1 += v[(long)(i + 1) * vs] * v[(long)(i + 1) * vs];
    }
    double s = s0 + s1;
    for (int i = m; i < n; ++i) s += v[(long)i * vs] * v[(long)i * vs];
    return s;
}
TC_HD double tc_cosine(double dot, double nu, double nv) {
    double c = tc_div(dot, nu * nv);
    if (fabs(c) > 1.0) c = copysign(1.0, c);
    return 1.0 - c;
}

struct TcLsapWork {
    double u[TC_GMAX], v[TC_GMAX], spc[TC_GMAX], temp[TC_KMAX * TC_GMAX];
    int path[TC_GMAX], col4row[TC_GMAX], row4col[TC_GMAX], remaining[TC_GMAX];
    int pr[TC_GMAX], pc[TC_GMAX];
    char SR[TC_GMAX], SC[TC_GMAX];
};

// lsap_solve: raw[0 .. *nraw) = the columns of the pairs sorted by row.  0 ok, 1 invalid entries, 2 infeasible.
TC_HD int tc_lsap(const double* cost_in, int nr, int nc, int* raw, int* nraw, TcLsapWork& w) {
    *nraw = 0;
    if (nr == 0 || nc == 0) return 0;
    const bool transpose = nc < nr;
    const double* cost = cost_in;
    if (transpose) {
        for (int i = 0; i < nr; ++i)
            for (int j = 0; j < nc; ++j) w.temp[j * nr + i] = cost_in[i * nc + j];
        const int t = nr;
        nr = nc;
        nc = t;
        cost = w.temp;
    }
    for (int i = 0; i < nr * nc; ++i)
        if (cost[i] != cost[i] || cost[i] == -INFINITY) return 1;
    for (int i = 0; i < nr; ++i) {
        w.u[i] = 0.0;
        w.col4row[i] = -1;
    }
    for (int j = 0; j < nc; ++j) {
        w.v[j] = 0.0;
        w.path[j] = -1;
        w.row4col[j] = -1;
    }
    for (int cur = 0; cur < nr; ++cur) {
        double minVal = 0.0;
        int num_remaining = nc;
        for (int it = 0; it < nc; ++it) w.remaining[it] = nc - it - 1;
        for (int i = 0; i < nr; ++i) w.SR[i] = 0;
        for (int j = 0; j < nc; ++j) {
            w.SC[j] = 0;
            w.spc[j] = INFINITY;
        }
        int sink = -1, i = cur;
        while (sink == -1) {
            int index = -1;
            double lowest = INFINITY;
            w.SR[i] = 1;
            for (int it = 0; it < num_remaining; ++it) {
                const int j = w.remaining[it];
                const double r = minVal + cost[i * nc + j] - w.u[i] - w.v[j];
                if (r < w.spc[j]) {
                    w.path[j] = i;
                    w.spc[j] = r;
                }
                if (w.spc[j] < lowest || (w.spc[j] == lowest && w.row4col[j] == -1)) {
                    lowest = w.spc[j];
                    index = it;
                }
            }
            minVal = lowest;
            if (minVal == INFINITY) return 2;
            const int j = w.remaining[index];
            if (w.row4col[j] == -1) sink = j;
            else i = w.row4col[j];
            w.SC[j] = 1;
            w.remaining[index] = w.remaining[--num_remaining];
        }
        w.u[cur] += minVal;
        for (int r = 0; r < nr; ++r)
            if (w.SR[r] && r != cur) w.u[r] += minVal - w.spc[w.col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (w.SC[j]) w.v[j] -= minVal - w.spc[j];
        int j = sink;
        while (true) {
            const int r = w.path[j];
            w.row4col[j] = r;
            const int t = w.col4row[r];
            w.col4row[r] = j;
            j = t;
            if (r == cur) break;
        }
    }
    if (transpose) {
        // rows of the transposed problem are the original columns: pairs (col4row[c], c), sorted by row
        for (int c = 0; c < nr; ++c) {
            int p = c;
            const int row = w.col4row[c];
            while (p > 0 && w.pr[p - 1] > row) {
                w.pr[p] = w.pr[p - 1];
                w.pc[p] = w.pc[p - 1];
                --p;
            }
            w.pr[p] = row;
            w.pc[p] = c;
        }
        for (int c = 0; c < nr; ++c) raw[c] = w.pc[c];
    } else {
        for (int r = 0; r < nr; ++r) raw[r] = w.col4row[r];
    }
    *nraw = nr;
    return 0;
}

// SpeakerMap, K x G fp64 at stride G
struct TcMap {
    double m[TC_KMAX * TC_GMAX];
    int raw[TC_GMAX];
    int nraw, K, G, solved, rc;
};
TC_HD void tc_map_init(TcMap& a, int K, int G) {
    a.K = K;
    a.G = G;
    a.solved = 0;
    a.rc = 0;
    a.nraw = 0;
    for (int i = 0; i < K * G; ++i) a.m[i] = TC_INVALID;
}
TC_HD void tc_map_copy(TcMap& d, const TcMap& s) {
    d.K = s.K;
    d.G = s.G;
    d.solved = s.solved;
    d.rc = s.rc;
    d.nraw = s.nraw;
    for (int i = 0; i < s.K * s.G; ++i) d.m[i] = s.m[i];
    for (int i = 0; i < s.nraw; ++i) d.raw[i] = s.raw[i];
}
TC_HD bool tc_source_mapped(const TcMap& a, int s) {
    double best = a.m[s * a.G];
    for (int t = 1; t < a.G; ++t) {
        const double x = a.m[s * a.G + t];
        if (x != x) return true;   // np.min propagates NaN
        if (x < best) best = x;
    }
    if (best != best) return true;
    return best != TC_INVALID;
}
TC_HD int tc_solve(TcMap& a, TcLsapWork& w) {
    if (!a.solved) {
        a.rc = tc_lsap(a.m, a.K, a.G, a.raw, &a.nraw, w);
        if (a.rc) a.nraw = 0;
        a.solved = 1;
    }
    return a.rc;
}
// mapping.py valid_assignments(strict=False): enumerate(raw), keep the mapped sources
TC_HD int tc_valid(TcMap& a, TcLsapWork& w, int* src, int* tgt, int* n) {
    *n = 0;
    const int rc = tc_solve(a, w);
    if (rc) return rc;
    for (int s = 0; s < a.nraw; ++s)
        if (tc_source_mapped(a, s)) {
            src[*n] = s;
            tgt[*n] = a.raw[s];
            ++*n;
        }
    return 0;
}
TC_HD void tc_unmap_source(TcMap& a, int s) {
    for (int t = 0; t < a.G; ++t) a.m[s * a.G + t] = TC_INVALID;
    a.solved = 0;
}
TC_HD void tc_set_source(TcMap& a, int s, int t) {
    a.m[s * a.G + t] = 0.0;
    a.solved = 0;
}

// What the lanes exchange around the decisions of one chunk.
struct TcStep {
    TcMap dist, valid;
    TcLsapWork work;
    double un[TC_KMAX], cn[TC_GMAX];
    int is_active[TC_KMAX], is_long[TC_KMAX];
    int upd[TC_KMAX];      // centroid that gets += emb[k], or -1
    int add[TC_KMAX];      // free centroid that becomes emb[k], or -1
    int assign[TC_KMAX];   // the chunk's answer
    unsigned active;       // bit g: centroid g is in use
    int rc;
    // scratch of the deciding lane (in the struct, so that it lives where the struct lives: LDS on the device)
    int src[TC_GMAX], tgt[TC_GMAX], pref[TC_GMAX];
    int missed[TC_KMAX], is_missed[TC_KMAX], newc[TC_KMAX];
};

TC_HD int tc_next_center(unsigned active, int G) {
    for (int c = 0; c < G; ++c)
        if (!((active >> c) & 1u)) return c;
    return -1;
}

// step()'s tail: mapping.py apply
TC_HD int tc_apply(TcStep& s, TcMap& map) {
    int *src = s.src, *tgt = s.tgt, n;
    if (tc_valid(map, s.work, src, tgt, &n)) return 3;
    for (int k = 0; k < map.K; ++k) s.assign[k] = -1;
    for (int i = 0; i < n; ++i)
        if (src[i] < map.K) s.assign[src[i]] = tgt[i];
    return 0;
}

// the first chunk of a chain (identify :149-158): every active speaker takes the next free centroid
TC_HD int tc_decide_first(TcStep& s, int K, int G) {
    for (int k = 0; k < K; ++k) s.upd[k] = s.add[k] = -1;
    s.active = 0;
    tc_map_init(s.valid, K, G);
    for (int k = 0; k < K; ++k)
        if (s.is_active[k]) {
            const int g = tc_next_center(s.active, G);
            if (g < 0) continue;
            s.active |= 1u << g;
            s.add[k] = g;
            tc_set_source(s.valid, k, g);
        }
    return tc_apply(s, s.valid);
}

// every later chunk: s.dist holds the cosine distances of the active speakers to the active centroids and the
// sentinel everywhere else (identify :161-166).  Returns 0, or 3 where the reference would raise.
TC_HD int tc_decide(TcStep& s, int K, int G, double delta) {
    int *src = s.src, *tgt = s.tgt, *pref = s.pref, *missed = s.missed, *is_missed = s.is_missed, *newc = s.newc, n;
    for (int k = 0; k < K; ++k) s.upd[k] = s.add[k] = -1;
    s.dist.solved = 0;
    tc_map_copy(s.valid, s.dist);
    if (tc_valid(s.dist, s.work, src, tgt, &n)) return 3;
    for (int i = 0; i < n; ++i)
        if (s.dist.m[src[i] * G + tgt[i]] >= delta) tc_unmap_source(s.valid, src[i]);

    int nmissed = 0;
    for (int k = 0; k < K; ++k) {
        is_missed[k] = s.is_active[k] && !tc_source_mapped(s.valid, k);
        if (is_missed[k]) missed[nmissed++] = k;
    }
    int nnew = 0;
    int known = 0;
    for (int g = 0; g < G; ++g) known += (s.active >> g) & 1u;
    const int num_free = G - known;
    for (int mi = 0; mi < nmissed; ++mi) {
        const int spk = missed[mi];
        if (nnew < num_free && s.is_long[spk]) {
            newc[nnew++] = spk;
            continue;
        }
        int np = 0;
        for (int g = 0; g < G; ++g) {
            if (!((s.active >> g) & 1u)) continue;
            // stable insertion by distance
            int p = np++;
            const double d = s.dist.m[spk * G + g];
            while (p > 0 && d < s.dist.m[spk * G + pref[p - 1]]) {
                pref[p] = pref[p - 1];
                --p;
            }
            pref[p] = g;
        }
        if (tc_valid(s.valid, s.work, src, tgt, &n)) return 3;
        for (int i = 0; i < np; ++i) {
            bool taken = false;
            for (int j = 0; j < n; ++j) taken = taken || tgt[j] == pref[i];
            if (!taken) {
                tc_set_source(s.valid, spk, pref[i]);
                break;
            }
        }
    }
    if (tc_valid(s.valid, s.work, src, tgt, &n)) return 3;
    for (int i = 0; i < n; ++i) {
        const int ls = src[i], gs = tgt[i];
        if (is_missed[ls] || !s.is_long[ls]) continue;
        if (!((s.active >> gs) & 1u)) return 3;   // "Cannot update unknown centers"
        s.upd[ls] = gs;
    }
    for (int i = 0; i < nnew; ++i) {
        const int g = tc_next_center(s.active, G);
        if (g < 0) return 3;
        s.active |= 1u << g;
        s.add[newc[i]] = g;
        tc_set_source(s.valid, newc[i], g);
    }
    return tc_apply(s, s.valid);
}

// ---------------------------------------------------------------------------------------------------------
// One (trial, file) chain: the file's chunks in order.  `lane` of `nl` lanes share the work that has no order
// (the norms, the K x G distances, the centroid rows); lane 0 takes the decisions; `sync` is the workgroup
// barrier (nothing on the host, where nl = 1).  The centroids are ctr[d * G + g] (lanes with neighbouring g read
// neighbouring doubles).  Returns -1, or the index of the first chunk at which dz_clu_step would return non-zero;
// the chunks from there on keep the -1 their assign rows were filled with.
// ---------------------------------------------------------------------------------------------------------
template <typename Sync>
TC_HD int tc_chain(const dz_tune_desc& d, int n, double tau, double rho, double delta, signed char* assign /* this trial's */,
                   double* ctr, TcStep& s, int lane, int nl, Sync sync) {
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
                    if ((s.active >> i) & 1u) s.cn[i] = tc_sqrt(tc_dot2_vv(ctr + i, G, D));
                } else if (s.is_active[i - G]) {
                    s.un[i - G] = tc_sqrt(tc_dot2_ff(e + (long)(i - G) * D, D));
                }
            }
            sync();
            for (int i = lane; i < K * G; i += nl) {
                const int k = i / G, g = i - k * G;
                double v = TC_INVALID;
                if (s.is_active[k] && ((s.active >> g) & 1u))
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
