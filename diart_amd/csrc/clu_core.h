// The decisions of one step of the incremental speaker clustering, fp64 like the reference: the ONE text of them.
// dz_clu_step (cluster.cpp) and the replay kernel of the hyper-parameter tuner (k_tune.hip through tune_core.h,
// DESIGN.md 4.16) compile it, so the reference's recorded outputs, the numpy oracle and scipy, which pin
// dz_clu_step and dz_lsap, pin what the GPU runs, and an assignment cannot flip at a tie between the two.
//
// Restates /root/reference/src/diart/blocks/clustering.py:119-218 (identify / __call__) and the SpeakerMap
// algebra it uses from /root/reference/src/diart/mapping.py (:15-21 optimal_assignments / mapped_indices,
// :217-231 valid_assignments (loose), :245-251 set_source_speaker, :260-294 unmap_threshold / unmap_speakers,
// :341-360 apply).  `tc_lsap` follows scipy.optimize.linear_sum_assignment (scipy/optimize/rectangular_lsap:
// Crouse's shortest augmenting path, columns scanned in reverse, ties resolved towards unassigned columns)
// because the 1e10 sentinels of mapping.py:48-52 make ties the normal case and the tie-breaking decides
// assignments.
//
// The logic is written once over a store S, which supplies where the arrays live and nothing else:
//   S::PerK<T>, S::PerG<T>, S::PerKG<T>   arrays of at least K, max(K, G) and K * G elements that decay to T*
//   S::Active                             the set of centroids in use: test / set / first_free / clear
//   S::Index                              the type a K x G offset is computed in
//   S::err(cause)                         what a step returns where the reference would raise
// CluFixed (below) is plain arrays of TC_KMAX / TC_GMAX elements and a 32-bit mask, so that one lane of a
// wavefront can take the decisions with the whole state in LDS; cluster.cpp has the heap-backed store of the
// handles, sized from K and G, without a limit.
#pragma once
#include <math.h>

#pragma clang fp contract(off)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TC_HD __host__ __device__ inline
#else
#define TC_HD inline
#endif

constexpr int TC_KMAX = 8;    // local speakers of a chunk
constexpr int TC_GMAX = 32;   // global speakers: the hypothesis of a frame is one 32-bit mask
constexpr double TC_INVALID = 1e10;   // MinimizationObjective.invalid_value, mapping.py:48-52

// why a step stops where the reference would raise
constexpr int TC_ERR_COST = 3;      // the assignment problem has NaN / -inf entries (scipy raises)
constexpr int TC_ERR_UNKNOWN = 4;   // clustering.py:98 assert, "Cannot update unknown centers"
constexpr int TC_ERR_FULL = 5;      // no free centroid for a new speaker

struct CluMask32 {
    unsigned bits;   // bit g: centroid g is in use
    TC_HD bool test(int g) const { return (bits >> g) & 1u; }
    TC_HD void set(int g) { bits |= 1u << g; }
    TC_HD void clear(int) { bits = 0; }
    TC_HD int first_free(int G) const {   // clustering.py:68-71
        const unsigned b = bits;
        for (int c = 0; c < G; ++c)
            if (!((b >> c) & 1u)) return c;
        return -1;
    }
};
struct CluFixed {
    template <typename T> using PerK = T[TC_KMAX];
    template <typename T> using PerG = T[TC_GMAX];
    template <typename T> using PerKG = T[TC_KMAX * TC_GMAX];
    using Active = CluMask32;
    using Index = int;
    // the tuner only asks for non-zero ("the chain stops here"): one value, so that the kernel has none to merge
    static constexpr int err(int) { return 3; }
};

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

// scipy.spatial.distance.cdist(..., "cosine"), fp64.  The scipy 1.15 x86-64 build sums dot products in two
// interleaved lanes (SSE2 doubles: even / odd elements, lanes added at the end, then the odd tail).  The order is
// reproduced exactly: with duplicated embeddings two rows of the cost matrix tie, and which one the Hungarian step
// favours depends on the last bit of the other entries (tests/golden/clustering_crowded.npz step 29 pins this).
// u is the float32 embedding (exact in fp64) at stride 1, v a centroid at stride vs.
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

template <class S>
struct TcLsapWork {
    typename S::template PerG<double> u, v, spc;
    typename S::template PerKG<double> temp;
    typename S::template PerG<int> path, col4row, row4col, remaining;
    typename S::template PerG<int> pr, pc;   // nc < nr: the pairs (row, column) sorted by row
    typename S::template PerG<char> SR, SC;
};

// rectangular LSAP (minimise): raw[0 .. *nraw) = the columns of the min(nr, nc) pairs sorted by row.
// 0 ok, 1 invalid entries, 2 infeasible.
template <class S>
TC_HD int tc_lsap(const double* cost_in, int nr, int nc, int* raw, int* nraw, TcLsapWork<S>& w) {
    using Index = typename S::Index;
    *nraw = 0;
    if (nr == 0 || nc == 0) return 0;
    const bool transpose = nc < nr;
    const double* cost = cost_in;
    if (transpose) {
        for (int i = 0; i < nr; ++i)
            for (int j = 0; j < nc; ++j) w.temp[(Index)j * nr + i] = cost_in[(Index)i * nc + j];
        const int t = nr;
        nr = nc;
        nc = t;
        cost = w.temp;
    }
    for (Index i = 0; i < (Index)nr * nc; ++i)
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
        // ---- augmenting path from row `cur`
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
                const double r = minVal + cost[(Index)i * nc + j] - w.u[i] - w.v[j];
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
        // ---- dual update
        w.u[cur] += minVal;
        for (int r = 0; r < nr; ++r)
            if (w.SR[r] && r != cur) w.u[r] += minVal - w.spc[w.col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (w.SC[j]) w.v[j] -= minVal - w.spc[j];
        // ---- augment
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

// SpeakerMap (minimisation objective only), K x G fp64 at stride G
template <class S>
struct TcMap {
    typename S::template PerKG<double> m;
    typename S::template PerG<int> raw;   // list(lsap(matrix)[1])  (mapping.py:15-16)
    int nraw, K, G, solved, rc;
};
template <class S>
TC_HD void tc_map_init(TcMap<S>& a, int K, int G) {
    a.K = K;
    a.G = G;
    a.solved = 0;
    a.rc = 0;
    a.nraw = 0;
    for (typename S::Index i = 0; i < (typename S::Index)K * G; ++i) a.m[i] = TC_INVALID;
}
template <class S>
TC_HD void tc_map_copy(TcMap<S>& d, const TcMap<S>& s) {
    d.K = s.K;
    d.G = s.G;
    d.solved = s.solved;
    d.rc = s.rc;
    d.nraw = s.nraw;
    for (typename S::Index i = 0; i < (typename S::Index)s.K * s.G; ++i) d.m[i] = s.m[i];
    for (int i = 0; i < s.nraw; ++i) d.raw[i] = s.raw[i];
}
// mapping.py:18-21 + :239-240 — a row is mapped iff its minimum is not the sentinel
template <class S>
TC_HD bool tc_source_mapped(const TcMap<S>& a, int s) {
    double best = a.m[(typename S::Index)s * a.G];
    for (int t = 1; t < a.G; ++t) {
        const double x = a.m[(typename S::Index)s * a.G + t];
        if (x != x) return true;   // np.min propagates NaN
        if (x < best) best = x;
    }
    if (best != best) return true;
    return best != TC_INVALID;
}
template <class S>
TC_HD int tc_solve(TcMap<S>& a, TcLsapWork<S>& w) {
    if (!a.solved) {
        a.rc = tc_lsap(a.m, a.K, a.G, a.raw, &a.nraw, w);
        if (a.rc) a.nraw = 0;
        a.solved = 1;
    }
    return a.rc;
}
// mapping.py:217-231 valid_assignments(strict=False): enumerate(raw), keep the mapped sources.  With G < K the
// problem is transposed and s runs over positions of the column list, not rows: the reference's quirk, kept.
template <class S>
TC_HD int tc_valid(TcMap<S>& a, TcLsapWork<S>& w, int* src, int* tgt, int* n) {
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
template <class S>
TC_HD void tc_unmap_source(TcMap<S>& a, int s) {
    for (int t = 0; t < a.G; ++t) a.m[(typename S::Index)s * a.G + t] = TC_INVALID;
    a.solved = 0;
}
template <class S>
TC_HD void tc_set_source(TcMap<S>& a, int s, int t) {   // mapping.py:245-251, best_possible_value = 0
    a.m[(typename S::Index)s * a.G + t] = 0.0;
    a.solved = 0;
}

// The state of one step: what the caller fills in (is_active, is_long, active, and dist for every chunk but the
// first), what the decision answers (upd, add, assign, active), and the scratch of whoever decides (in the struct,
// so that it lives where the struct lives: LDS on the device, the handle on the host).
template <class S>
struct TcStep {
    TcMap<S> dist, valid;
    TcLsapWork<S> work;
    typename S::template PerK<double> un;
    typename S::template PerG<double> cn;
    typename S::template PerK<int> is_active, is_long;
    typename S::template PerK<int> upd;      // centroid that gets += emb[k], or -1
    typename S::template PerK<int> add;      // free centroid that becomes emb[k], or -1
    typename S::template PerK<int> assign;   // the chunk's answer
    typename S::Active active;               // the centroids in use
    int rc;
    typename S::template PerG<int> src, tgt, pref;
    typename S::template PerK<int> missed, is_missed, newc;
};

// mapping.py:341-360 apply
template <class S>
TC_HD int tc_apply(TcStep<S>& s, TcMap<S>& map) {
    int *src = s.src, *tgt = s.tgt, n;
    if (tc_valid(map, s.work, src, tgt, &n)) return S::err(TC_ERR_COST);
    for (int k = 0; k < map.K; ++k) s.assign[k] = -1;
    for (int i = 0; i < n; ++i)
        if (src[i] < map.K) s.assign[src[i]] = tgt[i];
    return 0;
}

// The first chunk (clustering.py:149-158): every active speaker takes the next free centroid.  More active local
// speakers than centroids (only possible with max_speakers < K): the reference does not raise — its
// get_next_center_position() returns None and `centers[None] = emb` then overwrites EVERY centroid
// (clustering.py:101-117), i.e. undefined results.  Here the speakers that found no slot stay unmapped for this
// chunk, like any speaker that cannot be assigned later on.
template <class S>
TC_HD int tc_decide_first(TcStep<S>& s, int K, int G) {
    for (int k = 0; k < K; ++k) s.upd[k] = s.add[k] = -1;
    s.active.clear(G);
    tc_map_init(s.valid, K, G);
    for (int k = 0; k < K; ++k)
        if (s.is_active[k]) {
            const int g = s.active.first_free(G);
            if (g < 0) continue;
            s.active.set(g);
            s.add[k] = g;
            tc_set_source(s.valid, k, g);
        }
    return tc_apply(s, s.valid);
}

// Every later chunk (clustering.py:161-210): s.dist holds the cosine distances of the active speakers to the
// active centroids and the sentinel everywhere else.  Returns 0, or S::err(TC_ERR_*) where the reference would raise;
// upd / add / active then hold what was decided before that point (the reference updates centroids pair by pair
// and asserts mid-loop, so its state after a raise has exactly those updates).
template <class S>
TC_HD int tc_decide(TcStep<S>& s, int K, int G, double delta) {
    using Index = typename S::Index;
    int *src = s.src, *tgt = s.tgt, *pref = s.pref, *missed = s.missed, *is_missed = s.is_missed, *newc = s.newc, n;
    for (int k = 0; k < K; ++k) s.upd[k] = s.add[k] = -1;
    s.dist.solved = 0;
    tc_map_copy(s.valid, s.dist);
    // :168  unmap_threshold(delta_new): assignments with dist >= delta are dropped
    if (tc_valid(s.dist, s.work, src, tgt, &n)) return S::err(TC_ERR_COST);
    for (int i = 0; i < n; ++i)
        if (s.dist.m[(Index)src[i] * G + tgt[i]] >= delta) tc_unmap_source(s.valid, src[i]);

    // :171-194  a missed speaker opens a centroid if it is long and one is free, else takes the nearest free one
    int nmissed = 0;
    for (int k = 0; k < K; ++k) {
        is_missed[k] = s.is_active[k] && !tc_source_mapped(s.valid, k);
        if (is_missed[k]) missed[nmissed++] = k;
    }
    int nnew = 0;
    int known = 0;
    for (int g = 0; g < G; ++g) known += s.active.test(g);
    const int num_free = G - known;
    for (int mi = 0; mi < nmissed; ++mi) {
        const int spk = missed[mi];
        if (nnew < num_free && s.is_long[spk]) {
            newc[nnew++] = spk;
            continue;
        }
        int np = 0;
        for (int g = 0; g < G; ++g) {
            if (!s.active.test(g)) continue;
            // stable insertion by distance
            int p = np++;
            const double d = s.dist.m[(Index)spk * G + g];
            while (p > 0 && d < s.dist.m[(Index)spk * G + pref[p - 1]]) {
                pref[p] = pref[p - 1];
                --p;
            }
            pref[p] = g;
        }
        if (tc_valid(s.valid, s.work, src, tgt, &n)) return S::err(TC_ERR_COST);
        for (int i = 0; i < np; ++i) {
            bool taken = false;
            for (int j = 0; j < n; ++j) taken = taken || tgt[j] == pref[i];
            if (!taken) {
                tc_set_source(s.valid, spk, pref[i]);
                break;
            }
        }
    }
    // :197-202  update centroids of non-missed long speakers
    if (tc_valid(s.valid, s.work, src, tgt, &n)) return S::err(TC_ERR_COST);
    for (int i = 0; i < n; ++i) {
        const int ls = src[i], gs = tgt[i];
        if (is_missed[ls] || !s.is_long[ls]) continue;
        if (!s.active.test(gs)) return S::err(TC_ERR_UNKNOWN);
        s.upd[ls] = gs;
    }
    // :205-208  new centroids
    for (int i = 0; i < nnew; ++i) {
        const int g = s.active.first_free(G);
        if (g < 0) return S::err(TC_ERR_FULL);
        s.active.set(g);
        s.add[newc[i]] = g;
        tc_set_source(s.valid, newc[i], g);
    }
    return tc_apply(s, s.valid);
}
