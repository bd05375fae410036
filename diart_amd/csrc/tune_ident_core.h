// Tuning delta_id by replay: the naming rule of gallery.SpeakerNames over the chunks of one
// (trial, file) chain, and the identification error rate components of one (trial, file) pair.  Host and device
// compile this text: k_tune_ident.hip for the kernels, tune_score.cpp for the host backends.
//
// The rule, per global speaker g: (best_d, best_e) is the closest match seen so far.  A step's local speaker k with
// assign[k] = g, a match index[k] = e >= 0 and (double)distance[k] <= delta_id replaces it when distance[k] < best_d
// (float32, strictly; k ascending).  g carries the name of best_e unless another speaker holds the same voiceprint with
// a lower best_d, or with the same best_d and a lower g (SpeakerNames.holders: a stable order of best_d).
//
// The scoring starts where tc_score_pair starts (tc_score_cells: the hypothesis mask of every scoring cell); then
// every set bit g of a cell is looked up in the identities of the step that owns the cell: a reference bit 0..63 of
// the file, or "other" (an unnamed speaker, or a name no reference label of the file has).  Labels are compared as they
// are: no mapping, no co-occurrence sweep.
//
// Both halves take several (plane, threshold) points per clustering trial: a chain per (trial, point,
// file) for the names (ti_chain), and for the score the cells once and then every point's components (ti_score_pair
// over ti_score_point).  One point is the case points = 1 of the same text.
#pragma once
#include "tune_core.h"

#pragma clang fp contract(off)

constexpr int TI_OTHER = -1;   // an identity that is no reference label of the file
// A sweep evaluates one clustering trial at `points` (plane, threshold) points: a plane is one stored
// match of the cache (one top_n of a normalised gallery), and the points are plane-major.
constexpr int TI_MAX_POINTS = 256;
constexpr int TI_MAX_PLANES = 8;

// One step of speaker g's state.  A NaN distance passes neither comparison.
TC_HD void ti_update(float& best_d, int& best_e, int g, const signed char* assign, const int* index, const float* dist, int K,
                     double delta_id) {
    for (int k = 0; k < K; ++k) {
        if (assign[k] != g || index[k] < 0) continue;
        const float d = dist[k];
        if ((double)d <= delta_id && d < best_d) {
            best_d = d;
            best_e = index[k];
        }
    }
}

// The voiceprint whose name g carries in this step, or -1.  peer(g2, &d2, &e2) gives speaker g2's state; every caller
// runs the whole loop (on the device peer is a shuffle that all lanes of the wavefront take part in).
template <typename Peer>
TC_HD int ti_hold(float d, int e, int g, int G, Peer peer) {
    bool beaten = false;
    for (int g2 = 0; g2 < G; ++g2) {
        float d2;
        int e2;
        peer(g2, &d2, &e2);
        if (g2 != g && e2 == e && (d2 < d || (d2 == d && g2 < g))) beaten = true;
    }
    return (e >= 0 && !beaten) ? e : -1;
}

// The identity of a holder in file n's reference: vp_ref (N, V) holds the reference bit whose label is voiceprint v's
// name, or -1.
TC_HD signed char ti_identity(int hold, const signed char* vp_ref_n, int V) {
    if (hold < 0 || hold >= V) return (signed char)TI_OTHER;
    const int b = vp_ref_n[hold];
    return (signed char)((b >= 0 && b < 64) ? b : TI_OTHER);
}

struct TiScoreIn {
    TcScoreIn cells;             // what tc_score_cells takes
    const signed char* ident;    // this trial's identities (total_chunks, G)
    const int* cell_step;        // the file's cells: the step (a chunk of the cache) that owns each
};

struct TiScoreShared {
    double part[5][TC_SCORE_LANES];   // the lanes' partial sums
    double end_e[TC_SCORE_LANES];
    int end_cell[TC_SCORE_LANES];
    unsigned lane_any[TC_SCORE_LANES];
    unsigned lane_x[TC_SCORE_LANES];
    int err;
};

// One cell: the five components' integer factors from the hypothesis mask h under the identities of step `id`
// (G of them) and the reference mask rm.  n[0..4] in metrics.COMPONENTS order.
TC_HD void ti_cell_counts(unsigned h, unsigned long long rm, const signed char* id, int* n) {
    unsigned long long hm = 0;
    for (unsigned m = h; m; m &= m - 1) {
        const int b = id[__builtin_ctz(m)];
        if (b >= 0 && b < 64) hm |= 1ull << b;
    }
    const int nref = __builtin_popcountll(rm), nhyp = __builtin_popcount(h), both = __builtin_popcountll(hm & rm);
    n[0] = nref;
    n[1] = both;
    n[2] = nhyp > nref ? nhyp - nref : 0;
    n[3] = nref > nhyp ? nref - nhyp : 0;
    n[4] = (nref < nhyp ? nref : nhyp) - both;
}

// The components of one point of a pair: after tc_score_cells left the hypothesis masks in `scratch`, every cell's
// factors under the identities `ident` (total_chunks, G).  Lane l takes cells l, l + nl, ...; lane 0 adds the lanes'
// sums in lane order, so a point's doubles do not depend on how many points share the cells.
template <typename Lanes>
TC_HD void ti_score_point(const TiScoreIn& in, const signed char* ident, TiScoreShared& sh, const unsigned* scratch,
                          double* out /* 5 */, int* err, Lanes lanes) {
    const TcScoreIn& ci = in.cells;
    const int nl = lanes.nl, ncell = ci.ncell, G = ci.G;
    const unsigned gmask = G >= 32 ? 0xffffffffu : ((1u << G) - 1u);
    // ---- the components over the cells, per lane
    lanes([&](int lane) {
        double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = lane; i < ncell; i += nl) {
            const unsigned h = tc_word_load(scratch + i) & gmask;
            const unsigned long long rm = ci.cell_ref[i];
            if (!h && !rm) continue;
            const int c = in.cell_step[i];
            if (c < ci.c0 || c >= ci.c1) {   // (a cache whose cells name a step of another file)
                sh.err = TC_SCORE_ERR_CELLS;
                continue;
            }
            const double dur = ci.cell_dur[i];
            int n[5];
            ti_cell_counts(h, rm, ident + (long)c * G, n);
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[q] += dur * n[q];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) sh.part[q][lane] = acc[q];
    });
    // ---- lane 0: the lanes' sums in lane order
    lanes([&](int lane) {
        if (lane != 0) return;
        if (sh.err) {
            tc_err_raise(err, sh.err);
            return;
        }
        for (int q = 0; q < 5; ++q) {
            double s = 0.0;
            for (int j = 0; j < nl; ++j) s += sh.part[q][j];
            out[q] = s;
        }
    });
}

// One (trial, file) pair at `points` points: the cells once (the toggle and prefix-XOR phases depend on the masks
// alone), then the components of every point in turn.  in.ident is point 0's identities; point j's lie j *
// ident_stride bytes further and its five sums j * out_stride doubles further.
template <typename Lanes>
TC_HD void ti_score_pair(const TiScoreIn& in, int points, long long ident_stride, long long out_stride, TiScoreShared& sh,
                         unsigned* scratch, double* out, int* err, Lanes lanes) {
    tc_score_cells(in.cells, sh, scratch, lanes);
    for (int j = 0; j < points; ++j)
        ti_score_point(in, in.ident + j * ident_stride, sh, scratch, out + j * out_stride, err, lanes);
}

// The chain of a naming call: chain = (t * points + j) * n_files + n.  Point j reads plane j / (points / planes) of the
// stored match (planes divides points: the entry points check it) and threshold delta_id[t * points + j].
struct TiChain {
    int t, j, n, plane;
};
TC_HD TiChain ti_chain(long long chain, int points, int planes, int n_files) {
    const long long tj = chain / n_files;
    TiChain c;
    c.n = (int)(chain - tj * n_files);
    c.t = (int)(tj / points);
    c.j = (int)(tj - (long long)c.t * points);
    c.plane = c.j / (points / planes);
    return c;
}
