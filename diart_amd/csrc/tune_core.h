// The replay of the hyper-parameter tuner over cached model outputs: tc_chain walks one (trial, file)
// chain of clustering steps, tc_row_mask turns the assignments into one packed output row of the tail.  The
// decisions of a step are clu_core.h's, the text dz_clu_step runs too, here on its fixed store (K <= TC_KMAX,
// G <= TC_GMAX, the whole state in LDS); what this file adds is how the lanes of a wavefront share the arithmetic that
// feeds them (each norm and each of the K x G distances summed by ONE lane in the core's order).  The rules of the
// tail are tail_core.h's, the text dz_tail_step runs too: the clipped rows, the Hamming-weighted sum of a row, the
// edge walk of Binarize; what this file adds there is the plan's layout and the merging of the turns.  Host and device
// compile this text: k_tune.hip for the kernels, tune_score.cpp for backend="core", which tests/test_tune_host.py
// holds against dz_clu_step + dz_tail_step.  The track pipelines' half (tc_vad_row and tc_track_pair<Rule>, behind the
// replay: one pair routine for the single threshold and for hysteresis, whose lanes' state maps are DESIGN.md 4.21) is
// k_tune_vad.hip's and dz_tune_vad_host's in the same way, and the scoring of the diarization
// masks (tc_score_*, at the end) is k_tune_score.hip's and dz_tune_score_core's.  Three things are said once for all
// of them: how lanes share a range (tc_lane_steps), how workgroups share the pairs of a scoring call (tc_score_pairs),
// and what a phase over the lanes is on the device (TcDeviceLanes; the host's LanesInTurn is tune_score.cpp's).
#pragma once
#include "../../include/diart_amd.h"
#include "clu_core.h"
#include "tail_core.h"

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

// The hypothesis of packed output row p under one trial: bit g = the aggregated score of global speaker g is
// > tau (the tail's Hamming-weighted sum over the step's buffers divided by the sum of the weights, both
// tail_core.h's; the first chunk's prepended rows are that chunk's own scores).
TC_HD unsigned tc_row_mask(const dz_tune_desc& d, int p, double tau, const signed char* assign /* this trial's */) {
    const int K = d.K, F = d.F, G = d.G;
    const int c = d.row_chunk[p], r = p - d.row_off[c];
    const int* plan = d.plan + (long)c * (4 + d.nwin);
    const int pre = plan[1], nbuf = plan[3];
    const unsigned all = G >= 32 ? 0xffffffffu : ((1u << G) - 1u);
    unsigned out = 0, seen = 0;
    if (r < pre) {
        const int row = tail_clip(plan[2] + r, F - 1);
        for (int k = 0; k < K; ++k) {
            const int g = assign[(long)c * K + k];
            if (g < 0) continue;
            seen |= 1u << g;
            if ((double)d.seg[((long)c * F + row) * K + k] > tau) out |= 1u << g;
        }
    } else {
        const int ra = r - pre, cb0 = c - nbuf + 1;
        double den = 0.0;
        tail_hamming_num(d.seg, d.hamming, F, K, plan + 4, cb0, nbuf, ra, [](long) { return -1; }, &den);
        for (int b = 0; b < nbuf; ++b)
            for (int k = 0; k < K; ++k) {
                const int g = assign[(long)(cb0 + b) * K + k];
                if (g >= 0) seen |= 1u << g;
            }
        for (unsigned m = seen; m; m &= m - 1) {
            const int g = __builtin_ctz(m);
            auto local = [&](long cb) {
                int ks = -1;
                for (int k = 0; k < K; ++k)
                    if (assign[cb * K + k] == g) ks = k;
                return ks;
            };
            const double num = tail_hamming_num(d.seg, d.hamming, F, K, plan + 4, cb0, nbuf, ra, local, nullptr);
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
    if (r < pre) return (double)d.seg[(long)c * F + tail_clip(plan[2] + r, F - 1)];
    double den = 0.0;
    const double num =
        tail_hamming_num(d.seg, d.hamming, F, 1, plan + 4, c - nbuf + 1, nbuf, r - pre, [](long) { return 0; }, &den);
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

// Steps [c_lo, c_hi) of one file, in order.  Row p of the packed rows is active when on(p); a turn runs
// from mid[onset] to mid[first inactive row] (tail_edge_walk: the row after the step's last closes an open turn; mids
// holds rows + 1 values per step), turns no longer than 1e-6 are dropped (Segment.__bool__).  Turns arrive sorted by start (the
// cache checks that the steps' grids are), so Annotation.support(collar) is a running maximum: a turn whose gap to
// `end` is <= 1e-6 or < collar extends the covered span from `end` to its own end (if that is later), any other
// turn opens a new span.  Every turn therefore adds the cells [from, its end cell) with from = the cell of `end`
// or its own start cell, handed to add(from, to): nothing is covered twice.
template <typename On, typename Add>
TC_HD TcVadEnd tc_turn_walk(On on_row, Add add, const int* row_off, const double* mids, const int* mid_cell, double collar,
                            int c_lo, int c_hi, TcVadEnd end) {
    for (int c = c_lo; c < c_hi; ++c) {
        const int p = row_off[c], rows = row_off[c + 1] - p;
        const double* mid = mids + (long)p + c;
        const int* cell = mid_cell + (long)p + c;
        tail_edge_walk(rows, [&](int r) { return on_row(p + r); }, [&](int onset, int r) {
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
                    add(from, to);
                    end.e = e;
                    end.cell = to;
                }
            }
            return true;
        });
    }
    return end;
}

// The durations a turn of a track adds are differences of the file's prefix sums (dur_prefix / ref_prefix: ncell + 1
// values, cell_dur and cell_dur where the reference is active, summed in order).
struct TcVadAdd {
    const double *dur_prefix, *ref_prefix;
    TcVadSum* sum;
    TC_HD void operator()(int from, int to) const {
        sum->hyp += dur_prefix[to] - dur_prefix[from];
        sum->both += ref_prefix[to] - ref_prefix[from];
    }
};
struct TcNoAdd {
    TC_HD void operator()(int, int) const {}
};

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

// How a workgroup of nl lanes shares a file of `chunks` steps from c0 on: lane i walks steps [i * per, (i + 1) * per),
// clipped to the file (a lane behind the last step has lo == hi).  In long long: lane * per passes 2^31 for a file that
// itself fits an int.
struct TcSteps {
    int lo, hi;
};
TC_HD TcSteps tc_lane_steps(int c0, int chunks, int lane, int nl) {
    const long long per = ((unsigned)chunks + (unsigned)nl - 1u) / (unsigned)nl, at = lane * per;   // (a 32-bit quotient)
    const long long lo = at < chunks ? at : chunks, hi = lo + per < chunks ? lo + per : chunks;
    return {c0 + (int)lo, c0 + (int)hi};
}

// ---------------------------------------------------------------------------------------------------------
// One (trial, file) pair of a track pipeline, by the `nl` lanes of one workgroup: tc_track_pair<Rule>.
//
// The rule says whether a row is on: TcPlainRule, agg > tau, or TcHystRule (tail_hyst_on: agg > tau_active while the
// track is off and > tau_offset while it is on; the state is off at a file's first row and is carried across its
// steps).  Under the stateful rule a row depends on the row before it, and a lane that walks steps [i * per,
// (i + 1) * per) does not know the state its first row finds.  It does know what its rows make of either state:
// tc_state_map runs the machine from "off" and from "on" at once over the lane's rows and returns both out-states, two
// bits.  These maps compose (tc_state_apply), a lane without rows is the identity, and the state lane i starts from is
// the lanes 0 .. i - 1 applied in order to "off".  Nothing is approximated: the rule is a function of (state, score),
// every lane applies that function to exactly the rows the sequential walk would, in their order, and composing
// functions is associative; the `on` of every row is therefore the sequential machine's, bit for bit.  The stateless
// rule has no such phase (if constexpr) and no map and start arrays in its shared struct.  With tau_offset ==
// tau_active the stateful rule IS the stateless one, and the two give the same doubles.
//
// Then, for either rule, every lane walks its steps twice (tc_turn_walk): first alone, for the end of its
// latest-ending turn; an exclusive running maximum of those ends over the lanes, strictly greater in lane order
// (-infinity for a lane without a turn, so it carries across any number of empty steps), is "the end of the last turn
// before this lane"; then again from that end, summing the durations its turns add.  Lane 0 adds the lanes' sums in
// lane order and writes the five components.  (TcDurRule, the hysteresis rows with minimum durations, replaces these
// two walks by one walk per lane and a composition of the lanes' summaries: further down, before the routine.)
//
// Written as phases over the lanes, as tc_score_cells is: lanes(f) runs f(lane) for every lane and ends with the
// workgroup's barrier (k_tune_vad.hip), or plays the lanes in order (tune_score.cpp).  `out` (5 components) and `bits`
// (this trial's masks, indexed by packed row) may each be NULL, not both.  No atomics, plain compares.
// ---------------------------------------------------------------------------------------------------------
struct TcPlainRule {   // taus (T,)
    static constexpr bool stateful = false, durations = false;
    double tau;
    static TC_HD TcPlainRule of(const double* taus, int t) { return {taus[t]}; }
    TC_HD bool operator()(double y, bool) const { return y > tau; }
};
struct TcHystRule {    // taus (T, 2) = (tau_active, tau_offset)
    static constexpr bool stateful = true, durations = false;
    double tau_active, tau_offset;
    static TC_HD TcHystRule of(const double* taus, int t) { return {taus[2 * (long)t], taus[2 * (long)t + 1]}; }
    TC_HD bool operator()(double y, bool active) const { return tail_hyst_on(y, tau_active, tau_offset, active); }
};
// taus (T, 4) = (tau_active, tau_offset, min_duration_on, min_duration_off), DESIGN.md 4.22: the rows are TcHystRule's
// (a trial without hysteresis passes tau_offset == tau_active); the durations act on the file's merged spans
struct TcDurRule : TcHystRule {
    static constexpr bool durations = true;
    double min_on, min_off;
    static TC_HD TcDurRule of(const double* taus, int t) {
        const double* q = taus + 4 * (long)t;
        TcDurRule r;
        r.tau_active = q[0];
        r.tau_offset = q[1];
        r.min_on = q[2];
        r.min_off = q[3];
        return r;
    }
};

template <typename Rule>
TC_HD unsigned tc_state_map(const Rule& rule, const double* agg, int p0, int p1) {
    bool from_off = false, from_on = true;
    for (int p = p0; p < p1; ++p) {
        const double y = agg[p];
        from_off = rule(y, from_off);
        from_on = rule(y, from_on);
    }
    return (from_off ? 1u : 0u) | (from_on ? 2u : 0u);
}
TC_HD bool tc_state_apply(unsigned map, bool active) { return (map >> (active ? 1 : 0)) & 1u; }

template <typename Rule>
struct TcTrackOn {   // tc_turn_walk asks for the rows of its steps once each and in order
    const double* agg;
    Rule rule;
    bool* active;
    TC_HD bool operator()(int p) const { return *active = rule(agg[p], *active); }
};

constexpr int TC_TRACK_LANES = 256;   // the workgroup of tune_vad_score_kernel; the host plays at most as many

struct TcTrackIn {
    const double* agg;                        // (total_rows)
    const int* row_off;                       // (chunks + 1)
    const double* mids;                       // rows + 1 frame middles per step
    const int* mid_cell;
    const double *dur_prefix, *ref_prefix;    // THIS file's ncell + 1 prefix sums
    int c0, c1, ncell;
    double collar;
};
template <bool Stateful>
struct TcTrackStates {                        // what the stateful rule keeps per lane; the stateless form carries none
    unsigned char map[TC_TRACK_LANES];        // tc_state_map of every lane's rows
    unsigned char start[TC_TRACK_LANES];      // the state every lane's first row finds
};
template <>
struct TcTrackStates<false> {};
template <bool Stateful>
struct TcTrackShared : TcTrackStates<Stateful> {
    double end_e[TC_TRACK_LANES];
    double sum_hyp[TC_TRACK_LANES], sum_both[TC_TRACK_LANES];
    int end_cell[TC_TRACK_LANES];
};

// ---------------------------------------------------------------------------------------------------------
// Minimum durations (TcDurRule).  The file's turns are merged with the collar max(collar, min_off)
// into spans — Annotation.support: a turn whose gap to the running maximum of the ends is <= 1e-6 or < collar extends
// the span — and a span counts towards hyp / both unless end - start < min_on, both taken from `mids`.  Whether a span
// counts is known only when both its ends are, and a span may cross any number of lanes, so the two walks of the other
// rules do not serve.  Instead every lane reduces its steps, walked alone from "no span", to a summary: no span; or
// its first span, its last span (the same one when it has one) and the sums of the spans strictly between them, which
// no other lane can change.  One lane then composes the summaries in lane order (below, at tc_track_pair's end).
// ---------------------------------------------------------------------------------------------------------
struct TcSpan {
    double s, e;
    int cs, ce;   // the scoring cells that start at s and at e
};

// tc_turn_walk's sibling for whole spans: steps [c_lo, c_hi) from the open span `cur` (if `have`); close(span) for every
// span that a later turn does not join, in order.  Returns whether a span is open at the end, in `cur`.
template <typename On, typename Close>
TC_HD bool tc_span_walk(On on_row, Close close, const int* row_off, const double* mids, const int* mid_cell, double collar,
                        int c_lo, int c_hi, TcSpan& cur, bool have) {
    for (int c = c_lo; c < c_hi; ++c) {
        const int p = row_off[c], rows = row_off[c + 1] - p;
        const double* mid = mids + (long)p + c;
        const int* cell = mid_cell + (long)p + c;
        tail_edge_walk(rows, [&](int r) { return on_row(p + r); }, [&](int onset, int r) {
            const double s = mid[onset], e = mid[r];
            if (e - s > 1e-6) {
                bool joins = false;
                if (have) {
                    const double gap = s - cur.e;
                    joins = gap <= 1e-6 || gap < collar;
                }
                if (joins) {
                    if (e > cur.e) {
                        cur.e = e;
                        cur.ce = cell[r];
                    }
                } else {
                    if (have) close(cur);
                    cur.s = s;
                    cur.e = e;
                    cur.cs = cell[onset];
                    cur.ce = cell[r];
                    have = true;
                }
            }
            return true;
        });
    }
    return have;
}

struct TcSpanCount {   // a closed span counts unless it is shorter than min_on (strictly)
    const double *dur_prefix, *ref_prefix;
    double min_on;
    TcVadSum* sum;
    TC_HD void operator()(const TcSpan& u) const {
        if (u.e - u.s < min_on) return;
        sum->hyp += dur_prefix[u.ce] - dur_prefix[u.cs];
        sum->both += ref_prefix[u.ce] - ref_prefix[u.cs];
    }
};

struct TcDurShared : TcTrackStates<true> {    // the lanes' summaries (17.5 KB)
    double first_s[TC_TRACK_LANES], first_e[TC_TRACK_LANES], last_s[TC_TRACK_LANES], last_e[TC_TRACK_LANES];
    double mid_hyp[TC_TRACK_LANES], mid_both[TC_TRACK_LANES];
    int first_cs[TC_TRACK_LANES], first_ce[TC_TRACK_LANES], last_cs[TC_TRACK_LANES], last_ce[TC_TRACK_LANES];
    int spans[TC_TRACK_LANES];                // 0, 1, or 2: two or more
};
template <typename Rule, bool Durations = Rule::durations>
struct TcTrackSharedFor {
    using type = TcTrackShared<Rule::stateful>;
};
template <typename Rule>
struct TcTrackSharedFor<Rule, true> {
    using type = TcDurShared;
};
template <typename Rule>
using TcTrackSharedOf = typename TcTrackSharedFor<Rule>::type;

// One lane's steps, walked alone, as a summary.
template <typename Rule>
TC_HD void tc_span_summary(const TcTrackIn& in, const Rule& rule, double collar, TcSteps my, bool start, TcDurShared& sh,
                           int lane) {
    TcVadSum mid = {0.0, 0.0};
    const TcSpanCount count = {in.dur_prefix, in.ref_prefix, rule.min_on, &mid};
    TcSpan first = {0.0, 0.0, 0, 0}, cur = {0.0, 0.0, 0, 0};
    int closed = 0;
    bool active = start;
    const bool open = tc_span_walk(TcTrackOn<Rule>{in.agg, rule, &active}, [&](const TcSpan& u) {
        if (closed++ == 0)
            first = u;
        else
            count(u);
    }, in.row_off, in.mids, in.mid_cell, collar, my.lo, my.hi, cur, false);
    if (closed == 0) first = cur;   // (a span closes only because another opens: with none open, none closed either)
    sh.spans[lane] = !open ? 0 : closed == 0 ? 1 : 2;
    sh.first_s[lane] = first.s;
    sh.first_e[lane] = first.e;
    sh.first_cs[lane] = first.cs;
    sh.first_ce[lane] = first.ce;
    sh.last_s[lane] = cur.s;
    sh.last_e[lane] = cur.e;
    sh.last_cs[lane] = cur.cs;
    sh.last_ce[lane] = cur.ce;
    sh.mid_hyp[lane] = mid.hyp;
    sh.mid_both[lane] = mid.both;
}

// The summaries composed in lane order by one lane: the sequential walk of the whole file, lane by lane.  `cur` is the
// open span — its end is the running maximum of every end so far.  Lane j's summary was formed from "no span"; the
// sequential walk enters lane j with `cur`.  The lane's first span consists of turns that join each other against the
// lane's own running maximum; against a maximum that is no smaller they join all the more, so the sequential walk
// merges them too, into `cur` if the first of them joins it and into a span of their own otherwise, and leaves the
// maximum at max(cur.e, first.e).  Where that is first.e, the walk goes on exactly as the lane did alone: the spans
// between count as summed, the last stays open.  Where cur.e is greater — a turn of an earlier lane ends behind the
// lane's whole first span — and the lane has further spans, those may join `cur` as well: that lane is walked again
// here, from `cur` and the state its first row finds.  (Step grids sorted by time and of one resolution never get
// there.)  The sums are added in this order on every run; compares are the walk's own.
template <typename Rule>
TC_HD TcVadSum tc_span_compose(const TcTrackIn& in, const Rule& rule, double collar, const TcDurShared& sh, int nl) {
    TcVadSum all = {0.0, 0.0};
    const TcSpanCount count = {in.dur_prefix, in.ref_prefix, rule.min_on, &all};
    const int chunks = in.c1 - in.c0;
    TcSpan cur = {0.0, 0.0, 0, 0};
    bool have = false;
    for (int j = 0; j < nl; ++j) {
        const int n = sh.spans[j];
        if (!n) continue;
        const TcSpan first = {sh.first_s[j], sh.first_e[j], sh.first_cs[j], sh.first_ce[j]};
        bool joins = false;
        if (have) {
            const double gap = first.s - cur.e;
            joins = gap <= 1e-6 || gap < collar;
        }
        if (joins && n > 1 && cur.e > first.e) {
            const TcSteps my = tc_lane_steps(in.c0, chunks, j, nl);
            bool active = sh.start[j] != 0;
            have = tc_span_walk(TcTrackOn<Rule>{in.agg, rule, &active}, count, in.row_off, in.mids, in.mid_cell, collar, my.lo,
                                my.hi, cur, true);
            continue;
        }
        if (joins) {
            if (first.e > cur.e) {
                cur.e = first.e;
                cur.ce = first.ce;
            }
        } else {
            if (have) count(cur);
            cur = first;
            have = true;
        }
        if (n > 1) {
            count(cur);
            all.hyp += sh.mid_hyp[j];
            all.both += sh.mid_both[j];
            cur.s = sh.last_s[j];
            cur.e = sh.last_e[j];
            cur.cs = sh.last_cs[j];
            cur.ce = sh.last_ce[j];
        }
    }
    if (have) count(cur);
    return all;
}

template <typename Rule, typename Lanes>
TC_HD void tc_track_pair(const TcTrackIn& in, const Rule rule, TcTrackSharedOf<Rule>& sh, double* out, unsigned* bits,
                         Lanes lanes) {
    const int nl = lanes.nl, chunks = in.c1 - in.c0;
    [[maybe_unused]] const TcVadEnd none = {-INFINITY, 0};
    // ---- every lane's state map
    if constexpr (Rule::stateful)
        lanes([&](int lane) {
            const TcSteps my = tc_lane_steps(in.c0, chunks, lane, nl);
            sh.map[lane] = (unsigned char)tc_state_map(rule, in.agg, in.row_off[my.lo], in.row_off[my.hi]);
        });
    // ---- the maps composed in lane order; the masks; alone, the end of the lane's latest-ending turn
    lanes([&](int lane) {
        const TcSteps my = tc_lane_steps(in.c0, chunks, lane, nl);
        bool start = false;
        if constexpr (Rule::stateful) {
            for (int j = 0; j < lane; ++j) start = tc_state_apply(sh.map[j], start);
            sh.start[lane] = start ? 1 : 0;
        }
        if (bits) {
            bool active = start;
            for (int p = in.row_off[my.lo], p1 = in.row_off[my.hi]; p < p1; ++p) {
                active = rule(in.agg[p], active);
                bits[p] = active ? 1u : 0u;
            }
        }
        if (!out) return;
        if constexpr (Rule::durations) {
            tc_span_summary(in, rule, in.collar > rule.min_off ? in.collar : rule.min_off, my, start, sh, lane);
        } else {
            bool active = start;
            const TcVadEnd own = tc_turn_walk(TcTrackOn<Rule>{in.agg, rule, &active}, TcNoAdd{}, in.row_off, in.mids,
                                              in.mid_cell, in.collar, my.lo, my.hi, none);
            sh.end_e[lane] = own.e;
            sh.end_cell[lane] = own.cell;
        }
    });
    if (!out) return;
    if constexpr (Rule::durations) {
        // ---- one lane composes the summaries in lane order and writes the five components
        lanes([&](int lane) {
            if (lane != 0) return;
            const double collar = in.collar > rule.min_off ? in.collar : rule.min_off;
            tc_vad_components(in.ref_prefix[in.ncell], tc_span_compose(in, rule, collar, sh, nl), out);
        });
    } else {
    // ---- again from the end of the last turn before the lane, summing what its turns add
    lanes([&](int lane) {
        const TcSteps my = tc_lane_steps(in.c0, chunks, lane, nl);
        TcVadEnd before = none;
        for (int j = 0; j < lane; ++j)
            if (sh.end_e[j] > before.e) {
                before.e = sh.end_e[j];
                before.cell = sh.end_cell[j];
            }
        TcVadSum s = {0.0, 0.0};
        bool active = false;
        if constexpr (Rule::stateful) active = sh.start[lane] != 0;
        tc_turn_walk(TcTrackOn<Rule>{in.agg, rule, &active}, TcVadAdd{in.dur_prefix, in.ref_prefix, &s}, in.row_off, in.mids,
                     in.mid_cell, in.collar, my.lo, my.hi, before);
        sh.sum_hyp[lane] = s.hyp;
        sh.sum_both[lane] = s.both;
    });
    lanes([&](int lane) {
        if (lane != 0) return;
        TcVadSum all = {0.0, 0.0};
        for (int j = 0; j < nl; ++j) {
            all.hyp += sh.sum_hyp[j];
            all.both += sh.sum_both[j];
        }
        tc_vad_components(in.ref_prefix[in.ncell], all, out);
    });
    }
}

// ---------------------------------------------------------------------------------------------------------
// SpeakerDiarization: the diarization error rate components of one (trial, file) from the trial's packed masks
// (bit g of a row = global speaker g is active), as dz_tune_score forms them, by the `nl` lanes of one workgroup.
//
// Turns and their merging are tc_turn_walk's, per label: lane i walks steps [i * per, (i + 1) * per) twice, as
// tc_track_pair does (alone for the end of its latest-ending turn, then from the running maximum of the
// lanes before it).  The covered ranges of one label are disjoint, so a range [from, to) is recorded by toggling
// bit g of words `from` and `to` of the pair's scratch slice (ncell + 1 words, integer atomic XOR); a prefix XOR
// over the words then IS the hypothesis mask of every scoring cell.  Every sum over the cells is formed per lane
// (lane l takes cells l, l + nl, ...) and the lanes' sums are added in lane order by one lane: the same doubles on
// every run, and no floating-point atomic anywhere.  The co-occurrence matrix is formed TC_SCORE_SWEEP entries at
// a time (that many accumulators per lane, statically indexed); lane 0 solves the mapping (tc_lsap on -cooc).
// What differs from dz_tune_score is the order of these sums, nothing else.
//
// The text is written as phases over the lanes: lanes(f) runs f(lane) for every lane and ends with the workgroup's
// barrier (k_tune_score.hip), or plays the lanes one after the other (dz_tune_score_core).  Nothing in
// TcScoreShared or in the scratch slice is read before this pair has written it: LDS holds whatever was there, and
// the slice holds the hypothesis of the pair this workgroup took before.
// ---------------------------------------------------------------------------------------------------------
struct CluMapping {   // the store of the mapping problem: up to TC_GMAX hypothesis x 64 reference labels
    template <typename T> using PerK = T[TC_GMAX];
    template <typename T> using PerG = T[64];
    template <typename T> using PerKG = T[TC_GMAX * 64];
    using Active = CluMask32;
    using Index = int;
    static constexpr int err(int) { return 3; }
};

constexpr int TC_SCORE_LANES = 256;   // the workgroup of tune_score_kernel; dz_tune_score_core plays at most as many
constexpr int TC_SCORE_SWEEP = 8;     // co-occurrence entries per pass over the cells
// dz_tune_score's return codes
constexpr int TC_SCORE_ERR_ARGS = 2;    // a file with more cells than a scratch slice holds
constexpr int TC_SCORE_ERR_MAP = 3;     // the mapping's assignment problem failed
constexpr int TC_SCORE_ERR_CELLS = 4;   // a speech turn does not start and end on the file's scoring cells

// The words of a scratch slice are toggled with device-scope atomics, which act in L2: every other access to them
// goes there too (relaxed, device scope), so that no lane reads a line its CU cached before the toggles.
TC_HD unsigned tc_word_load(const unsigned* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(const_cast<unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
TC_HD void tc_word_store(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p = v;
#endif
}
TC_HD void tc_word_xor(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_xor(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p ^= v;
#endif
}
TC_HD void tc_err_raise(int* err, int code) {   // the call's error word: the largest code any pair met
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_max(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (*err < code) *err = code;
#endif
}

struct TcScoreIn {
    const unsigned* bits;                 // this trial's masks (total_rows)
    const int* row_off;                   // (chunks + 1) the packed rows of every step
    const double* mids;                   // rows + 1 frame middles per step
    const int* mid_cell;                  // the file's cell that starts at each of them
    const double* cell_dur;               // the file's cells: duration
    const unsigned long long* cell_ref;   //                   reference speakers
    int c0, c1, ncell, G;
    double collar;
};

struct TcScoreShared {
    double cost[TC_GMAX * 64];            // -cooc of (hypothesis label a, reference label b) at a * nr + b
    TcLsapWork<CluMapping> work;
    double part[TC_SCORE_SWEEP][TC_SCORE_LANES];   // the lanes' partial sums
    double end_e[TC_SCORE_LANES];
    unsigned long long lane_ref[TC_SCORE_LANES];
    int end_cell[TC_SCORE_LANES];
    unsigned lane_any[TC_SCORE_LANES];    // the labels in a lane's steps
    unsigned lane_x[TC_SCORE_LANES];      // the XOR of a lane's block of words; then the labels in a lane's cells
    double sums[4];                       // total, missed, false alarm, sum dur x min(Nref, Nhyp)
    int hl[TC_GMAX], rl[64], raw[64], col[TC_GMAX];
    int nh, nr, err;
};

// The pairs of one scoring call as its `blocks` workgroups share them: workgroup `block` takes pairs block,
// block + blocks, ... and hands score(pair, t, cell0, in) each of them with the pair's slice of the call's arrays.  A
// file with more cells than a scratch slice holds is skipped and raises TC_SCORE_ERR_ARGS (`raises`: one lane's job).
struct TcScoreCall {
    const unsigned* bits;                 // (trials, total_rows)
    int trials, n_files, total_rows;
    const int *file_chunk_off, *row_off;
    const double* mids;
    const int *mid_cell, *file_cell_off;
    const double* cell_dur;
    const unsigned long long* cell_ref;
    int max_cells, max_speakers;
    double collar;
};
template <typename Score>
TC_HD void tc_score_pairs(const TcScoreCall& c, int block, int blocks, bool raises, int* err, Score score) {
    const long long pairs = (long long)c.trials * c.n_files;
    for (long long pair = block; pair < pairs; pair += blocks) {
        const int t = (int)(pair / c.n_files), n = (int)(pair - (long long)t * c.n_files);
        const int cell0 = c.file_cell_off[n], ncell = c.file_cell_off[n + 1] - cell0;
        if (ncell < 0 || ncell > c.max_cells) {   // (the same for every lane) the file does not fit a slice
            if (raises) tc_err_raise(err, TC_SCORE_ERR_ARGS);
            continue;
        }
        const TcScoreIn in = {c.bits + (long long)t * c.total_rows, c.row_off, c.mids, c.mid_cell, c.cell_dur + cell0,
                              c.cell_ref + cell0, c.file_chunk_off[n], c.file_chunk_off[n + 1], ncell, c.max_speakers, c.collar};
        score(pair, t, cell0, in);
    }
}

// dz_tune_cells, the geometry as it crosses the C boundary (host side of every entry, device pointers or host ones).
// The members an entry reads, one bit per pointer in declaration order, and the sets that several entries share.
enum : unsigned {
    TC_CELLS_FILE_CHUNK_OFF = 1u << 0, TC_CELLS_FILE_ROW_OFF = 1u << 1, TC_CELLS_ROW_OFF = 1u << 2,
    TC_CELLS_STEP_ROWS = 1u << 3, TC_CELLS_MIDS = 1u << 4, TC_CELLS_MID_CELL = 1u << 5, TC_CELLS_FILE_CELL_OFF = 1u << 6,
    TC_CELLS_CELL_DUR = 1u << 7, TC_CELLS_CELL_REF = 1u << 8, TC_CELLS_CELL_STEP = 1u << 9, TC_CELLS_DUR_PREFIX = 1u << 10,
    TC_CELLS_REF_PREFIX = 1u << 11,
    TC_CELLS_GRID = TC_CELLS_MIDS | TC_CELLS_MID_CELL | TC_CELLS_FILE_CELL_OFF,
    TC_CELLS_REFERENCE = TC_CELLS_CELL_DUR | TC_CELLS_CELL_REF,
    TC_CELLS_SEQUENTIAL = TC_CELLS_FILE_ROW_OFF | TC_CELLS_FILE_CHUNK_OFF | TC_CELLS_STEP_ROWS | TC_CELLS_GRID | TC_CELLS_REFERENCE,
    TC_CELLS_KERNEL = TC_CELLS_FILE_CHUNK_OFF | TC_CELLS_ROW_OFF | TC_CELLS_GRID | TC_CELLS_REFERENCE,
    TC_CELLS_TRACK_PAIR = TC_CELLS_GRID | TC_CELLS_DUR_PREFIX | TC_CELLS_REF_PREFIX,
    TC_CELLS_TRACK = TC_CELLS_FILE_CHUNK_OFF | TC_CELLS_ROW_OFF | TC_CELLS_TRACK_PAIR,
};
// The first of the `need`ed members that is NULL, by name (the descriptor itself when there is none), or nullptr.
inline const char* tc_cells_missing(const dz_tune_cells* c, unsigned need) {
    if (!c) return "cells";
    const void* const ptr[12] = {c->file_chunk_off, c->file_row_off, c->row_off,   c->step_rows, c->mids,       c->mid_cell,
                                 c->file_cell_off,  c->cell_dur,     c->cell_ref,  c->cell_step, c->dur_prefix, c->ref_prefix};
    static const char* const name[12] = {"cells->file_chunk_off", "cells->file_row_off", "cells->row_off",    "cells->step_rows",
                                         "cells->mids",           "cells->mid_cell",     "cells->file_cell_off", "cells->cell_dur",
                                         "cells->cell_ref",       "cells->cell_step",    "cells->dur_prefix", "cells->ref_prefix"};
    for (int i = 0; i < 12; ++i)
        if (((need >> i) & 1u) && !ptr[i]) return name[i];
    return nullptr;
}
inline TcScoreCall tc_score_call(const dz_tune_cells& c, const unsigned* bits, int trials) {
    return {bits,       trials,          c.n_files,  c.total_rows, c.file_chunk_off, c.row_off,      c.mids,
            c.mid_cell, c.file_cell_off, c.cell_dur, c.cell_ref,   c.max_cells,      c.max_speakers, c.collar};
}

#if defined(TC_KERNEL_UNIT)   // the kernels' translation units define it before this header: threadIdx, the barrier
// The lanes of a phase on the device: every thread of the workgroup is one, and the phase ends with the barrier.
struct TcDeviceLanes {
    int nl;
    template <typename F>
    __device__ void operator()(F f) const {
        f((int)threadIdx.x);
        __syncthreads();
    }
};
#endif

struct TcBitOn {
    const unsigned* bits;
    int g;
    TC_HD bool operator()(int p) const { return (bits[p] >> g) & 1u; }
};
struct TcToggle {
    unsigned* scratch;
    unsigned bit;
    int ncell;
    int* err;
    TC_HD void operator()(int from, int to) const {
        if (from < 0 || to > ncell || from > to) {   // dz_tune_score's rc 4, before any word is touched
            *err = TC_SCORE_ERR_CELLS;
            return;
        }
        tc_word_xor(scratch + from, bit);
        tc_word_xor(scratch + to, bit);
    }
};

// str(a) < str(b) for label numbers below 100: "10" < "2" (metrics.optimal_mapping sorts the labels as strings)
TC_HD bool tc_str_less(int a, int b) {
    const int a0 = a >= 10 ? a / 10 : a, b0 = b >= 10 ? b / 10 : b;
    if (a0 != b0) return a0 < b0;
    const int a1 = a >= 10 ? a % 10 : -1, b1 = b >= 10 ? b % 10 : -1;   // -1: the string ends here
    return a1 < b1;
}

// The first half of a pair, which the identification scoring shares (tune_ident_core.h): after it word i of the slice
// is the hypothesis mask of scoring cell i, and sh.err says whether a turn left the file's cells.  `Shared` has
// lane_any, lane_x, end_e, end_cell (one per lane) and err.
template <typename Shared, typename Lanes>
TC_HD void tc_score_cells(const TcScoreIn& in, Shared& sh, unsigned* scratch, Lanes lanes) {
    const int nl = lanes.nl, ncell = in.ncell, chunks = in.c1 - in.c0;
    const unsigned gmask = in.G >= 32 ? 0xffffffffu : ((1u << in.G) - 1u);   // dz_tune_score ignores bits >= G
    const TcVadEnd none = {-INFINITY, 0};
    // ---- the slice starts from zeros; the labels of every lane's steps
    lanes([&](int lane) {
        for (int i = lane; i <= ncell; i += nl) tc_word_store(scratch + i, 0u);
        const TcSteps my = tc_lane_steps(in.c0, chunks, lane, nl);
        unsigned any = 0;
        for (int p = in.row_off[my.lo], p1 = in.row_off[my.hi]; p < p1; ++p) any |= in.bits[p];
        sh.lane_any[lane] = any & gmask;
        if (lane == 0) sh.err = 0;
    });
    unsigned any = 0;
    for (int j = 0; j < nl; ++j) any |= sh.lane_any[j];
    // ---- per label: the merged turns toggle the words at which they start and end
    for (unsigned m = any; m; m &= m - 1) {
        const int g = __builtin_ctz(m);
        lanes([&](int lane) {
            const TcSteps my = tc_lane_steps(in.c0, chunks, lane, nl);
            TcVadEnd own = none;
            if ((sh.lane_any[lane] >> g) & 1u)
                own = tc_turn_walk(TcBitOn{in.bits, g}, TcNoAdd{}, in.row_off, in.mids, in.mid_cell, in.collar, my.lo, my.hi,
                                   none);
            sh.end_e[lane] = own.e;
            sh.end_cell[lane] = own.cell;
        });
        lanes([&](int lane) {
            if (!((sh.lane_any[lane] >> g) & 1u)) return;   // no turn of g in this lane's steps: nothing to add
            const TcSteps my = tc_lane_steps(in.c0, chunks, lane, nl);
            TcVadEnd before = none;
            for (int j = 0; j < lane; ++j)
                if (sh.end_e[j] > before.e) {
                    before.e = sh.end_e[j];
                    before.cell = sh.end_cell[j];
                }
            tc_turn_walk(TcBitOn{in.bits, g}, TcToggle{scratch, 1u << g, ncell, &sh.err}, in.row_off, in.mids, in.mid_cell,
                         in.collar, my.lo, my.hi, before);
        });
    }
    // ---- prefix XOR: word i becomes the hypothesis mask of cell i (lane l scans the block [l * blk, (l + 1) * blk))
    lanes([&](int lane) {
        const TcSteps my = tc_lane_steps(0, ncell, lane, nl);
        unsigned x = 0;
        for (int i = my.lo; i < my.hi; ++i) x ^= tc_word_load(scratch + i);
        sh.lane_x[lane] = x;
    });
    lanes([&](int lane) {
        unsigned carry = 0;
        for (int j = 0; j < lane; ++j) carry ^= sh.lane_x[j];
        const TcSteps my = tc_lane_steps(0, ncell, lane, nl);
        for (int i = my.lo; i < my.hi; ++i) {
            carry ^= tc_word_load(scratch + i);
            tc_word_store(scratch + i, carry);
        }
    });
}

template <typename Lanes>
TC_HD void tc_score_pair(const TcScoreIn& in, TcScoreShared& sh, unsigned* scratch, double* out /* 5 */, int* err,
                         Lanes lanes) {
    const int nl = lanes.nl, ncell = in.ncell;
    tc_score_cells(in, sh, scratch, lanes);
    // ---- the components over the cells, per lane
    lanes([&](int lane) {
        double total = 0.0, missed = 0.0, fa = 0.0, both = 0.0;
        unsigned hseen = 0;
        unsigned long long rseen = 0;
        for (int i = lane; i < ncell; i += nl) {
            const unsigned h = tc_word_load(scratch + i);
            const unsigned long long rm = in.cell_ref[i];
            if (!h && !rm) continue;
            const double dur = in.cell_dur[i];
            const int nref = __builtin_popcountll(rm), nhyp = __builtin_popcount(h);
            total += dur * nref;
            missed += dur * (nref > nhyp ? nref - nhyp : 0);
            fa += dur * (nhyp > nref ? nhyp - nref : 0);
            both += dur * (nref < nhyp ? nref : nhyp);
            hseen |= h;
            rseen |= rm;
        }
        sh.part[0][lane] = total;
        sh.part[1][lane] = missed;
        sh.part[2][lane] = fa;
        sh.part[3][lane] = both;
        sh.lane_x[lane] = hseen;
        sh.lane_ref[lane] = rseen;
    });
    // ---- lane 0: the lanes' sums in lane order; the labels (hypothesis in str order, reference in bit order)
    lanes([&](int lane) {
        if (lane != 0) return;
        unsigned hseen = 0;
        unsigned long long rseen = 0;
        for (int q = 0; q < 4; ++q) {
            double s = 0.0;
            for (int j = 0; j < nl; ++j) s += sh.part[q][j];
            sh.sums[q] = s;
        }
        for (int j = 0; j < nl; ++j) {
            hseen |= sh.lane_x[j];
            rseen |= sh.lane_ref[j];
        }
        int nh = 0, nr = 0;
        for (int g = 0; g < in.G; ++g)
            if ((hseen >> g) & 1u) {
                int p = nh++;
                while (p > 0 && tc_str_less(g, sh.hl[p - 1])) {
                    sh.hl[p] = sh.hl[p - 1];
                    --p;
                }
                sh.hl[p] = g;
            }
        for (int r = 0; r < 64; ++r)
            if ((rseen >> r) & 1ull) sh.rl[nr++] = r;
        sh.nh = nh;
        sh.nr = nr;
    });
    // ---- cooc[a][b] = the duration in which hypothesis label hl[a] and reference label rl[b] are both active
    const int nh = sh.nh, nr = sh.nr, nent = nh * nr;
    for (int e0 = 0; e0 < nent; e0 += TC_SCORE_SWEEP) {
        lanes([&](int lane) {
            unsigned hm[TC_SCORE_SWEEP];
            unsigned long long rk[TC_SCORE_SWEEP];
            double acc[TC_SCORE_SWEEP];
#pragma unroll
            for (int j = 0; j < TC_SCORE_SWEEP; ++j) {
                const int e = e0 + j < nent ? e0 + j : 0;
                hm[j] = e0 + j < nent ? 1u << sh.hl[e / nr] : 0u;
                rk[j] = e0 + j < nent ? 1ull << sh.rl[e - (e / nr) * nr] : 0ull;
                acc[j] = 0.0;
            }
            for (int i = lane; i < ncell; i += nl) {
                const unsigned h = tc_word_load(scratch + i);
                const unsigned long long rm = in.cell_ref[i];
                if (!h || !rm) continue;
                const double dur = in.cell_dur[i];
#pragma unroll
                for (int j = 0; j < TC_SCORE_SWEEP; ++j) acc[j] += ((h & hm[j]) && (rm & rk[j])) ? dur : 0.0;   // (x + 0.0 is x)
            }
#pragma unroll
            for (int j = 0; j < TC_SCORE_SWEEP; ++j) sh.part[j][lane] = acc[j];
        });
        lanes([&](int lane) {
            if (lane >= TC_SCORE_SWEEP || e0 + lane >= nent) return;
            double s = 0.0;
            for (int j = 0; j < nl; ++j) s += sh.part[lane][j];
            sh.cost[e0 + lane] = -s;
        });
    }
    // ---- lane 0: metrics.optimal_mapping (LSAP on -cooc, pairs with cooc > 0 kept), the five components
    lanes([&](int lane) {
        if (lane != 0) return;
        double correct = 0.0;
        if (nh > 0 && nr > 0) {
            int nraw = 0;
            if (tc_lsap(sh.cost, nh, nr, sh.raw, &nraw, sh.work)) {
                sh.err = TC_SCORE_ERR_MAP;
            } else {
                // raw holds the columns of the pairs sorted by row: every row has one, or (nr < nh) their rows are work.pr
                for (int a = 0; a < nh; ++a) sh.col[a] = -1;
                for (int i = 0; i < nraw; ++i) sh.col[nr < nh ? sh.work.pr[i] : i] = sh.raw[i];
                for (int a = 0; a < nh; ++a)
                    if (sh.col[a] >= 0 && -sh.cost[a * nr + sh.col[a]] > 0.0) correct += -sh.cost[a * nr + sh.col[a]];
            }
        }
        if (sh.err) {
            tc_err_raise(err, sh.err);
            return;
        }
        out[0] = sh.sums[0];   // metrics.COMPONENTS order
        out[1] = correct;
        out[2] = sh.sums[2];
        out[3] = sh.sums[1];
        out[4] = sh.sums[3] - correct;
    });
}
