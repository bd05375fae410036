// Host side of the hyper-parameter tuner:
//
//   dz_tune_plan         what the output tail (Hamming aggregation, "loose" cropping) does at every step of a file that
//                        does not depend on the scores: rows, buffers, cropped rows, the first-chunk prepend.  A loop
//                        over tail_core.h's tail_geometry, the function dz_tail_step calls over its own buffers
//   dz_tune_replay_host  T x N (trial, file) chains on host threads, either through the existing handles (dz_clu_step ->
//                        dz_tail_step: the yardstick of the GPU kernels and the backend of a machine without a GPU) or
//                        through tune_core.h, the text the kernels are compiled from (the clustering decisions are
//                        clu_core.h's either way: on the handles' heap store or on the kernels' fixed one)
//   dz_tune_score        diarization error rate components of every pair from the packed frame masks
//                        (diart_amd/metrics.py DiarizationErrorRate, collar 0, overlap included; PredictionAccumulator's
//                        gap merging), without building an Annotation
//   dz_tune_score_core   the same components from the text tune_score_kernel compiles (k_tune_score.hip), the lanes of its
//                        workgroup played one after the other: scoring="device" on backend="core"
//   dz_tune_vad_host     VoiceActivityDetection: the aggregated speech scores, the masks and (backend="core") the
//                        scoring of k_tune_vad.hip, from the text those kernels compile; OverlappedSpeechDetection
//                        too (both track pipelines: another track, other reference prefix sums).  With an offset
//                        threshold (hysteresis) and with minimum durations: one implementation, another row rule
//   dz_tune_vad_replay_tails  its yardstick: the masks through dz_tail_create + dz_tail_set_offset + dz_tail_step
//   dz_tune_name_host    the names a gallery gives the global speakers of every (trial, point, file) chain, step by step,
//                        from the text tune_name_kernel compiles (tune_ident_core.h)
//   dz_tune_ident_score  identification error rate components of every pair: dz_tune_score's cells, the labels compared
//                        as they are;  dz_tune_ident_score_core: the same from the text of tune_ident_score_kernel, at
//                        several (plane, threshold) points per trial
// The scoring geometry reaches every entry as one descriptor, dz_tune_cells (include/diart_amd.h).
#include "tune_core.h"
#include "tune_ident_core.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "hostpool.h"

void dz_set_error(const char* fmt, ...);

namespace {

struct NoBarrier {
    void operator()() const {}
};

struct LanesInTurn {   // the lanes of a workgroup, one after the other: a phase ends when the last lane has run it
    int nl;
    template <typename F>
    void operator()(F f) const {
        for (int lane = 0; lane < nl; ++lane) f(lane);
    }
};

// fn(worker, i) for i in [0, n) on at most `threads` threads (1 .. n of them); in order, on the caller's, when that is one
template <typename F>
void each_item(int n, int threads, F fn) {
    const int nt = dz_host_threads(threads, n);
    if (nt == 1)
        for (int i = 0; i < n; ++i) fn(0, i);
    else
        dz_host_parallel(n, nt, fn);
}

// The workgroups of a scoring call on the host (dz_tune_score_core, dz_tune_ident_score_core).  As on the device,
// "workgroup" b of score_blocks takes pairs b, b + score_blocks, ... (tc_score_pairs) on one scratch slice of
// max_cells + 1 words, which every pair finds as the pair before left it; the shared state starts from a pattern, as
// LDS starts from whatever was there.  score(in, shared, slice, pair, t, cell0, err) scores one pair; returns the
// largest code a workgroup's error word holds.
template <typename Shared, typename Score>
int score_core(const TcScoreCall& call, int score_blocks, int num_threads, Score score) {
    const long long pairs = (long long)call.trials * call.n_files;
    const int blocks = (int)(pairs < score_blocks ? pairs : score_blocks);
    std::vector<int> errs(blocks, 0);
    each_item(blocks, num_threads, [&](int, int b) {
        std::vector<unsigned> slice((size_t)call.max_cells + 1, 0xa5a5a5a5u);
        std::vector<Shared> sh(1);
        tc_score_pairs(call, b, blocks, true, &errs[b], [&](long long pair, int t, int cell0, const TcScoreIn& in) {
            std::memset(sh.data(), (pair & 1) ? 0x7f : 0xff, sizeof(Shared));
            score(in, sh[0], slice.data(), pair, t, cell0, &errs[b]);
        });
    });
    return *std::max_element(errs.begin(), errs.end());
}

struct Turn {
    double s, e;
    int is, ie;   // the cells that start at s and at e
};

struct ScoreScratch {
    std::vector<Turn> turns[TC_GMAX];
    std::vector<unsigned> hyp;
};

// The hypothesis mask of every scoring cell of file n from one trial's masks B (dz_tune_score and
// dz_tune_ident_score): Binarize's turns per step and speaker, Annotation.support(collar) per speaker, then the cells
// each merged turn covers.  Returns 4 when a turn does not start and end on the file's cells.
int hyp_cells(ScoreScratch& sc, const unsigned* B, int n, const dz_tune_cells& cells, int ncell) {
    const int G = cells.max_speakers;
    const double collar = cells.collar;
    int rc = 0;
    for (int g = 0; g < G; ++g) sc.turns[g].clear();
    // ---- Binarize (tail_edge_walk): per step and speaker, [middle(onset), middle(first inactive row))
    int p = cells.file_row_off[n];
    for (int c = cells.file_chunk_off[n]; c < cells.file_chunk_off[n + 1]; ++c) {
        const int rows = cells.step_rows[c];
        const double* mid = cells.mids + (size_t)p + c;      // rows + 1 values
        const int* cell = cells.mid_cell + (size_t)p + c;
        unsigned any = 0;
        for (int r = 0; r < rows; ++r) any |= B[p + r];
        for (unsigned m = any; m; m &= m - 1) {
            const int g = __builtin_ctz(m);
            if (g >= G) break;
            tail_edge_walk(rows, [&](int r) { return (B[p + r] >> g) & 1u; }, [&](int onset, int r) {
                if (mid[r] - mid[onset] > 1e-6)   // Segment.__bool__: shorter segments are not stored
                    sc.turns[g].push_back(Turn{mid[onset], mid[r], cell[onset], cell[r]});
                return true;
            });
        }
        p += rows;
    }
    // ---- Annotation.support(collar) per speaker, then the cells each merged turn covers
    sc.hyp.assign((size_t)ncell, 0u);
    for (int g = 0; g < G; ++g) {
        std::vector<Turn>& tv = sc.turns[g];
        if (tv.empty()) continue;
        std::sort(tv.begin(), tv.end(), [](const Turn& a, const Turn& b) { return a.s < b.s || (a.s == b.s && a.e < b.e); });
        Turn cur = tv[0];
        auto flush = [&](const Turn& u) {
            if (u.is < 0 || u.ie > ncell || u.is > u.ie) {
                rc = 4;
                return;
            }
            for (int i = u.is; i < u.ie; ++i) sc.hyp[i] |= 1u << g;
        };
        for (size_t i = 1; i < tv.size(); ++i) {
            const double gap = tv[i].s - cur.e;
            if (gap <= 1e-6 || gap < collar) {
                if (tv[i].e > cur.e) {
                    cur.e = tv[i].e;
                    cur.ie = tv[i].ie;
                }
            } else {
                flush(cur);
                cur = tv[i];
            }
        }
        flush(cur);
    }
    return rc;
}

// What every entry that takes the scoring geometry refuses first: a NULL among the members it reads (`need`,
// tune_core.h) or among its own arrays (`rest`: all of them non-NULL).  `who` is the entry.
int check_cells(const char* who, const dz_tune_cells* cells, unsigned need, bool rest) {
    const char* missing = tc_cells_missing(cells, need);
    if (missing || !rest) {
        dz_set_error("%s: NULL argument (%s)", who, missing ? missing : "an array of the call");
        return 2;
    }
    return 0;
}

}  // namespace

extern "C" int dz_tune_cells_abi_size(void) { return (int)sizeof(dz_tune_cells); }

extern "C" int dz_tune_plan(int chunks, int frames, double step, double latency, const double* starts,
                            const double* resolution, int* plan, double* t0_out, double* res_out) {
    if (chunks < 1 || frames < 1 || !(step > 0.0) || !(latency >= step) || !starts || !resolution || !plan || !t0_out ||
        !res_out) {
        dz_set_error("dz_tune_plan: bad arguments (latency must be >= step)");
        return 2;
    }
    const int nwin = (int)nearbyint(latency / step), stride = 4 + nwin;
    std::vector<long> first(nwin);
    auto fits = [](long row) { return row > -(1l << 30) && row < (1l << 30); };   // the plan holds rows as int
    for (int c = 0; c < chunks; ++c) {
        if (!(resolution[c] > 0.0)) {
            dz_set_error("dz_tune_plan: chunk %d has resolution %g", c, resolution[c]);
            return 2;
        }
        // the buffers a handle holds at step c: the last nwin chunks
        const int nbuf = c + 1 < nwin ? c + 1 : nwin, b0 = c - nbuf + 1;
        TailGeometry geo;
        bool ok = !tail_geometry(frames, step, latency, DZ_CROP_LOOSE, nbuf, true,
                                 [&](int b, double* start, double* res) {
                                     *start = starts[b0 + b];
                                     *res = resolution[b0 + b];
                                 },
                                 &geo, first.data()) &&
                  fits(geo.pre_first);
        int* p = plan + (size_t)c * stride;
        for (int b = 0; b < nwin; ++b) p[4 + b] = 0;
        for (int b = 0; ok && b < nbuf; ++b) {
            ok = fits(first[b]);
            p[4 + b] = (int)first[b];
        }
        if (!ok) {
            dz_set_error("dz_tune_plan: the output region of step %d does not map onto the frame grid of every buffer", c);
            return 4;
        }
        p[0] = geo.rows;
        p[1] = geo.pre;
        p[2] = (int)geo.pre_first;
        p[3] = nbuf;
        t0_out[c] = geo.out_start;
        res_out[c] = geo.out_res;
    }
    return 0;
}

extern "C" int dz_tune_replay_host(const dz_tune_desc* d, const double* hparams, int trials, double step, double latency,
                                   const double* starts, const double* resolution, signed char* assign, int* status,
                                   unsigned* bits, int use_core, int num_threads) {
    if (!d || !hparams || !assign || !status || !bits || trials < 1 || (!use_core && (!starts || !resolution))) {
        dz_set_error("dz_tune_replay_host: bad arguments");
        return 2;
    }
    if (d->K < 1 || d->K > TC_KMAX || d->G < 1 || d->G > TC_GMAX || d->N < 1 || d->F < 1 || d->D < 1 || d->nwin < 1) {
        dz_set_error("dz_tune_replay_host: %d local / %d global speakers (at most %d / %d), %d files", d->K, d->G, TC_KMAX,
                     TC_GMAX, d->N);
        return 2;
    }
    const int N = d->N, F = d->F, K = d->K, D = d->D, G = d->G;
    const int pairs = trials * N;
    const int nt = dz_host_threads(num_threads, pairs);
    std::memset(assign, 0xff, (size_t)trials * d->total_chunks * K);
    struct Scratch {
        std::vector<double> a, b;
        std::vector<int> ia;
        TcStep<CluFixed> s;
    };
    std::vector<Scratch> scratch(nt);
    auto run_handles = [&](int w, int pair) {
        const int t = pair / N, n = pair - t * N;
        const double tau = hparams[3 * t], rho = hparams[3 * t + 1], delta = hparams[3 * t + 2];
        signed char* A = assign + (size_t)t * d->total_chunks * K;
        unsigned* B = bits + (size_t)t * d->total_rows;
        Scratch& sc = scratch[w];
        sc.a.assign((size_t)F * G, 0.0);
        sc.b.resize((size_t)(F + 2) * G);
        sc.ia.resize(K);
        dz_clu* clu = nullptr;
        dz_tail* tail = nullptr;
        if (dz_clu_create(tau, rho, delta, G, &clu) ||
            dz_tail_create(F, G, step, latency, tau, DZ_AGG_HAMMING, DZ_CROP_LOOSE, d->hamming, &tail)) {
            dz_clu_destroy(clu);
            return 2;   // with the message of the create that failed
        }
        int stat = -1, failed = 0;
        for (int c = d->chunk_off[n]; c < d->chunk_off[n + 1] && !failed; ++c) {
            if (stat < 0) {
                const int rc = dz_clu_step(clu, d->seg + (size_t)c * F * K, F, K, d->emb + (size_t)c * K * D, D, sc.a.data(),
                                           sc.ia.data());
                if (rc) {   // the chain stops: its remaining chunks map nobody
                    stat = c - d->chunk_off[n];
                    std::fill(sc.a.begin(), sc.a.end(), 0.0);
                } else {
                    for (int k = 0; k < K; ++k) A[(size_t)c * K + k] = (signed char)sc.ia[k];
                }
            }
            int rows = 0;
            double t0 = 0.0, res = 0.0;
            failed = dz_tail_step(tail, sc.a.data(), starts[c], resolution[c], sc.b.data(), &rows, &t0, &res, nullptr, 0,
                                  nullptr);
            if (failed) break;
            // the plan is the same geometry (tail_core.h); what this still guards is the cache's row_off
            const int* p = d->plan + (size_t)c * (4 + d->nwin);
            if (rows != p[0] + p[1] || rows != d->row_off[c + 1] - d->row_off[c]) {
                dz_set_error("dz_tune_replay_host: dz_tail_step and the plan disagree on the rows of a step");
                failed = 4;
                break;
            }
            for (int r = 0; r < rows; ++r) {
                unsigned m = 0;
                for (int g = 0; g < G; ++g)
                    if (sc.b[(size_t)r * G + g] > tau) m |= 1u << g;
                B[d->row_off[c] + r] = m;
            }
        }
        status[pair] = stat;
        dz_clu_destroy(clu);
        dz_tail_destroy(tail);
        return failed;
    };
    auto run_core = [&](int w, int pair) {
        const int t = pair / N, n = pair - t * N;
        signed char* A = assign + (size_t)t * d->total_chunks * K;
        unsigned* B = bits + (size_t)t * d->total_rows;
        Scratch& sc = scratch[w];
        sc.a.assign((size_t)D * G, std::nan(""));   // (and its work buffer: a centroid is written before it is read)
        // the device's LDS starts with whatever was there: nothing in the step's state may be read before it is written
        std::memset(&sc.s, (pair & 1) ? 0x7f : 0xff, sizeof(sc.s));
        status[pair] = tc_chain(*d, n, hparams[3 * t], hparams[3 * t + 1], hparams[3 * t + 2], A, sc.a.data(), sc.s, 0, 1,
                                NoBarrier());
        const int c0 = d->chunk_off[n], c1 = d->chunk_off[n + 1];
        for (int p = d->row_off[c0]; p < d->row_off[c1]; ++p) B[p] = tc_row_mask(*d, p, hparams[3 * t], A);
        return 0;
    };
    const dz_host_failure f =
        dz_host_parallel_rc(pairs, nt, [&](int w, int pair) { return use_core ? run_core(w, pair) : run_handles(w, pair); });
    if (f.code) dz_set_error("dz_tune_replay_host: %s", f.message.c_str());
    return f.code;
}

extern "C" int dz_tune_score(const dz_tune_cells* cells, int trials, const unsigned* bits, double* out, int num_threads) {
    if (check_cells("dz_tune_score", cells, TC_CELLS_SEQUENTIAL, bits && out)) return 2;
    if (trials < 1 || cells->n_files < 1 || cells->max_speakers < 1 || cells->max_speakers > TC_GMAX) {
        dz_set_error("dz_tune_score: bad arguments");
        return 2;
    }
    const int N = cells->n_files, G = cells->max_speakers, pairs = trials * N;
    const int* file_cell_off = cells->file_cell_off;
    const double* cell_dur = cells->cell_dur;
    const unsigned long long* cell_ref = cells->cell_ref;
    const int nt = dz_host_threads(num_threads, pairs);
    std::vector<ScoreScratch> scratch(nt);
    std::vector<int> rcs(nt, 0);
    each_item(pairs, nt, [&](int w, int pair) {
        const int t = pair / N, n = pair - t * N;
        ScoreScratch& sc = scratch[w];
        const int cell0 = file_cell_off[n], ncell = file_cell_off[n + 1] - cell0;
        if (hyp_cells(sc, bits + (size_t)t * cells->total_rows, n, *cells, ncell)) rcs[w] = 4;
        // ---- the components over the cells
        double total = 0.0, missed = 0.0, fa = 0.0, both = 0.0;
        double cooc[TC_GMAX][64];
        unsigned hseen = 0;
        unsigned long long rseen = 0;
        for (int g = 0; g < G; ++g)
            for (int r = 0; r < 64; ++r) cooc[g][r] = 0.0;
        for (int i = 0; i < ncell; ++i) {
            const unsigned h = sc.hyp[i];
            const unsigned long long rm = cell_ref[cell0 + i];
            if (!h && !rm) continue;
            const double dur = cell_dur[cell0 + i];
            const int nref = __builtin_popcountll(rm), nhyp = __builtin_popcount(h);
            total += dur * nref;
            missed += dur * (nref > nhyp ? nref - nhyp : 0);
            fa += dur * (nhyp > nref ? nhyp - nref : 0);
            both += dur * (nref < nhyp ? nref : nhyp);
            hseen |= h;
            rseen |= rm;
            for (unsigned m = h; m; m &= m - 1) {
                const int g = __builtin_ctz(m);
                for (unsigned long long q = rm; q; q &= q - 1) cooc[g][__builtin_ctzll(q)] += dur;
            }
        }
        // ---- metrics.optimal_mapping: hypothesis labels "speaker<g>" and reference labels in str order, LSAP on -cooc
        double correct = 0.0;
        int hl[TC_GMAX], nh = 0, rl[64], nr = 0;
        for (int g = 0; g < G; ++g)
            if ((hseen >> g) & 1u) hl[nh++] = g;
        std::sort(hl, hl + nh, [](int a, int b) { return std::to_string(a) < std::to_string(b); });
        for (int r = 0; r < 64; ++r)
            if ((rseen >> r) & 1ull) rl[nr++] = r;   // the bit order IS the label order (the cache sorts them)
        if (nh > 0 && nr > 0) {
            std::vector<double> cost((size_t)nh * nr);
            std::vector<int> col(nh);
            for (int a = 0; a < nh; ++a)
                for (int b = 0; b < nr; ++b) cost[(size_t)a * nr + b] = -cooc[hl[a]][rl[b]];
            if (dz_lsap(cost.data(), nh, nr, col.data())) {
                rcs[w] = 3;
                return;
            }
            for (int a = 0; a < nh; ++a)
                if (col[a] >= 0 && cooc[hl[a]][rl[col[a]]] > 0.0) correct += cooc[hl[a]][rl[col[a]]];
        }
        double* o = out + (size_t)pair * 5;   // metrics.COMPONENTS order
        o[0] = total;
        o[1] = correct;
        o[2] = fa;
        o[3] = missed;
        o[4] = both - correct;
    });
    for (int w = 0; w < nt; ++w)
        if (rcs[w]) {
            dz_set_error(rcs[w] == 4 ? "dz_tune_score: a speech turn does not start and end on the file's scoring cells"
                                     : "dz_tune_score: the mapping's assignment problem failed");
            return rcs[w];
        }
    return 0;
}

// dz_tune_score's components from the text of tune_score_kernel (tune_core.h: tc_score_pair), on host memory
// (score_core above).
extern "C" int dz_tune_score_core(const dz_tune_cells* cells, int trials, const unsigned* bits, int lanes, int score_blocks,
                                  double* out, int num_threads) {
    if (check_cells("dz_tune_score_core", cells, TC_CELLS_KERNEL, bits && out)) return 2;
    if (trials < 1 || cells->n_files < 1 || cells->max_speakers < 1 || cells->max_speakers > TC_GMAX || cells->max_cells < 0 ||
        lanes < 1 || lanes > TC_SCORE_LANES || score_blocks < 1) {
        dz_set_error("dz_tune_score_core: bad arguments (at most %d speakers, %d lanes)", TC_GMAX, TC_SCORE_LANES);
        return 2;
    }
    const int rc = score_core<TcScoreShared>(
        tc_score_call(*cells, bits, trials), score_blocks, num_threads,
        [&](const TcScoreIn& in, TcScoreShared& sh, unsigned* slice, long long pair, int, int, int* err) {
            tc_score_pair(in, sh, slice, out + (size_t)pair * 5, err, LanesInTurn{lanes});
        });
    if (rc) {
        dz_set_error(rc == TC_SCORE_ERR_CELLS ? "dz_tune_score: a speech turn does not start and end on the file's scoring cells"
                     : rc == TC_SCORE_ERR_MAP ? "dz_tune_score: the mapping's assignment problem failed"
                                              : "dz_tune_score_core: a file has more scoring cells than a scratch slice holds");
        return rc;
    }
    return 0;
}

// The track pipelines on the host, from the text k_tune_vad.hip compiles, under the rule
// dz_tune_vad_host's `cols` selects.  agg (total_rows) once; then the pairs as tune_vad_score_kernel<Rule> runs them
// (tc_track_pair), `lanes` lanes of a workgroup played one after the other: the components where `out` is given
// (backend="core"; backend="host" scores the bits with dz_tune_score instead, the yardstick of the device scoring) and,
// under the stateful rules, the masks, which come from the lanes' state maps.  The stateless masks are agg > tau row by
// row, as on the device.
namespace {
template <typename Rule>
int track_host(const dz_tune_desc* d, const dz_tune_cells* cells, const double* taus, int trials, double* agg,
               unsigned* bits, int lanes, double* out, int num_threads) {
    const char* name = "dz_tune_vad_host";
    const bool pair_call = Rule::stateful || out;   // (whether anything goes through tc_track_pair)
    if (!d || !taus || !agg || trials < 1 || !d->seg || !d->chunk_off || !d->plan || !d->row_off || !d->row_chunk ||
        !d->hamming || d->K != 1 || d->N < 1 || d->F < 1 || d->nwin < 1 || d->total_rows < 1 || lanes > TC_TRACK_LANES ||
        (pair_call && lanes < 1)) {
        dz_set_error("%s: bad arguments (one track per chunk, 1 .. %d lanes expected)", name, TC_TRACK_LANES);
        return 2;
    }
    if (pair_call && check_cells(name, cells, TC_CELLS_TRACK_PAIR, true)) return 2;
    if constexpr (Rule::stateful) {
        const int cols = Rule::durations ? 4 : 2;
        for (int t = 0; t < trials; ++t) {
            const double* q = taus + (size_t)cols * t;
            if (!std::isfinite(q[1])) {
                dz_set_error("%s: tau_offset of trial %d is %g, not a finite number", name, t, q[1]);
                return 2;
            }
            for (int k = 2; k < cols; ++k)
                if (!(std::isfinite(q[k]) && q[k] >= 0.0)) {
                    dz_set_error("%s: %s of trial %d is %g, not a finite number >= 0", name,
                                 k == 2 ? "min_duration_on" : "min_duration_off", t, q[k]);
                    return 2;
                }
        }
    }
    const int N = d->N, rows = d->total_rows;
    const int slices = dz_host_threads(num_threads, rows);   // the rows, in slices
    each_item(slices, slices, [&](int, int s) {
        const int a = (int)((long long)rows * s / slices), b = (int)((long long)rows * (s + 1) / slices);
        for (int p = a; p < b; ++p) agg[p] = tc_vad_row(*d, p);
    });
    unsigned* pair_bits = Rule::stateful ? bits : nullptr;
    if (bits && !pair_bits)
        each_item(trials, num_threads, [&](int, int t) {
            unsigned* B = bits + (size_t)t * rows;
            const Rule rule = Rule::of(taus, t);
            for (int p = 0; p < rows; ++p) B[p] = rule(agg[p], false) ? 1u : 0u;
        });
    if (!out && !pair_bits) return 0;
    const int* file_cell_off = cells->file_cell_off;
    each_item(trials * N, num_threads, [&](int, int pair) {
        const int t = pair / N, n = pair - t * N;
        const size_t pre = (size_t)file_cell_off[n] + n;
        std::vector<TcTrackSharedOf<Rule>> sh(1);
        // LDS starts with whatever was there: nothing in it may be read before this pair has written it
        std::memset(sh.data(), (pair & 1) ? 0x7f : 0xff, sizeof(sh[0]));
        const TcTrackIn in = {agg, d->row_off, cells->mids, cells->mid_cell, cells->dur_prefix + pre, cells->ref_prefix + pre,
                              d->chunk_off[n], d->chunk_off[n + 1], file_cell_off[n + 1] - file_cell_off[n], cells->collar};
        tc_track_pair(in, Rule::of(taus, t), sh[0], out ? out + (size_t)pair * 5 : nullptr,
                      pair_bits ? pair_bits + (size_t)t * rows : nullptr, LanesInTurn{lanes});
    });
    return 0;
}
}  // namespace

extern "C" int dz_tune_vad_host(const dz_tune_desc* d, const dz_tune_cells* cells, int cols, const double* taus, int trials,
                                double* agg, unsigned* bits, int lanes, double* out, int num_threads) {
    switch (cols) {
        case 1: return track_host<TcPlainRule>(d, cells, taus, trials, agg, bits, lanes, out, num_threads);
        case 2: return track_host<TcHystRule>(d, cells, taus, trials, agg, bits, lanes, out, num_threads);
        case 4: return track_host<TcDurRule>(d, cells, taus, trials, agg, bits, lanes, out, num_threads);
    }
    dz_set_error("dz_tune_vad_host: taus of %d columns (1: tau_active; 2: and tau_offset; 4: and the two minimum durations)", cols);
    return 2;
}

// The same components from an independent sequential text, behind masks that were made elsewhere (backend="host": the
// dz_tail handles of dz_tune_vad_replay_tails).  One host thread per pair and no lanes: the turns of the file's steps
// from the masks, sorted by start; Annotation.support(max(collar, min_duration_off)); the spans shorter than
// min_duration_on dropped; the cells of the others summed one by one, from cell_dur and cell_ref and not from prefix
// sums.  bits (T, total_rows), bit 0; taus (T, 4), of which the two durations are read; out (T, N, 5).
extern "C" int dz_tune_track_score_dur(const dz_tune_cells* cells, int trials, const unsigned* bits, const double* taus,
                                       double* out, int num_threads) {
    if (check_cells("dz_tune_track_score_dur", cells, TC_CELLS_KERNEL, bits && taus && out)) return 2;
    const int n_files = cells->n_files, total_rows = cells->total_rows;
    if (trials < 1 || n_files < 1 || total_rows < 1) {
        dz_set_error("dz_tune_track_score_dur: empty shape (%d trials, %d files, %d rows)", trials, n_files, total_rows);
        return 2;
    }
    for (int t = 0; t < trials; ++t)
        for (int k = 2; k < 4; ++k) {
            const double v = taus[4 * (size_t)t + k];
            if (!(std::isfinite(v) && v >= 0.0)) {
                dz_set_error("dz_tune_track_score_dur: %s of trial %d is %g, not a finite number >= 0",
                             k == 2 ? "min_duration_on" : "min_duration_off", t, v);
                return 2;
            }
        }
    const int *file_chunk_off = cells->file_chunk_off, *row_off = cells->row_off, *mid_cell = cells->mid_cell,
              *file_cell_off = cells->file_cell_off;
    const double *mids = cells->mids, *cell_dur = cells->cell_dur, collar = cells->collar;
    const unsigned long long* cell_ref = cells->cell_ref;
    const dz_host_failure f = dz_host_parallel_rc(trials * n_files, dz_host_threads(num_threads, trials * n_files), [&](int, int pair) {
        const int t = pair / n_files, n = pair - t * n_files;
        const unsigned* B = bits + (size_t)t * total_rows;
        const double min_on = taus[4 * (size_t)t + 2], min_off = taus[4 * (size_t)t + 3];
        const double join = collar > min_off ? collar : min_off;
        const int cell0 = file_cell_off[n], ncell = file_cell_off[n + 1] - cell0;
        std::vector<Turn> turns;
        for (int c = file_chunk_off[n]; c < file_chunk_off[n + 1]; ++c) {
            const int p = row_off[c], rows = row_off[c + 1] - p;
            const double* mid = mids + (size_t)p + c;
            const int* cell = mid_cell + (size_t)p + c;
            for (int r = 0; r < rows;) {
                if (!(B[p + r] & 1u)) {
                    ++r;
                    continue;
                }
                int e = r;
                while (e < rows && (B[p + e] & 1u)) ++e;
                if (mid[e] - mid[r] > 1e-6) turns.push_back(Turn{mid[r], mid[e], cell[r], cell[e]});
                r = e;
            }
        }
        std::stable_sort(turns.begin(), turns.end(), [](const Turn& a, const Turn& b) { return a.s < b.s; });
        std::vector<Turn> spans;
        for (const Turn& u : turns) {
            if (!spans.empty()) {
                Turn& last = spans.back();
                const double gap = u.s - last.e;
                if (gap <= 1e-6 || gap < join) {
                    if (u.e > last.e) {
                        last.e = u.e;
                        last.ie = u.ie;
                    }
                    continue;
                }
            }
            spans.push_back(u);
        }
        double total = 0.0, hyp = 0.0, both = 0.0;
        for (int i = 0; i < ncell; ++i)
            if (cell_ref[cell0 + i]) total += cell_dur[cell0 + i];
        for (const Turn& u : spans) {
            if (u.e - u.s < min_on) continue;
            if (u.is < 0 || u.ie > ncell || u.is > u.ie) return 4;
            for (int i = u.is; i < u.ie; ++i) {
                hyp += cell_dur[cell0 + i];
                if (cell_ref[cell0 + i]) both += cell_dur[cell0 + i];
            }
        }
        double* o = out + (size_t)pair * 5;
        const double fa = hyp - both, missed = total - both;
        o[0] = total;
        o[1] = both;
        o[2] = fa > 0.0 ? fa : 0.0;
        o[3] = missed > 0.0 ? missed : 0.0;
        o[4] = 0.0;
        return 0;
    });
    if (f.code) dz_set_error("dz_tune_track_score_dur: a speech turn does not start and end on the file's scoring cells");
    return f.code;
}

// The same masks from an independent text: one dz_tail handle per (trial, file) with dz_tail_set_offset, the file's
// track fed step by step (what a live stream or a file batch does), pairs on host threads.  The masks are read back from
// the turns dz_tail_step returns: a turn [middle(onset), middle(r)) covers rows onset .. r - 1 of its step.  taus (T, 2);
// starts, resolution (chunks), step, latency as dz_tail_step gets them; bits (T, total_rows).  backend="host".
extern "C" int dz_tune_vad_replay_tails(const dz_tune_desc* d, const double* taus, int trials, double step, double latency,
                                        const double* starts, const double* resolution, unsigned* bits, int num_threads) {
    if (!d || !taus || !starts || !resolution || !bits || trials < 1 || !d->seg || !d->chunk_off || !d->row_off ||
        !d->hamming || d->K != 1 || d->N < 1 || d->F < 1 || d->total_rows < 1) {
        dz_set_error("dz_tune_vad_replay_tails: bad arguments (one track per chunk expected)");
        return 2;
    }
    for (int t = 0; t < trials; ++t)
        if (!std::isfinite(taus[2 * (size_t)t + 1])) {
            dz_set_error("dz_tune_vad_replay_tails: tau_offset of trial %d is %g, not a finite number", t,
                         taus[2 * (size_t)t + 1]);
            return 2;
        }
    const int N = d->N, F = d->F, pairs = trials * N;
    const int max_turns = (F + 2) / 2 + 1;
    const dz_host_failure f = dz_host_parallel_rc(pairs, dz_host_threads(num_threads, pairs), [&](int, int pair) {
        const int t = pair / N, n = pair - t * N;
        unsigned* B = bits + (size_t)t * d->total_rows;
        std::vector<double> in(F), agg((size_t)F + 2), turns((size_t)max_turns * 3);
        dz_tail* tail = nullptr;
        if (dz_tail_create(F, 1, step, latency, taus[2 * (size_t)t], DZ_AGG_HAMMING, DZ_CROP_LOOSE, d->hamming, &tail)) return 2;
        int rc = dz_tail_set_offset(tail, taus[2 * (size_t)t + 1]);
        for (int c = d->chunk_off[n]; c < d->chunk_off[n + 1] && !rc; ++c) {
            for (int i = 0; i < F; ++i) in[i] = (double)d->seg[(size_t)c * F + i];
            int rows = 0, nturns = 0;
            double t0 = 0.0, res = 0.0;
            rc = dz_tail_step(tail, in.data(), starts[c], resolution[c], agg.data(), &rows, &t0, &res, turns.data(), max_turns,
                              &nturns);
            if (rc) break;
            if (rows != d->row_off[c + 1] - d->row_off[c]) {
                dz_set_error("dz_tune_vad_replay_tails: dz_tail_step and the plan disagree on the rows of a step");
                rc = 4;
                break;
            }
            unsigned* row = B + d->row_off[c];
            for (int r = 0; r < rows; ++r) row[r] = 0u;
            for (int k = 0; k < nturns; ++k) {   // middle(i) = t0 + (i + 0.5) * res
                const long a = (long)nearbyint((turns[3 * k] - t0) / res - 0.5), b = (long)nearbyint((turns[3 * k + 1] - t0) / res - 0.5);
                // the rounding finds the rows only while t0 / res is far below 2^52 / rows; rather than trust that, the
                // rows must give back the turn's own times through dz_tail_step's expression for a frame's middle
                auto middle = [&](long i) {
                    const double s = t0 + (int)i * res;
                    return 0.5 * (s + (s + res));
                };
                if (a < 0 || b > rows || a >= b || middle(a) != turns[3 * k] || middle(b) != turns[3 * k + 1]) {
                    dz_set_error("dz_tune_vad_replay_tails: a turn of step %d does not map back onto the step's rows", c);
                    rc = 4;
                    break;
                }
                for (long r = a; r < b; ++r) row[r] = 1u;
            }
        }
        dz_tail_destroy(tail);
        return rc;
    });
    if (f.code) dz_set_error("dz_tune_vad_replay_tails: %s", f.message.c_str());
    return f.code;
}

// ---------------------------------------------------------------------------------------------------------
// Tuning delta_id
// ---------------------------------------------------------------------------------------------------------
extern "C" int dz_tune_name_host(int trials, int points, int planes, int n_files, int total_chunks, int k_local,
                                       int max_speakers, int voiceprints, const int* file_chunk_off,
                                       const signed char* assign, const int* status, const int* match_index,
                                       const float* match_distance, const signed char* vp_ref, const double* delta_id,
                                       signed char* ident, int* hold, int num_threads) {
    if (!file_chunk_off || !assign || !status || !match_index || !match_distance || !vp_ref || !delta_id || !ident) {
        dz_set_error("dz_tune_name_host: NULL argument");
        return 2;
    }
    if (trials < 1 || n_files < 1 || total_chunks < n_files || k_local < 1 || k_local > TC_KMAX || max_speakers < 1 ||
        max_speakers > TC_GMAX || voiceprints < 1) {
        dz_set_error("dz_tune_name_host: bad arguments (%d trials, %d files, %d chunks, %d local / %d global speakers (at "
                     "most %d / %d), %d voiceprints)",
                     trials, n_files, total_chunks, k_local, max_speakers, TC_KMAX, TC_GMAX, voiceprints);
        return 2;
    }
    if (points < 1 || points > TI_MAX_POINTS || planes < 1 || planes > TI_MAX_PLANES || points % planes != 0) {
        dz_set_error("dz_tune_name_host: %d points (1 .. %d) in %d planes (1 .. %d, a divisor of the points)", points,
                     TI_MAX_POINTS, planes, TI_MAX_PLANES);
        return 2;
    }
    const int N = n_files, K = k_local, G = max_speakers, V = voiceprints;
    const long long chains = (long long)trials * points * N;
    if (chains >= (1ll << 31)) {
        dz_set_error("dz_tune_name_host: %lld chains in one call; evaluate fewer trials per batch", chains);
        return 2;
    }
    each_item((int)chains, num_threads, [&](int, int chain) {
        const TiChain ch = ti_chain(chain, points, planes, N);
        const int n = ch.n;
        const int c0 = file_chunk_off[n], c1 = file_chunk_off[n + 1];
        const int st = status[(size_t)ch.t * N + n];
        const int stop = st < 0 ? c1 : std::min(c0 + st, c1);
        const size_t tj = (size_t)ch.t * points + ch.j;
        const double delta = delta_id[tj];
        const signed char* A = assign + (size_t)ch.t * total_chunks * K;
        const int* MI = match_index + (size_t)ch.plane * total_chunks * K;
        const float* MD = match_distance + (size_t)ch.plane * total_chunks * K;
        signed char* I = ident + tj * total_chunks * G;
        int* H = hold ? hold + tj * total_chunks * G : nullptr;
        float best_d[TC_GMAX];
        int best_e[TC_GMAX];
        for (int g = 0; g < G; ++g) {
            best_d[g] = INFINITY;
            best_e[g] = -1;
        }
        for (int c = c0; c < c1; ++c) {
            if (c < stop)
                for (int g = 0; g < G; ++g)
                    ti_update(best_d[g], best_e[g], g, A + (size_t)c * K, MI + (size_t)c * K, MD + (size_t)c * K, K, delta);
            for (int g = 0; g < G; ++g) {
                const int h = ti_hold(best_d[g], best_e[g], g, G, [&](int g2, float* d2, int* e2) {
                    *d2 = best_d[g2];
                    *e2 = best_e[g2];
                });
                I[(size_t)c * G + g] = ti_identity(h, vp_ref + (size_t)n * V, V);
                if (H) H[(size_t)c * G + g] = h;
            }
        }
    });
    return 0;
}

extern "C" int dz_tune_ident_score(const dz_tune_cells* cells, int trials, const unsigned* bits, const signed char* ident,
                                   double* out, int num_threads) {
    if (check_cells("dz_tune_ident_score", cells, TC_CELLS_SEQUENTIAL | TC_CELLS_CELL_STEP, bits && ident && out)) return 2;
    const int N = cells->n_files, G = cells->max_speakers, total_chunks = cells->total_chunks;
    if (trials < 1 || N < 1 || cells->total_rows < 1 || total_chunks < N || G < 1 || G > TC_GMAX) {
        dz_set_error("dz_tune_ident_score: bad arguments (%d trials, %d files, %d rows, %d chunks, %d speakers (at most %d))",
                     trials, N, cells->total_rows, total_chunks, G, TC_GMAX);
        return 2;
    }
    const int pairs = trials * N;
    const int *file_cell_off = cells->file_cell_off, *file_chunk_off = cells->file_chunk_off;
    const int nt = dz_host_threads(num_threads, pairs);
    std::vector<ScoreScratch> scratch(nt);
    std::vector<int> rcs(nt, 0);
    each_item(pairs, nt, [&](int w, int pair) {
        const int t = pair / N, n = pair - t * N;
        ScoreScratch& sc = scratch[w];
        const int cell0 = file_cell_off[n], ncell = file_cell_off[n + 1] - cell0;
        if (hyp_cells(sc, bits + (size_t)t * cells->total_rows, n, *cells, ncell)) rcs[w] = 4;
        const signed char* I = ident + (size_t)t * total_chunks * G;
        double* o = out + (size_t)pair * 5;   // metrics.COMPONENTS order
        for (int q = 0; q < 5; ++q) o[q] = 0.0;
        for (int i = 0; i < ncell; ++i) {
            const unsigned h = sc.hyp[i];
            const unsigned long long rm = cells->cell_ref[cell0 + i];
            if (!h && !rm) continue;
            const int c = cells->cell_step[cell0 + i];
            if (c < file_chunk_off[n] || c >= file_chunk_off[n + 1]) {
                rcs[w] = 4;
                continue;
            }
            int cnt[5];
            ti_cell_counts(h, rm, I + (size_t)c * G, cnt);
            for (int q = 0; q < 5; ++q) o[q] += cells->cell_dur[cell0 + i] * cnt[q];
        }
    });
    for (int w = 0; w < nt; ++w)
        if (rcs[w]) {
            dz_set_error("dz_tune_ident_score: a speech turn or a step does not lie on the file's scoring cells");
            return rcs[w];
        }
    return 0;
}

extern "C" int dz_tune_ident_score_core(const dz_tune_cells* cells, int trials, int points, const unsigned* bits,
                                        const signed char* ident, int lanes, int score_blocks, double* out,
                                        int num_threads) {
    const char* who = "dz_tune_ident_score_core";
    if (check_cells(who, cells, TC_CELLS_KERNEL | TC_CELLS_CELL_STEP, bits && ident && out)) return 2;
    const int n_files = cells->n_files, max_speakers = cells->max_speakers;
    if (trials < 1 || n_files < 1 || cells->total_rows < 1 || cells->total_chunks < n_files || max_speakers < 1 ||
        max_speakers > TC_GMAX || cells->max_cells < 0 || lanes < 1 || lanes > TC_SCORE_LANES || score_blocks < 1) {
        dz_set_error("%s: bad arguments (%d trials, at most %d speakers, %d lanes)", who, trials, TC_GMAX, TC_SCORE_LANES);
        return 2;
    }
    if (points < 1 || points > TI_MAX_POINTS) {
        dz_set_error("%s: %d points (1 .. %d)", who, points, TI_MAX_POINTS);
        return 2;
    }
    const long long plane = (long long)cells->total_chunks * max_speakers;   // one point's identities of one trial
    const int rc = score_core<TiScoreShared>(
        tc_score_call(*cells, bits, trials), score_blocks, num_threads,
        [&](const TcScoreIn& in_cells, TiScoreShared& sh, unsigned* slice, long long pair, int t, int cell0, int* err) {
            const int n = (int)(pair - (long long)t * n_files);
            const TiScoreIn in = {in_cells, ident + (size_t)t * points * plane, cells->cell_step + cell0};
            ti_score_pair(in, points, plane, (long long)n_files * 5, sh, slice, out + ((size_t)t * points * n_files + n) * 5,
                          err, LanesInTurn{lanes});
        });
    if (rc) {
        dz_set_error(rc == TC_SCORE_ERR_ARGS ? "%s: a file has more scoring cells than a scratch slice holds"
                                             : "%s: a speech turn or a step does not lie on the file's scoring cells", who);
        return rc;
    }
    return 0;
}
