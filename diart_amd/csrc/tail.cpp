// Per-stream output tail of the diarization step, on the host in fp64:
//
//   DelayedAggregation   /root/reference/src/diart/blocks/aggregation.py:120-218
//     strategies         :73-118  (hamming :95-118, mean :73-92 ("average"), first :60-70)
//     first-chunk prepend :188-211
//   Binarize             /root/reference/src/diart/blocks/utils.py:11-59
//   the buffer handling of SpeakerDiarization.__call__
//                        /root/reference/src/diart/blocks/diarization.py:203-232
//
// The reference wraps every buffered prediction and a fresh Hamming window in
// pyannote.core.SlidingWindowFeature objects, crops each of them and walks the frames in a Python
// loop to build the Annotation: per chunk that is ~100 us of interpreter time, i.e. more than the
// GPU spends on the chunk.  Here the frame range of the output region is computed once per
// buffer from the frame grid with the same fp64 expressions pyannote.core evaluates
// (SlidingWindow.crop with return_ranges / fixed duration), rows outside a buffer repeat its
// first / last row, and the sums run in the buffer order numpy's axis-0 reduction uses, so the
// aggregated scores are bit-identical to the reference's and the speech turns come out of one
// pass over rising / falling edges of `score > threshold`.
//
// The crop rule, the geometry of a step and the edge walk are tail_core.h's, the text the tuner's
// plan and its GPU kernels compile too.  What is here is what a handle adds: the buffers of a
// stream, the strategies over them, the speech turns as (start, end, speaker), the C entry points.
#include <stddef.h>
#include <string.h>

#include <cmath>
#include <deque>
#include <new>
#include <vector>

#include "hostpool.h"
#include "tail_core.h"

void dz_set_error(const char* fmt, ...);

namespace {

struct Buffer {
    std::vector<double> data;  // [F][G]
    double start, res;         // frame grid: frame i covers [start + i*res, start + (i+1)*res)
};

}  // namespace

struct dz_tail {
    int F, G, strategy, mode, nwin;
    double step, latency, threshold;
    std::vector<double> hamming;  // [F]
    std::deque<Buffer> buffers;
    std::vector<double> num, den;  // scratch
    std::vector<long> first;       // the region's first row in every buffer
    // hysteresis (dz_tail_set_offset): off until it is called, and then today's walk runs
    bool has_offset = false;
    double offset = 0.0;
    std::vector<unsigned char> active;   // [G] the state every speaker column's last row left
};

namespace {

int tail_step(dz_tail* t, const double* scores, double chunk_start, double res, double* agg_out,
              int* rows_out, double* t0_out, double* res_out, double* turns_out, int max_turns,
              int* nturns_out) {
    const int F = t->F, G = t->G;
    if (!(res > 0.0)) return 2;
    t->buffers.emplace_back();
    Buffer& nb = t->buffers.back();
    nb.data.assign(scores, scores + (size_t)F * G);
    nb.start = chunk_start;
    nb.res = res;
    const int nbuf = (int)t->buffers.size();
    if (t->first.size() < (size_t)nbuf) t->first.resize(nbuf);  // (nwin; more only after a step that failed)
    TailGeometry geo;
    // "first" reads buffer 0 alone; for the others np.stack would raise in the reference on unequal crops
    if (tail_geometry(F, t->step, t->latency, t->mode, nbuf, t->strategy != DZ_AGG_FIRST,
                      [&](int b, double* start, double* r) {
                          *start = t->buffers[b].start;
                          *r = t->buffers[b].res;
                      },
                      &geo, t->first.data()))
        return 4;
    int rows = geo.rows;
    // ---- aggregate the region over the buffers ---------------------------------------
    if (t->strategy == DZ_AGG_FIRST) {
        const Buffer& b = t->buffers[0];
        for (int r = 0; r < rows; ++r)
            memcpy(agg_out + (size_t)r * G, b.data.data() + (size_t)tail_clip(t->first[0] + r, F - 1) * G,
                   sizeof(double) * G);
    } else {
        t->num.assign((size_t)rows * G, 0.0);
        t->den.assign(rows, 0.0);
        for (int bi = 0; bi < nbuf; ++bi) {
            const Buffer& b = t->buffers[bi];
            const long first = t->first[bi];
            for (int r = 0; r < rows; ++r) {
                const int row = tail_clip(first + r, F - 1);
                const double* src = b.data.data() + (size_t)row * G;
                double* dst = t->num.data() + (size_t)r * G;
                if (t->strategy == DZ_AGG_HAMMING) {
                    const double h = t->hamming[row];
                    if (bi == 0) {
                        for (int g = 0; g < G; ++g) dst[g] = h * src[g];
                        t->den[r] = h;
                    } else {
                        for (int g = 0; g < G; ++g) dst[g] += h * src[g];
                        t->den[r] += h;
                    }
                } else {
                    if (bi == 0)
                        for (int g = 0; g < G; ++g) dst[g] = src[g];
                    else
                        for (int g = 0; g < G; ++g) dst[g] += src[g];
                }
            }
        }
        for (int r = 0; r < rows; ++r) {
            const double d = t->strategy == DZ_AGG_HAMMING ? t->den[r] : (double)nbuf;
            for (int g = 0; g < G; ++g) agg_out[(size_t)r * G + g] = t->num[(size_t)r * G + g] / d;
        }
    }
    // ---- first buffer of a stream: everything up to the end of the region (aggregation.py:188-211)
    if (geo.pre > 0) {
        const Buffer& b = t->buffers[0];
        // the aggregated rows become the LAST `rows` rows; move them first (ranges may overlap)
        memmove(agg_out + (size_t)geo.pre * G, agg_out, sizeof(double) * (size_t)rows * G);
        for (int r = 0; r < geo.pre; ++r)
            memcpy(agg_out + (size_t)r * G, b.data.data() + (size_t)tail_clip(geo.pre_first + r, F - 1) * G,
                   sizeof(double) * G);
        rows += geo.pre;
    }
    const double out_start = geo.out_start, out_res = geo.out_res;
    *rows_out = rows;
    *t0_out = out_start;
    *res_out = out_res;
    // ---- Binarize (utils.py:43-59): strict `>`; a turn spans [middle(first active frame),
    // middle(first inactive frame after it))
    int nt = 0;
    if (turns_out) {
        auto middle = [&](int i) {
            const double s = out_start + i * out_res;
            return 0.5 * (s + (s + out_res));
        };
        bool full = false;   // hysteresis: more turns than max_turns — the walk goes on without storing, so that the
                             // state of EVERY column has seen the whole step when 5 is returned
        for (int g = 0; g < G; ++g) {
            auto emit = [&](int onset, int r) {
                if (nt >= max_turns) {
                    full = true;
                    return t->has_offset;
                }
                turns_out[3 * nt + 0] = middle(onset);
                turns_out[3 * nt + 1] = middle(r);
                turns_out[3 * nt + 2] = (double)g;
                ++nt;
                return true;
            };
            bool room;
            if (t->has_offset) {
                bool state = t->active[g] != 0;
                room = tail_edge_walk_hyst(
                    rows, [&](int r) { return agg_out[(size_t)r * G + g]; }, t->threshold, t->offset, &state, emit);
                t->active[g] = state;
            } else {
                room = tail_edge_walk(rows, [&](int r) { return agg_out[(size_t)r * G + g] > t->threshold; }, emit);
            }
            if (!room) return 5;
        }
        if (full) return 5;
    } else if (t->has_offset) {   // no turns asked for: the states still follow the rows
        for (int g = 0; g < G; ++g) {
            bool state = t->active[g] != 0;
            tail_edge_walk_hyst(
                rows, [&](int r) { return agg_out[(size_t)r * G + g]; }, t->threshold, t->offset, &state,
                [](int, int) { return true; });
            t->active[g] = state;
        }
    }
    if (nturns_out) *nturns_out = nt;
    // diarization.py:228-232
    if ((int)t->buffers.size() == t->nwin) t->buffers.pop_front();
    return 0;
}

}  // namespace

extern "C" int dz_tail_create(int frames, int speakers, double step, double latency,
                              double threshold, int strategy, int cropping_mode,
                              const double* hamming, dz_tail** out) {
    if (!out || frames < 1 || speakers < 1 || !(step > 0.0) || !(latency >= step) ||
        strategy < DZ_AGG_HAMMING || strategy > DZ_AGG_FIRST || cropping_mode < DZ_CROP_STRICT ||
        cropping_mode > DZ_CROP_CENTER || (strategy == DZ_AGG_HAMMING && !hamming)) {
        dz_set_error("dz_tail_create: bad arguments (latency must be >= step)");
        return 2;
    }
    dz_tail* t = new (std::nothrow) dz_tail;
    if (!t) {
        dz_set_error("dz_tail_create: out of memory");
        return 1;
    }
    t->F = frames; t->G = speakers; t->strategy = strategy; t->mode = cropping_mode;
    t->step = step; t->latency = latency; t->threshold = threshold;
    t->nwin = (int)nearbyint(latency / step);  // int(round(latency / step)), aggregation.py:157
    if (hamming) t->hamming.assign(hamming, hamming + frames);
    *out = t;
    return 0;
}
extern "C" int dz_tail_reset(dz_tail* t) {
    if (!t) return 2;
    t->buffers.clear();
    t->active.assign(t->active.size(), 0);   // the states; the offset stays
    return 0;
}
extern "C" int dz_tail_set_offset(dz_tail* t, double offset) {
    if (!t) {
        dz_set_error("dz_tail_set_offset: NULL handle");
        return 2;
    }
    if (!std::isfinite(offset)) {
        dz_set_error("dz_tail_set_offset: the offset threshold must be finite, got %g", offset);
        return 2;
    }
    if (!t->has_offset) t->active.assign(t->G, 0);
    t->has_offset = true;
    t->offset = offset;
    return 0;
}
extern "C" int dz_tail_destroy(dz_tail* t) {
    delete t;
    return 0;
}
extern "C" int dz_tail_max_rows(const dz_tail* t) { return t ? t->F + 2 : 0; }
extern "C" int dz_tail_speakers(const dz_tail* t) { return t ? t->G : 0; }

static int tail_fail(const char* who, int rc) {
    if (rc == 4)
        dz_set_error("%s: the output region does not map onto the frame grid of every buffer", who);
    else if (rc == 5)
        dz_set_error("%s: more speech turns than max_turns", who);
    else if (rc)
        dz_set_error("%s: bad arguments", who);
    return rc;
}

extern "C" int dz_tail_step(dz_tail* t, const double* scores, double chunk_start, double resolution,
                            double* agg_out, int* rows_out, double* t0_out, double* res_out,
                            double* turns_out, int max_turns, int* nturns_out) {
    if (!t || !scores || !agg_out || !rows_out || !t0_out || !res_out) {
        dz_set_error("dz_tail_step: NULL argument");
        return 2;
    }
    return tail_fail("dz_tail_step", tail_step(t, scores, chunk_start, resolution, agg_out, rows_out,
                                               t0_out, res_out, turns_out, max_turns, nturns_out));
}

extern "C" int dz_tail_step_batch(dz_tail** tails, int n, const double* scores,
                                  const double* chunk_start, const double* resolution,
                                  double* agg_out, int* rows_out, double* t0_out, double* res_out,
                                  double* turns_out, int max_turns, int* nturns_out,
                                  int num_threads) {
    if (!tails || n < 1 || !scores || !chunk_start || !resolution || !agg_out || !rows_out ||
        !t0_out || !res_out) {
        dz_set_error("dz_tail_step_batch: NULL argument");
        return 2;
    }
    const int F = tails[0]->F, G = tails[0]->G;
    for (int i = 0; i < n; ++i)
        if (!tails[i] || tails[i]->F != F || tails[i]->G != G) {
            dz_set_error("dz_tail_step_batch: handles must share frames / speakers");
            return 2;
        }
    const size_t mr = (size_t)F + 2;
    return tail_fail("dz_tail_step_batch", dz_host_parallel_rc(n, num_threads, [&](int, int i) {
        return tail_step(tails[i], scores + (size_t)i * F * G, chunk_start[i], resolution[i],
                         agg_out + (size_t)i * mr * G, rows_out + i, t0_out + i, res_out + i,
                         turns_out ? turns_out + (size_t)i * max_turns * 3 : nullptr, max_turns,
                         nturns_out ? nturns_out + i : nullptr);
    }).code);
}
