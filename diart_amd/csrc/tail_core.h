// The output tail of a step, DelayedAggregation + Binarize, fp64 like the reference: the ONE text of its rules.
// dz_tail_step (tail.cpp), the tuner's plan and host scoring (tune_score.cpp) and the tuner's kernels (k_tune.hip,
// k_tune_vad.hip, k_tune_score.hip through tune_core.h) compile it, so the reference's recorded outputs and the Python
// blocks, which pin dz_tail_step (tests/test_tail.py), pin what the GPU runs, and a rounding rule cannot be mended in
// one of them and forgotten in another.  What is here:
//
//   tail_crop_range    pyannote.core's SlidingWindow.crop(focus, mode, fixed=focus.duration, return_ranges): the first
//                      frame and the frame count of a focus on a frame grid, for "strict", "loose" and "center"
//   tail_geometry      what a step does that does not depend on the scores: the output region, its cropped rows in
//                      every buffer, the first-chunk prepend, the output grid
//   tail_edge_walk     Binarize: the rising and falling edges of "row r is on"
//   tail_edge_walk_hyst  the same with an offset threshold: the on/off state is taken from and handed to the caller
//   tail_hamming_num   the Hamming-weighted sum of one output row of the tuner, one speaker at a time
//
// Arithmetic and control flow only: no allocation, nothing of the standard library; the callers own the memory.
//
// dz_tail_step does not take its Hamming sum from tail_hamming_num: it is the per-stream host hot path and keeps its
// loop nest (buffers outer, the G speakers of a row inner and contiguous, the "first buffer assigns" branch outside
// the speaker loop, where it vectorises).  Per element it is the same rule in the same order, buffers ascending, the
// first term assigned and not added to 0.0; tests/test_tune_host.py holds the two against each other bit for bit.
#pragma once
#include "../../include/diart_amd.h"
#include "clu_core.h"

#pragma clang fp contract(off)

TC_HD double tail_seg_duration(double s, double e) { return e > s ? e - s : 0.0; }

// pyannote.core SlidingWindow.samples(from_duration, mode)
TC_HD long tail_samples_for(double from_duration, double dur, double step, int mode) {
    if (mode == DZ_CROP_STRICT) return (long)floor((from_duration - dur) / step) + 1;
    if (mode == DZ_CROP_LOOSE) return (long)floor((from_duration + dur) / step);
    return (long)nearbyint(from_duration / step);  // center; np.rint = round half to even
}
TC_HD long tail_closest_frame(double t, double start, double dur, double step) {
    return (long)nearbyint((t - start - 0.5 * dur) / step);
}
// first frame index and frame count of focus [fs, fe) on the grid (start, res) for a crop with
// fixed = focus duration
TC_HD void tail_crop_range(double fs, double fe, double start, double res, int mode, long* first, long* count) {
    long i;
    if (mode == DZ_CROP_LOOSE)
        i = (long)ceil((fs - res - start) / res);
    else if (mode == DZ_CROP_STRICT)
        i = (long)ceil((fs - start) / res);
    else
        i = tail_closest_frame(fs, start, res, res);
    *first = i;
    *count = tail_samples_for(tail_seg_duration(fs, fe), res, res, mode);
}
// rows asked for outside a buffer repeat its first / last row
TC_HD int tail_clip(long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// ---------------------------------------------------------------------------------------------------------
// The geometry of one step over `nbuf` buffers of F frames, the last of which is the chunk that just arrived:
// grid(b, &start, &res) is the frame grid of buffer b.  The output region is
// [buffers[-1].extent.end - latency, ... + step) (aggregation.py:214-216); `first[b]` receives the row of buffer b at
// which it starts.  same_count: every buffer must crop to the same number of rows (np.stack raises otherwise in the
// reference; strategy "first" reads buffer 0 alone, and then first[0] alone is written).  One buffer that starts at
// 0.0 is the first chunk of a stream: the output is everything up to the end of the region (aggregation.py:188-211),
// the aggregated rows last and `pre` rows of that buffer from row `pre_first` before them.
// Returns 0, or 4: the region does not map onto the frame grid of every buffer (a count outside 1 .. F + 2 too).
// ---------------------------------------------------------------------------------------------------------
struct TailGeometry {
    int rows;         // aggregated rows
    int pre;          // rows prepended to them (first chunk of a stream), else 0
    long pre_first;   // the buffer's row the prepended rows start at
    double out_start, out_res;   // the output grid: rows + pre frames from out_start
};
template <typename Grid>
TC_HD int tail_geometry(int F, double step, double latency, int mode, int nbuf, bool same_count, Grid grid,
                        TailGeometry* out, long* first) {
    double start, res;
    grid(nbuf - 1, &start, &res);
    // extent = start + (n-1)*step + duration
    const double ext_end = start + (F - 1) * res + res;
    const double rs = ext_end - latency;
    const double re = rs + step;
    const int max_rows = F + 2;
    long count;
    grid(0, &start, &res);
    tail_crop_range(rs, re, start, res, mode, &first[0], &count);
    if (count < 1 || count > max_rows) return 4;
    for (int b = 1; same_count && b < nbuf; ++b) {
        long cnt;
        grid(b, &start, &res);
        tail_crop_range(rs, re, start, res, mode, &first[b], &cnt);
        if (cnt != count) return 4;
    }
    out->rows = (int)count;
    out->pre = 0;
    out->pre_first = 0;
    out->out_start = rs;
    out->out_res = tail_seg_duration(rs, re) / out->rows;
    grid(0, &start, &res);
    if (nbuf == 1 && start == 0.0) {
        long c1;
        tail_crop_range(0.0, re, start, res, mode, &out->pre_first, &c1);
        if (c1 < out->rows || c1 > max_rows) return 4;
        out->pre = (int)c1 - out->rows;
        out->out_start = 0.0;
        out->out_res = re / (int)c1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Binarize (utils.py:43-59) over rows 0 .. rows - 1 of one speaker: on(r) says whether row r is active; a turn runs
// from the first active row `onset` to the first inactive row r after it, and the row after the last one closes an
// open turn.  emit(onset, r) takes each turn and returns whether the walk goes on.  Returns false where emit stopped.
// ---------------------------------------------------------------------------------------------------------
template <typename On, typename Emit>
TC_HD bool tail_edge_walk(int rows, On on, Emit emit) {
    int onset = -1;
    for (int r = 0; r <= rows; ++r) {
        const bool active = r < rows && on(r);
        if (active && onset < 0) onset = r;
        if (!active && onset >= 0) {
            if (!emit(onset, r)) return false;
            onset = -1;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// Binarize with hysteresis (two thresholds, pyannote's onset / offset): a row is on when its score is > tau_active
// while the track is off and > tau_offset while it is on.  Plain compares: a NaN row is off and leaves the state off.
// tau_offset == tau_active is `y > tau`, row for row; any finite pair is defined by this line, tau_offset above
// tau_active included.
// ---------------------------------------------------------------------------------------------------------
TC_HD bool tail_hyst_on(double y, double tau_active, double tau_offset, bool active) {
    return y > (active ? tau_offset : tau_active);
}
// tail_edge_walk's stateful sibling: score(r) is the aggregated score of row r, *state the state the step before left
// (off at the start of a stream and after a reset) and, on return, the state after the last row walked.  The turns are
// formed from `on` as tail_edge_walk forms them: within the step, the row after the last closes an open turn — the
// state, not the turn, crosses into the next step.
template <typename Score, typename Emit>
TC_HD bool tail_edge_walk_hyst(int rows, Score score, double tau_active, double tau_offset, bool* state, Emit emit) {
    bool active = *state;
    const bool room = tail_edge_walk(
        rows, [&](int r) { return active = tail_hyst_on(score(r), tau_active, tau_offset, active); }, emit);
    *state = active;
    return room;
}

// ---------------------------------------------------------------------------------------------------------
// Aggregated row `ra` of a step of the tuner, one global speaker: the sum over the step's nbuf buffers, in order, of
// hamming[row] * seg[row] with row = first[b] + ra clipped into the buffer; the first term is assigned, not added to
// 0.0, as numpy's axis-0 reduction does.  Buffer b is chunk cb0 + b of seg (chunks, F, K) float32, and local(cb) is
// the local speaker of chunk cb that is mapped to this global speaker, or < 0: none.  A buffer without one adds
// h * 0.0 in dz_tail_step: leaving that addition out changes at most the sign of a zero, which no comparison sees.
// den, where given, receives the sum of the weights over ALL the buffers, formed in the same way.  (cb0 + b is formed
// as an int: counted in 64 bits, tune_mask_kernel took more vector registers.)
// ---------------------------------------------------------------------------------------------------------
template <typename Local>
TC_HD double tail_hamming_num(const float* seg, const double* hamming, int F, int K, const int* first, int cb0, int nbuf,
                              int ra, Local local, double* den) {
    double num = 0.0;
    bool none_yet = true;
    for (int b = 0; b < nbuf; ++b) {
        const long cb = cb0 + b;
        const int ks = local(cb);
        if (ks < 0 && !den) continue;
        const int row = tail_clip(first[b] + ra, F - 1);
        const double h = hamming[row];
        if (den) *den = b == 0 ? h : *den + h;
        if (ks < 0) continue;
        const double term = h * (double)seg[(cb * F + row) * K + ks];
        num = none_yet ? term : num + term;
        none_yet = false;
    }
    return num;
}
