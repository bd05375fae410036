// File-parallel evaluation (BASELINE.json configs 1 / 4): the host half of a GPU step whose rows
// are the next few CONSECUTIVE windows of several files of one rank.
//
// The reference's Benchmark feeds one file at a time, 32 consecutive windows per batch, through
// SpeakerDiarization.__call__ (/root/reference/src/diart/inference.py:392-432,
// blocks/diarization.py:193-232): segmentation / embedding are batched, then a Python loop runs
// clustering -> DelayedAggregation -> Binarize chunk by chunk.  Only that loop is sequential, and
// only WITHIN a file.  Here the rows of one GPU batch are file-major: file i contributes
// count[i] consecutive windows starting at row row0[i]; a host thread takes a whole file and walks
// its windows in order (dz_clu_step -> dz_tail_step), files run in parallel.  No barrier per window.
#include <cstddef>
#include <vector>

#include "../../include/diart_amd.h"
#include "hostpool.h"

void dz_set_error(const char* fmt, ...);

// A file stops at its first failing window.  On the pool the other files are walked to the end of their rows
// all the same; on one thread the call ends there.  The lowest failing file is reported with its own message.
static int file_fail(const char* who, int n_files, const dz_host_failure& f) {
    if (f.code) dz_set_error("%s: file %d of %d failed (code %d): %s", who, f.index, n_files, f.code, f.message.c_str());
    return f.code;
}

extern "C" int dz_file_step_batch(dz_clu** clus, dz_tail** tails, int n_files, const int* row0,
                                  const int* count, const float* seg, int frames, int k_local,
                                  const float* emb, int dim, int max_speakers, const double* chunk_start,
                                  double resolution, double* turns_out, int max_turns, int* nturns_out,
                                  int* assign_out, int num_threads) {
    if (!clus || !tails || n_files < 1 || !row0 || !count || !seg || !emb || !chunk_start || !turns_out ||
        !nturns_out) {
        dz_set_error("dz_file_step_batch: NULL argument");
        return 2;
    }
    if (frames < 1 || k_local < 1 || dim < 1 || max_speakers < 1 || max_turns < 1) {
        dz_set_error("dz_file_step_batch: empty shape");
        return 2;
    }
    for (int i = 0; i < n_files; ++i)
        if (!clus[i] || !tails[i] || count[i] < 0 || row0[i] < 0 || dz_tail_max_rows(tails[i]) != frames + 2) {
            dz_set_error("dz_file_step_batch: bad handle / row range of file %d", i);
            return 2;
        }
    const int nt = dz_host_threads(num_threads, n_files);
    const size_t F = (size_t)frames, G = (size_t)max_speakers;
    // per worker: the permuted scores of the current window and the aggregated region (discarded:
    // the RTTM needs the speech turns only)
    std::vector<std::vector<double>> scores(nt, std::vector<double>(F * G)), agg(nt, std::vector<double>((F + 2) * G));
    return file_fail("dz_file_step_batch", n_files, dz_host_parallel_rc(n_files, nt, [&](int worker, int i) {
        int rows = 0, rc = 0;
        double t0 = 0.0, res = 0.0;
        std::vector<int> assign((size_t)k_local);
        for (int t = 0; t < count[i] && !rc; ++t) {
            const size_t r = (size_t)row0[i] + t;
            rc = dz_clu_step(clus[i], seg + r * F * k_local, frames, k_local, emb + r * (size_t)k_local * dim, dim,
                             scores[worker].data(), assign_out ? assign_out + r * k_local : assign.data());
            if (!rc)
                rc = dz_tail_step(tails[i], scores[worker].data(), chunk_start[r], resolution, agg[worker].data(), &rows,
                                  &t0, &res, turns_out + r * (size_t)max_turns * 3, max_turns, nturns_out + r);
        }
        return rc;
    }));
}

// The VoiceActivityDetection sibling: no clustering, the (frames,) speech track of a window is the one "speaker" of its
// file's aggregation state (built with speakers = 1).  Same rows, same walk, same error report.
extern "C" int dz_file_vad_step_batch(dz_tail** tails, int n_files, const int* row0, const int* count,
                                      const float* track, int frames, const double* chunk_start, double resolution,
                                      double* turns_out, int max_turns, int* nturns_out, int num_threads) {
    if (!tails || n_files < 1 || !row0 || !count || !track || !chunk_start || !turns_out || !nturns_out) {
        dz_set_error("dz_file_vad_step_batch: NULL argument");
        return 2;
    }
    if (frames < 1 || max_turns < 1) {
        dz_set_error("dz_file_vad_step_batch: empty shape");
        return 2;
    }
    for (int i = 0; i < n_files; ++i)
        if (!tails[i] || count[i] < 0 || row0[i] < 0 || dz_tail_max_rows(tails[i]) != frames + 2 ||
            dz_tail_speakers(tails[i]) != 1) {
            dz_set_error("dz_file_vad_step_batch: bad handle / row range of file %d", i);
            return 2;
        }
    const int nt = dz_host_threads(num_threads, n_files);
    const size_t F = (size_t)frames;
    // per worker: the current window's track in fp64 and the aggregated region (discarded, as above)
    std::vector<std::vector<double>> scores(nt, std::vector<double>(F)), agg(nt, std::vector<double>(F + 2));
    return file_fail("dz_file_vad_step_batch", n_files, dz_host_parallel_rc(n_files, nt, [&](int worker, int i) {
        int rows = 0, rc = 0;
        double t0 = 0.0, res = 0.0;
        for (int t = 0; t < count[i] && !rc; ++t) {
            const size_t r = (size_t)row0[i] + t;
            double* s = scores[worker].data();
            for (size_t f = 0; f < F; ++f) s[f] = (double)track[r * F + f];
            rc = dz_tail_step(tails[i], s, chunk_start[r], resolution, agg[worker].data(), &rows, &t0, &res,
                              turns_out + r * (size_t)max_turns * 3, max_turns, nturns_out + r);
        }
        return rc;
    }));
}
