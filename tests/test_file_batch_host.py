"""The host side of the file batches that are not pyannote/embedding, without a GPU: ``dz_file_vad_step_batch`` (the
VoiceActivityDetection sibling of ``dz_file_step_batch``) against per-file sequences of ``dz_tail_step`` on handles of
their own, its refusals, and ``inference.file_batch_kind``, the rule that says which (pipeline, models, batch size) take
a ``FileBatch``."""
import ctypes as C

import numpy as np
import pytest

from diart_amd import _lib
from diart_amd.blocks.aggregation import BatchedOutputTail

F = 293
COUNTS = ([7, 0, 1, 12, 3], [2, 5, 0, 1, 9])      # one call, then a second one continuing the same files


def _tracks(seed=5):
    rng = np.random.default_rng(seed)
    calls = [rng.random((sum(c), F), dtype=np.float32) for c in COUNTS]
    calls[0][COUNTS[0][0] + COUNTS[0][1] + COUNTS[0][2] + 4] = np.nan      # a NaN row in the fourth file
    return calls


def _starts(counts_so_far, counts, step):
    """Window start times per row, file-major, by repeated addition as the pipelines count them."""
    out = []
    for done, c in zip(counts_so_far, counts):
        t = 0.0
        for _ in range(done):
            t += step
        for _ in range(c):
            out.append(t)
            t += step
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("step,latency", [(0.5, 0.5), (0.5, 2.0), (0.25, 1.0)])
def test_vad_file_step_equals_per_file_sequences_of_tail_steps(step, latency, threads):
    lib = _lib.load()
    n = len(COUNTS[0])
    batch = BatchedOutputTail(n, F, 1, step, latency, 0.6, num_threads=threads)
    single = BatchedOutputTail(n, F, 1, step, latency, 0.6)
    mt, res = batch.max_turns, 5.0 / F
    handles = (_lib.vp * n)(*batch._hs)
    done = [0] * n
    some_turns = False
    for track, counts in zip(_tracks(), COUNTS):
        rows = sum(counts)
        row0 = np.cumsum([0] + counts[:-1]).astype(np.int32)
        count = np.array(counts, dtype=np.int32)
        starts = _starts(done, counts, step)
        turns = np.full((rows, mt, 3), -7.0)
        nturns = np.full(rows, -7, dtype=np.int32)
        rc = lib.dz_file_vad_step_batch(handles, n, row0.ctypes.data, count.ctypes.data, track.ctypes.data, F,
                                        starts.ctypes.data, res, turns.ctypes.data, mt, nturns.ctypes.data, threads)
        assert rc == 0, lib.dz_last_error()
        # the same windows, one dz_tail_step at a time on handles of their own
        agg = np.empty((F + 2, 1))
        o_rows, o_t0, o_res = C.c_int(), C.c_double(), C.c_double()
        for i in range(n):
            for t in range(counts[i]):
                r = int(row0[i]) + t
                want = np.full((mt, 3), -7.0)
                want_n = C.c_int(-7)
                scores = track[r].astype(np.float64)
                rc = lib.dz_tail_step(single._hs[i], scores.ctypes.data, float(starts[r]), res, agg.ctypes.data,
                                      C.byref(o_rows), C.byref(o_t0), C.byref(o_res), want.ctypes.data, mt,
                                      C.byref(want_n))
                assert rc == 0, lib.dz_last_error()
                assert int(nturns[r]) == want_n.value, (i, t)
                assert np.array_equal(turns[r, :want_n.value], want[:want_n.value]), (i, t)
                some_turns |= want_n.value > 0
        done = [d + c for d, c in zip(done, counts)]
    assert some_turns, "no window of any file had a speech turn: the comparison shows nothing"


def test_vad_file_step_refuses_bad_arguments_and_touches_nothing():
    lib = _lib.load()
    tails = BatchedOutputTail(2, F, 1, 0.5, 0.5, 0.6)
    other = BatchedOutputTail(1, F + 1, 1, 0.5, 0.5, 0.6)          # built for other frames
    wide = BatchedOutputTail(1, F, 3, 0.5, 0.5, 0.6)               # built for three speakers
    mt = tails.max_turns
    track = np.random.default_rng(1).random((4, F), dtype=np.float32)
    row0, count = np.array([0, 2], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    starts = np.array([0.0, 0.5, 0.0, 0.5])
    turns = np.full((4, mt, 3), -7.0)
    nturns = np.full(4, -7, dtype=np.int32)

    def call(handles=None, n=2, row0_=row0, count_=count, track_=track.ctypes.data, frames=F, turns_=turns.ctypes.data):
        handles = (_lib.vp * 2)(*tails._hs) if handles is None else handles
        return lib.dz_file_vad_step_batch(handles, n, row0_.ctypes.data, count_.ctypes.data, track_, frames,
                                          starts.ctypes.data, 5.0 / F, turns_, mt, nturns.ctypes.data, 2)

    cases = {
        "NULL track": lambda: call(track_=None),
        "NULL turns": lambda: call(turns_=None),
        "NULL handle": lambda: call(handles=(_lib.vp * 2)(tails._hs[0], None)),
        "negative count": lambda: call(count_=np.array([2, -1], dtype=np.int32)),
        "negative row": lambda: call(row0_=np.array([-1, 2], dtype=np.int32)),
        "other frames": lambda: call(handles=(_lib.vp * 2)(tails._hs[0], other._hs[0])),
        "other speakers": lambda: call(handles=(_lib.vp * 2)(tails._hs[0], wide._hs[0])),
        "no files": lambda: call(n=0),
    }
    for name, bad in cases.items():
        assert bad() == 2, name
        assert b"dz_file_vad_step_batch" in lib.dz_last_error(), name
        assert (turns == -7.0).all() and (nturns == -7).all(), name
    # ... and the states were not stepped either: the good call now gives what fresh handles give
    assert call() == 0
    fresh = BatchedOutputTail(2, F, 1, 0.5, 0.5, 0.6)
    got_t, got_n = turns.copy(), nturns.copy()
    turns[:], nturns[:] = -7.0, -7
    assert call(handles=(_lib.vp * 2)(*fresh._hs)) == 0
    assert np.array_equal(got_n, nturns) and np.array_equal(got_t, turns)


def test_routing_rule():
    from diart_amd import models as M
    from diart_amd.blocks import SpeakerDiarization, VoiceActivityDetection
    from diart_amd.inference import file_batch_kind
    seg = M.HipSegmentation
    assert file_batch_kind(SpeakerDiarization, seg, M.HipEmbedding, 32) == "xvector"
    assert file_batch_kind(SpeakerDiarization, seg, M.HipWeSpeakerEmbedding, 32) == "wespeaker"
    assert file_batch_kind(VoiceActivityDetection, seg, None, 32) == "vad"
    groups = (M.HipEcapaEmbedding, M.HipSbXvectorEmbedding, M.HipTitaNetEmbedding, M.HipSbResNetEmbedding,
              M.HipEcapaMelEmbedding)
    for emb in groups:
        assert file_batch_kind(SpeakerDiarization, seg, emb, 1) == "groups", emb
        assert file_batch_kind(SpeakerDiarization, seg, emb, 32) is None, emb      # the batch shapes its embeddings
        assert file_batch_kind(SpeakerDiarization, seg, emb, 2) is None, emb
    for emb, bs in ((M.HipEmbedding, 32), (M.HipWeSpeakerEmbedding, 32), (M.HipEcapaEmbedding, 1)):
        assert file_batch_kind(SpeakerDiarization, seg, emb, bs, concurrent_files=0) is None
        assert file_batch_kind(SpeakerDiarization, seg, emb, bs, device_type="cpu") is None

        class Custom(SpeakerDiarization):
            pass
        assert file_batch_kind(Custom, seg, emb, bs) is None
        assert file_batch_kind(SpeakerDiarization, object, emb, bs) is None        # not a HIP segmentation
    assert file_batch_kind(VoiceActivityDetection, seg, None, 32, concurrent_files=0) is None
    assert file_batch_kind(VoiceActivityDetection, seg, None, 32, device_type="cpu") is None

    class CustomVad(VoiceActivityDetection):
        pass
    assert file_batch_kind(CustomVad, seg, None, 32) is None
    assert file_batch_kind(SpeakerDiarization, seg, None, 32) is None               # diarization needs an embedding
    assert file_batch_kind(SpeakerDiarization, seg, object, 32) is None             # not a HIP embedding


def test_benchmark_routes_without_a_device(tmp_path):
    """``Benchmark.file_batch`` asks the rule before it touches a model: a CPU config and ``concurrent_files=0`` fall
    back to the loop with nothing loaded."""
    import torch
    from diart_amd import models as M
    from diart_amd.blocks import VoiceActivityDetection, VoiceActivityDetectionConfig
    from diart_amd.inference import Benchmark

    def never():
        raise AssertionError("the model was loaded")
    cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel(never), device=torch.device("cpu"))
    assert Benchmark(tmp_path, None, tmp_path / "o").file_batch(VoiceActivityDetection, cfg) is None
    cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel(never), device=torch.device("cuda", 0))
    assert Benchmark(tmp_path, None, tmp_path / "o", concurrent_files=0).file_batch(VoiceActivityDetection, cfg) is None
