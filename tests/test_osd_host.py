"""OverlappedSpeechDetection, the parts that need no GPU: the C entry points of the overlap track exist and refuse bad
arguments by name, ``functional.overlap_track`` on the host is the defining torch statement, the pipeline's host half
gives the turns of the C++ output tail fed the float64 overlap track (labelled ``"overlap"``), the overlap reference and
its error rate count what a hand can count, and the routing rules know the new pipeline without moving the old
answers."""
import ctypes as C

import numpy as np
import pytest
import torch

from diart_amd import _lib
from diart_amd import models as M
from diart_amd.blocks import (OverlappedSpeechDetection, OverlappedSpeechDetectionConfig, SpeakerDiarization,
                              VoiceActivityDetection)
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.features import Annotation, Segment, SlidingWindow, SlidingWindowFeature
from diart_amd.functional import overlap_track

SR, DURATION, FRAMES = 16000, 5.0, 293
TAU = 0.5
nan, inf = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_the_two_entry_points_are_exported_with_prototypes():
    lib = C.CDLL(str(_lib.lib_path()))
    assert hasattr(lib, "dz_seg_forward_track") and hasattr(lib, "dz_overlap_track")
    res, args = _lib.SIGNATURES["dz_seg_forward_track"]
    assert res is C.c_int and len(args) == 8 and args[2] is C.c_longlong and args[3] is C.c_int and args[6] is C.c_int
    res, args = _lib.SIGNATURES["dz_overlap_track"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_longlong and args[2] is C.c_longlong \
        and args[3] is C.c_int
    header = (_lib.lib_path().parent.parent / "include" / "diart_amd.h").read_text()
    assert "int dz_seg_forward_track(dz_seg* seg, const float* d_wave, long long wave_stride, int batch," in header
    assert "float* d_out, float* d_track, int track, void* stream);" in header
    assert "int dz_overlap_track(const float* d_scores, long long row_stride, long long rows, int K, float* d_out, " \
           "void* stream);" in header
    assert "enum { DZ_TRACK_SPEECH = 0, DZ_TRACK_OVERLAP = 1 };" in header
    assert (_lib.TRACK_SPEECH, _lib.TRACK_OVERLAP) == (0, 1)
    # the function the speech track came from keeps its prototype
    assert "int dz_seg_forward_vad(dz_seg* seg, const float* d_wave, long long wave_stride, int batch,\n" \
           "                       float* d_out, float* d_vad, void* stream);" in header
    assert len(_lib.SIGNATURES["dz_seg_forward_vad"][1]) == 7


@pytest.mark.parametrize("track", [0, 1])
@pytest.mark.parametrize("handle, stride, batch, out, trk, what", [
    (None, 80000, 1, 16, 16, "NULL handle"),
    (None, 80000, 1, 16, None, "NULL output"),
    (None, 80000, 1, None, 16, "NULL output"),
    (None, 80000, 0, 16, 16, "batch 0"),
    (None, 80000, -3, 16, 16, "batch -3"),
    (None, -4, 1, 16, 16, "negative stride"),
])
def test_forward_track_refuses_bad_arguments_without_touching_the_gpu(handle, stride, batch, out, trk, what, track):
    lib = _lib.load()
    rc = lib.dz_seg_forward_track(handle, 16, stride, batch, out, trk, track, None)
    assert rc != 0
    msg = lib.dz_last_error().decode()
    assert "dz_seg_forward_track" in msg and what in msg, msg


@pytest.mark.parametrize("track", [-1, 2, 7])
def test_forward_track_refuses_an_unknown_track(track):
    lib = _lib.load()
    assert lib.dz_seg_forward_track(None, 16, 80000, 1, 16, 16, track, None) != 0
    msg = lib.dz_last_error().decode()
    assert "dz_seg_forward_track" in msg and f"unknown track {track}" in msg, msg


@pytest.mark.parametrize("scores, stride, rows, K, out, what", [
    (None, 3, 10, 3, 16, "NULL"),
    (16, 3, 10, 3, None, "NULL"),
    (16, 3, 10, 1, 16, "got 1"),          # one speaker has no overlap: refused, not answered with zeros
    (16, 3, 10, 0, 16, "got 0"),
    (16, 9, 10, 9, 16, "got 9"),
    (16, -3, 10, 3, 16, "negative stride"),
    (16, 2, 10, 3, 16, "hold no 3 scores"),
    (16, 3, 0, 3, 16, "rows 0"),
])
def test_overlap_track_refuses_bad_arguments_without_touching_the_gpu(scores, stride, rows, K, out, what):
    lib = _lib.load()
    rc = lib.dz_overlap_track(scores, stride, rows, K, out, None)
    assert rc != 0
    msg = lib.dz_last_error().decode()
    assert "dz_overlap_track" in msg and what in msg, msg


@pytest.mark.parametrize("handle, stride, batch, out, vad, what", [
    (None, 80000, 1, 16, 16, "dz_seg_forward_vad: NULL handle"),
    (None, 80000, 1, 16, None, "dz_seg_forward_vad: NULL output"),
    (None, 80000, 0, 16, 16, "dz_seg_forward_vad: batch 0 < 1"),
    (None, -4, 1, 16, 16, "dz_seg_forward_vad: negative stride -4"),
])
def test_forward_vad_refusals_are_worded_as_before(handle, stride, batch, out, vad, what):
    lib = _lib.load()
    assert lib.dz_seg_forward_vad(handle, 16, stride, batch, out, vad, None) != 0
    assert lib.dz_last_error().decode() == what


# ---------------------------------------------------------------------------------------------------- the definition
TABLE = [([1, 1, 0], 1.0), ([.3, .3, .3], .3), ([.2, nan, .7], .7), ([nan, nan, .1], nan), ([inf, -inf, 0], 0.0)]


@pytest.mark.parametrize("row, want", TABLE)
def test_overlap_track_on_the_host_is_the_second_largest_with_multiplicity(row, want):
    got = overlap_track(torch.tensor([row], dtype=torch.float32))
    assert got.shape == (1, 1)
    want = torch.tensor([[want]], dtype=torch.float32)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    if not torch.isnan(want).any():
        assert torch.equal(got, want)


def test_overlap_track_keeps_the_leading_shape_and_takes_arrays():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 7, 4, generator=g)
    got = overlap_track(x)
    assert got.shape == (2, 7, 1)
    assert torch.equal(got, torch.sort(x, dim=-1, descending=True).values[..., 1:2])
    arr = overlap_track(x.numpy())
    assert isinstance(arr, np.ndarray) and arr.shape == (2, 7, 1) and np.array_equal(arr, got.numpy())
    with pytest.raises(ValueError, match="overlap_track"):
        overlap_track(torch.rand(5, 1))


# ---------------------------------------------------------------------------------------------------- the host half
def _blocks_osd(step, latency):
    """The blocks pipeline on the host: finalise() is its host half for given segmentation scores."""
    cfg = OverlappedSpeechDetectionConfig(segmentation=M.SegmentationModel(lambda: torch.nn.Identity()), step=step,
                                          latency=latency, tau_active=TAU, device=torch.device("cpu"))
    return OverlappedSpeechDetection(cfg)


def _tracks(ann):
    return sorted((round(s.start, 9), round(s.end, 9), str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


def test_the_pipeline_is_a_sibling_with_its_own_defaults():
    assert not issubclass(OverlappedSpeechDetection, VoiceActivityDetection)
    pipe = _blocks_osd(0.5, 0.5)
    assert OverlappedSpeechDetection.get_config_class() is OverlappedSpeechDetectionConfig
    assert OverlappedSpeechDetectionConfig(segmentation=M.SegmentationModel(lambda: torch.nn.Identity()),
                                           device=torch.device("cpu")).tau_active == 0.5
    from diart_amd.blocks import base
    assert list(OverlappedSpeechDetection.hyper_parameters()) == [base.TauActive]
    from diart_amd.metrics import DetectionErrorRate, OverlapDetectionErrorRate
    metric = OverlappedSpeechDetection.suggest_metric()
    assert isinstance(metric, OverlapDetectionErrorRate) and isinstance(metric, DetectionErrorRate)
    wav = SlidingWindowFeature(np.zeros((int(DURATION * SR), 1), dtype=np.float32),
                               SlidingWindow(start=0.0, duration=1 / SR, step=1 / SR))
    with pytest.raises(ValueError, match="OverlappedSpeechDetection"):
        pipe.finalise([wav], torch.rand(1, FRAMES, 1))          # one speaker: no overlap, refused by name


@pytest.mark.parametrize("step", [0.25, 0.5])
@pytest.mark.parametrize("latency", ["step", "duration"])
def test_output_tail_on_the_overlap_track_equals_the_blocks_pipeline(step, latency):
    """Random piecewise-constant scores for 3 speakers, a few of their overlap-track values right at tau, through
    OverlappedSpeechDetection.finalise and through the engine's host half (BatchedOutputTail with one speaker, fed the
    float64 overlap track, turns labelled "overlap"): the same turns at every step, for several streams at once."""
    lat = step if latency == "step" else DURATION
    n, steps = 3, int(round(DURATION / step)) + 6
    rng = np.random.default_rng(40 + int(step * 100) + (latency == "step"))
    tail = BatchedOutputTail(n, FRAMES, 1, step, lat, TAU, strategy="hamming", cropping_mode="loose", num_threads=2)
    pipes = [_blocks_osd(step, lat) for _ in range(n)]
    some, none = 0, 0
    for t in range(steps):
        # runs of 32 frames per speaker (longer than a step, so that steps without a turn exist), offset against each
        # other, so that the second largest changes speaker
        scores = np.stack([np.repeat(rng.uniform(0.0, 1.0, (n, FRAMES // 32 + 2)), 32, axis=1)[:, k * 3:k * 3 + FRAMES]
                           for k in range(3)], axis=-1).astype(np.float32)
        if t > 0:
            # values exactly at the threshold (not in a stream's first window: there the blocks pipeline binarises its
            # float32 buffer, and numpy compares a float32 array with tau in float32; the tail compares in float64):
            # two speakers at tau and one below, so the track is tau itself
            f = rng.integers(0, FRAMES, 5)
            scores[:, f, :] = np.float32(TAU)
            scores[:, f, rng.integers(0, 3)] = np.float32(0.1)
        track = np.sort(scores.astype(np.float64), axis=-1)[..., 1:2]       # second largest of 3 = the middle one
        assert np.array_equal(track.astype(np.float32),
                              torch.sort(torch.from_numpy(scores), dim=-1, descending=True).values[..., 1:2].numpy())
        _, _, _, _, turns, nturns = tail(track, t * step, DURATION / FRAMES)
        for i in range(n):
            got = BatchedOutputTail.annotation(turns[i], int(nturns[i]), label="overlap")
            wav = SlidingWindowFeature(np.zeros((int(DURATION * SR), 1), dtype=np.float32),
                                       SlidingWindow(start=t * step, duration=1 / SR, step=1 / SR))
            (want, _), = pipes[i].finalise([wav], torch.from_numpy(scores[i:i + 1]))
            assert _tracks(got) == _tracks(want), (step, latency, t, i)
            assert all(lab == "overlap" for lab in want.labels()) and all(lab == "overlap" for lab in got.labels())
            some += len(_tracks(want)) > 0
            none += len(_tracks(want)) == 0
    print(f"steps with an overlap turn: {some}, without: {none}")
    assert some > 0, "no overlap turn anywhere: the comparison shows nothing"
    assert none > 0, "every step of every stream has an overlap turn: a track stuck high would pass"


# ---------------------------------------------------------------------------------------------------- the metric
def _annotation(turns, uri="x"):
    ann = Annotation(uri=uri)
    for i, (s, e, lab) in enumerate(turns):
        ann[Segment(s, e), i] = lab
    return ann


def _segments(ann):
    return [(s.start, s.end, lab) for s, _, lab in ann.itertracks(yield_label=True)]


def test_overlap_reference_on_a_hand_written_annotation():
    from diart_amd.metrics import overlap_reference
    ref = _annotation([
        (0.0, 10.0, "A"),
        (2.0, 4.0, "B"),            # nested in A                      -> [2, 4]
        (4.0, 5.0, "C"),            # touches B's end, nested in A     -> merged: [2, 5]
        (6.0, 8.0, "A"),            # the same label over itself: one speaker, no overlap
        (10.0, 11.0, "B"),          # touches A's end: nothing in common
        (12.0, 14.0, "B"), (13.0, 15.0, "C"), (13.5, 16.0, "A"),     # three at once: ONE region [13, 15]
        (20.0, 21.0, "A"), (22.0, 23.0, "B"),                        # disjoint
    ], uri="meeting")
    got = overlap_reference(ref)
    assert got.uri == "meeting"
    assert _segments(got) == [(2.0, 5.0, "overlap"), (13.0, 15.0, "overlap")]
    assert _segments(overlap_reference(_annotation([(0.0, 1.0, "A"), (0.5, 2.0, "A")]))) == []
    assert _segments(overlap_reference(Annotation(uri="empty"))) == []


def test_overlap_detection_error_rate_counts_by_hand():
    from diart_amd.metrics import OverlapDetectionErrorRate
    ref = _annotation([(0.0, 10.0, "A"), (2.0, 5.0, "B"), (13.0, 15.0, "B"), (12.0, 16.0, "C")])
    # overlap regions of the reference: [2, 5] and [13, 15], 5 s in all
    hyp = _annotation([(1.0, 4.0, "overlap"),          # 1 s false alarm, 2 s correct, [4, 5] missed
                       (14.0, 17.0, "overlap")])       # [13, 14] missed, 1 s correct, 2 s false alarm
    metric = OverlapDetectionErrorRate(collar=0, skip_overlap=False)
    d = metric(ref, hyp, detailed=True)
    assert d["total"] == pytest.approx(5.0) and d["correct"] == pytest.approx(3.0)
    assert d["missed detection"] == pytest.approx(2.0) and d["false alarm"] == pytest.approx(3.0)
    assert d["confusion"] == 0.0
    assert d["overlap detection error rate"] == pytest.approx(1.0) and abs(metric) == pytest.approx(1.0)
    perfect = OverlapDetectionErrorRate()
    assert perfect(ref, _annotation([(2.0, 5.0, "overlap"), (13.0, 15.0, "overlap")])) == 0.0
    with pytest.raises(NotImplementedError):
        OverlapDetectionErrorRate(collar=0.25)


# ---------------------------------------------------------------------------------------------------- the routing
def test_file_batch_kind_knows_the_pipeline_and_keeps_its_other_answers():
    from diart_amd.inference import FILE_BATCH_BY_DEFAULT, file_batch_kind
    from diart_amd.pipeline import FileBatch
    seg = M.HipSegmentation
    assert file_batch_kind(OverlappedSpeechDetection, seg, None, 32) == "osd"
    assert file_batch_kind(OverlappedSpeechDetection, seg, None, 1) == "osd"
    assert file_batch_kind(OverlappedSpeechDetection, seg, None, 32, explicit=False) == "osd"
    assert file_batch_kind(OverlappedSpeechDetection, seg, None, 32, concurrent_files=0) is None
    assert file_batch_kind(OverlappedSpeechDetection, seg, None, 32, device_type="cpu") is None
    assert file_batch_kind(OverlappedSpeechDetection, object, None, 32) is None

    class CustomOsd(OverlappedSpeechDetection):
        pass
    assert file_batch_kind(CustomOsd, seg, None, 32) is None
    assert FILE_BATCH_BY_DEFAULT["osd"] == FILE_BATCH_BY_DEFAULT["vad"]
    assert FileBatch.GATHER_DEFAULT["osd"] == FileBatch.GATHER_DEFAULT["vad"]
    # the answers that existed did not move
    assert file_batch_kind(SpeakerDiarization, seg, M.HipEmbedding, 32) == "xvector"
    assert file_batch_kind(SpeakerDiarization, seg, M.HipWeSpeakerEmbedding, 32) == "wespeaker"
    assert file_batch_kind(SpeakerDiarization, seg, M.HipEcapaEmbedding, 1) == "groups"
    assert file_batch_kind(SpeakerDiarization, seg, M.HipEcapaEmbedding, 32) is None
    assert file_batch_kind(VoiceActivityDetection, seg, None, 32) == "vad"
    assert file_batch_kind(VoiceActivityDetection, seg, None, 32, concurrent_files=0) is None

    class CustomVad(VoiceActivityDetection):
        pass
    assert file_batch_kind(CustomVad, seg, None, 32) is None
    assert file_batch_kind(SpeakerDiarization, seg, None, 32) is None


def test_stream_server_and_file_batch_refusals_that_need_no_device():
    from diart_amd.pipeline import FileBatch
    from diart_amd.serve import PIPELINES, StreamServer
    assert PIPELINES == ("diarization", "vad", "osd")
    with pytest.raises(ValueError, match="embedding"):
        StreamServer(None, object(), max_streams=2, pipeline="osd")
    with pytest.raises(ValueError, match="OverlappedSpeechDetection"):
        StreamServer(None, object(), max_streams=2, pipeline="osd")
    with pytest.raises(ValueError, match="embedding"):
        StreamServer(None, object(), max_streams=2, pipeline="vad")
    with pytest.raises(ValueError, match="bogus"):
        StreamServer(None, None, max_streams=2, pipeline="bogus")
    with pytest.raises(ValueError, match="embedding"):
        FileBatch(None, object(), pipeline="osd")
    with pytest.raises(ValueError, match="bogus"):
        FileBatch(None, None, pipeline="bogus")


def test_the_tuner_still_refuses_the_pipeline():
    """Tuning by replay is a follow-up: any class but the two existing pipelines stays a ValueError."""
    from diart_amd.optim import _pipeline_kind
    with pytest.raises(ValueError):
        _pipeline_kind(OverlappedSpeechDetection)
