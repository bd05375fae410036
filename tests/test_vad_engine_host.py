"""VoiceActivityDetection on the N-stream engine, the parts that need no GPU: the C entry point of the fused speech
track refuses bad arguments, ``StreamServer`` refuses pipelines it does not serve, and the engine's host half — the C++
output tail fed the (F, 1) speech track, turns labelled ``"speech"`` — gives the turns of the blocks pipeline's own
host half (``VoiceActivityDetection.finalise``: ``DelayedAggregation`` + ``Binarize``, reference vad.py:146-191)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diart_amd import _lib
from diart_amd import models as M
from diart_amd.blocks import VoiceActivityDetection, VoiceActivityDetectionConfig
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.features import SlidingWindow, SlidingWindowFeature

SR, DURATION, FRAMES = 16000, 5.0, 293


def test_forward_vad_symbol_is_exported_with_a_prototype():
    lib = C.CDLL(str(_lib.lib_path()))
    assert hasattr(lib, "dz_seg_forward_vad")
    res, args = _lib.SIGNATURES["dz_seg_forward_vad"]
    assert res is C.c_int and len(args) == 7 and args[2] is C.c_longlong and args[3] is C.c_int
    header = (_lib.lib_path().parent.parent / "include" / "diart_amd.h").read_text()
    assert "int dz_seg_forward_vad(dz_seg* seg, const float* d_wave, long long wave_stride, int batch," in header


@pytest.mark.parametrize("handle, stride, batch, out, vad, what", [
    (None, 80000, 1, 16, 16, "NULL handle"),
    (None, 80000, 1, 16, None, "NULL output"),
    (None, 80000, 1, None, 16, "NULL output"),
    (None, 80000, 0, 16, 16, "batch 0"),
    (None, 80000, -3, 16, 16, "batch -3"),
    (None, -4, 1, 16, 16, "negative stride"),
])
def test_forward_vad_refuses_bad_arguments_without_touching_the_gpu(handle, stride, batch, out, vad, what):
    lib = _lib.load()
    rc = lib.dz_seg_forward_vad(handle, 16, stride, batch, out, vad, None)
    assert rc != 0
    msg = lib.dz_last_error().decode()
    assert "dz_seg_forward_vad" in msg and what in msg, msg


def test_stream_server_refuses_unknown_pipelines_and_an_embedding_for_vad():
    from diart_amd.serve import StreamServer
    with pytest.raises(ValueError, match="bogus"):
        StreamServer(None, None, max_streams=2, pipeline="bogus")
    with pytest.raises(ValueError, match="embedding"):
        StreamServer(None, object(), max_streams=2, pipeline="vad")


def test_labelled_annotation_keeps_the_default_speaker_labels():
    turns = np.array([[0.5, 1.25, 0.0], [2.0, 3.0, 0.0]])
    default = BatchedOutputTail.annotation(turns, 2)
    assert [lab for _, _, lab in default.itertracks(yield_label=True)] == ["speaker0", "speaker0"]
    speech = BatchedOutputTail.annotation(turns, 2, uri="s", label="speech")
    assert [(s.start, s.end, lab) for s, _, lab in speech.itertracks(yield_label=True)] == \
        [(0.5, 1.25, "speech"), (2.0, 3.0, "speech")]
    assert speech.to_rttm().splitlines()[0].split()[7] == "speech"


def _blocks_vad(step, latency):
    """The blocks pipeline on the host: finalise() is its host half for given segmentation scores."""
    cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel(lambda: torch.nn.Identity()), step=step,
                                       latency=latency, tau_active=0.6, device=torch.device("cpu"))
    return VoiceActivityDetection(cfg)


def _tracks(ann):
    return sorted((round(s.start, 9), round(s.end, 9), str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


@pytest.mark.parametrize("step", [0.25, 0.5])
@pytest.mark.parametrize("latency", ["step", "duration"])
def test_output_tail_on_the_speech_track_equals_the_blocks_pipeline(step, latency):
    """Random speech tracks, with runs above and below tau and a few values right at it, through the engine's host
    half (BatchedOutputTail with one speaker, fed the f64 track, turns labelled "speech") and through
    VoiceActivityDetection.finalise (segmentation scores whose max over 3 speakers is that track): the same turns at
    every step, for several streams at once."""
    lat = step if latency == "step" else DURATION
    n, steps = 3, int(round(DURATION / step)) + 6
    rng = np.random.default_rng(int(step * 100) + (latency == "step"))
    tail = BatchedOutputTail(n, FRAMES, 1, step, lat, 0.6, strategy="hamming", cropping_mode="loose", num_threads=2)
    pipes = [_blocks_vad(step, lat) for _ in range(n)]
    for t in range(steps):
        # piecewise-constant runs so that binarisation yields turns; some frames exactly at the threshold (not in
        # a stream's first window: there the blocks pipeline binarises its float32 buffer, and numpy compares a
        # float32 array with tau in float32, so float32(0.6) is not above it; the tail compares in float64)
        track = np.repeat(rng.uniform(0.0, 1.0, (n, FRAMES // 8 + 1)), 8, axis=1)[:, :FRAMES].astype(np.float32)
        if t > 0:
            track[:, rng.integers(0, FRAMES, 5)] = np.float32(0.6)
        scores = rng.uniform(0.0, 1.0, (n, FRAMES, 3)).astype(np.float32) * track[:, :, None]
        scores[np.arange(n), :, rng.integers(0, 3, n)] = track          # max over speakers = the track
        assert np.array_equal(scores.max(axis=-1), track)
        _, _, _, _, turns, nturns = tail(track[:, :, None].astype(np.float64), t * step, DURATION / FRAMES)
        for i in range(n):
            got = BatchedOutputTail.annotation(turns[i], int(nturns[i]), label="speech")
            wav = SlidingWindowFeature(np.zeros((int(DURATION * SR), 1), dtype=np.float32),
                                       SlidingWindow(start=t * step, duration=1 / SR, step=1 / SR))
            (want, _), = pipes[i].finalise([wav], torch.from_numpy(scores[i:i + 1]))
            assert _tracks(got) == _tracks(want), (step, latency, t, i)
            assert all(lab == "speech" for lab in got.labels())
