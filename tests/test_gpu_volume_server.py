"""``StreamServer(volume_in_db=...)``: every window of every stream is brought to the target volume on its own before
the models see it (DESIGN.md "Volume adjustment").  Three streams carry ONE signal at 0.01, 0.3 and 2.0 times its level,
a few steps past the first full window."""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.blocks import (AdjustVolume, SpeakerDiarization, SpeakerDiarizationConfig, VoiceActivityDetection,
                              VoiceActivityDetectionConfig)
from diart_amd.functional import adjust_volume
from diart_amd.inference import PredictionAccumulator, rolling_windows
from diart_amd.pipeline import StreamBatch, VadBatch
from diart_amd.serve import StreamServer
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_streams

pytestmark = pytest.mark.gpu

SR, HOP, TARGET = 16000, 8000, -20.0
SCALES = {"quiet": 0.01, "plain": 0.3, "loud": 2.0}
SECONDS = 6.5                      # the first full window and three more steps: 4 windows per stream


@pytest.fixture(scope="module")
def audio():
    x = synth_streams(1, SECONDS, seed0=640)[0]
    return {k: (x * np.float32(s)).astype(np.float32) for k, s in SCALES.items()}


def windows_of(x):
    blocks = (x[None, i:i + HOP] for i in range(0, len(x) // HOP * HOP, HOP))
    return list(rolling_windows(blocks, 5.0, 0.5, SR))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def feed(srv, audio):
    for k, x in audio.items():
        srv.open(k)
        srv.push(k, x)
    srv.drain()


def captured_windows(audio, gpu, volume_in_db):
    """The windows a custom engine is handed, keyed (stream, window start)."""
    seen = {}
    slot_of = {}

    def engine(windows, starts, slots):
        assert isinstance(windows, np.ndarray) and windows.dtype == np.float32 and windows.shape[1] == 5 * SR
        for w, t, s in zip(windows, starts, slots):
            seen[(s, round(float(t), 6))] = w.copy()
        return [np.zeros((0, 3)) for _ in slots]

    srv = StreamServer(None, None, max_streams=3, device=gpu, engine=engine, volume_in_db=volume_in_db)
    assert srv.volume_in_db == volume_in_db
    for k, x in audio.items():
        srv.open(k)
        slot_of[k] = srv._streams[k].slot
        srv.push(k, x)
    srv.drain()
    return {(k, t): w for k in audio for (s, t), w in seen.items() if s == slot_of[k]}


def test_custom_engine_windows(gpu, audio):
    """Under ``None`` the windows are the raw rolling windows; under -20 dB they are ``adjust_volume`` of those, bit for
    bit."""
    raw = captured_windows(audio, gpu, None)
    adj = captured_windows(audio, gpu, TARGET)
    assert sorted(raw) == sorted(adj) and len(raw) == 3 * 4
    for k, x in audio.items():
        for w in windows_of(x):
            key = (k, round(float(w.sliding_window.start), 6))
            assert np.array_equal(bits(raw[key]), bits(w.data[:, 0])), key
    keys = sorted(raw)
    want = adjust_volume(np.stack([raw[key] for key in keys]), TARGET)
    for key, w in zip(keys, want):
        assert np.array_equal(bits(adj[key]), bits(w)), key
        assert not np.array_equal(bits(adj[key]), bits(raw[key]))
    # one signal at three levels: whatever the level, the models see (nearly) the same window
    for t in sorted({t for _, t in keys}):
        a, b, c = (adj[(k, t)] for k in SCALES)
        assert np.allclose(a, b, rtol=0, atol=1e-6) and np.allclose(a, c, rtol=0, atol=1e-6)


@pytest.mark.parametrize("mode", ["rings", "host", "vad"])
def test_default_engines_equal_pipelines_behind_the_block(gpu, audio, mode):
    """Device rings, host windows and ``pipeline="vad"``: every stream's turns equal those of its own batch-1 pipeline
    fed the same windows through the ``AdjustVolume`` block."""
    seg_sd = synth_segmentation_state(seed=31) if mode == "vad" else synth_segmentation_state()
    if mode == "vad":
        srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=4), None, max_streams=4, device=gpu, tau_active=0.5,
                           pipeline="vad", volume_in_db=TARGET)
        assert isinstance(srv.batch, VadBatch) and srv.rings is not None
    else:
        emb_sd = synth_embedding_state()
        srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=4), M.HipEmbedding(emb_sd, max_batch=4), max_streams=4,
                           device=gpu, device_rings=(mode == "rings"), volume_in_db=TARGET)
        assert isinstance(srv.batch, StreamBatch) and (srv.rings is not None) == (mode == "rings")
    feed(srv, audio)
    block = AdjustVolume(TARGET, gpu)
    turns = 0
    for k, x in audio.items():
        got = srv.close(k)
        if mode == "vad":
            cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=1),
                                               tau_active=0.5, device=gpu)
            pipe = VoiceActivityDetection(cfg)
        else:
            cfg = SpeakerDiarizationConfig(segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=1),
                                           embedding=M.EmbeddingModel.from_state(emb_sd, max_batch=1), device=gpu)
            pipe = SpeakerDiarization(cfg)
        acc = PredictionAccumulator(k)
        for w in windows_of(x):
            for out in pipe([block(w)]):
                acc.on_next(out)
        want = acc.get_prediction()
        assert want is not None and got.to_rttm() == want.to_rttm(), (mode, k)
        turns += len(got)
    if mode == "vad":
        assert turns > 0


def test_none_launches_nothing_and_bad_targets_are_refused(gpu, audio, monkeypatch):
    """The default leaves the windows as they are (no volume kernel is enqueued); a non-finite or non-numeric target is
    a ValueError before anything touches a device."""
    for bad in (float("nan"), float("inf"), "loud"):
        with pytest.raises(ValueError):
            StreamServer(None, None, max_streams=1, engine=lambda w, s, k: [], volume_in_db=bad)
        with pytest.raises(ValueError):          # models are not looked at before the check
            StreamServer(object(), object(), max_streams=1, volume_in_db=bad)
    from diart_amd import serve
    calls = []
    real = serve.adjust_volume_rows
    monkeypatch.setattr(serve, "adjust_volume_rows", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    seg_sd = synth_segmentation_state(seed=31)
    for target, expected in ((None, 0), (TARGET, 4)):
        calls.clear()
        srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=4), None, max_streams=4, device=gpu, tau_active=0.5,
                           pipeline="vad", volume_in_db=target)
        feed(srv, audio)
        assert len(calls) == expected
        torch.cuda.synchronize(gpu)
