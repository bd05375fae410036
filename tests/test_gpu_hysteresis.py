"""Hysteresis (tau_offset) on the GPU: the tuner's kernel with the lanes' state maps (tune_vad_score_kernel<TcHystRule>)
against the kernel's text on the host and the host tail; VadBatch, OverlapBatch, StreamServer and the file batch with tau_offset
against each stream's / file's own blocks pipeline.  The rule and the tuner's cases are tests/hysteresis_cases.py's."""
import gc
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hysteresis_cases as hc  # noqa: E402

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import (OverlappedSpeechDetection, OverlappedSpeechDetectionConfig, VoiceActivityDetection,  # noqa: E402
                              VoiceActivityDetectionConfig)
from diart_amd.features import SlidingWindow, SlidingWindowFeature  # noqa: E402
from diart_amd.pipeline import OverlapBatch, VadBatch  # noqa: E402
from diart_amd.synth import synth_segmentation_state, synth_stream, synth_streams  # noqa: E402

pytestmark = pytest.mark.gpu

W, SR = 80000, 16000
# per pipeline (tau_active, tau_offset): wide bands around the synthetic model's scores; every test checks for itself
# that the offset changes its turns (otherwise it would show nothing)
PAIRS = {"vad": (0.6, 0.3), "osd": (0.5, 0.2)}
KINDS = {"vad": (VoiceActivityDetection, VoiceActivityDetectionConfig, VadBatch, "speech"),
         "osd": (OverlappedSpeechDetection, OverlappedSpeechDetectionConfig, OverlapBatch, "overlap")}


# ---------------------------------------------------------------------------------------------------- 5. the tuner
def _bars(cache, per_file):
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_tuner_on_the_device(gpu, kind):
    """On the cases of the host test (files of 9, 60, 300 and 520 chunks: one, one, two and three steps per lane; a turn
    held across a hundred lanes by state alone, a file that begins inside the band, a NaN step inside a held turn,
    thresholds that meet a score): the masks of "gpu" equal those of "core" exactly, its components are within 1e-9 x
    total of "host" and the same doubles on a second call; (T,) input is what it was."""
    cache = hc.cache(kind)
    agg = cache.replay(np.array([hc.ON]), backend="host")[0]
    pairs = hc.trials(agg)
    agg_g, bits = cache.replay(pairs, backend="gpu")
    agg_c, bits_core = cache.replay(pairs, backend="core")
    assert np.array_equal(agg_g, agg_c, equal_nan=True)
    assert bits.dtype == np.uint32 and np.array_equal(bits, bits_core)
    assert np.array_equal(bits, cache.replay(pairs, backend="host")[1])
    for t in hc.BAND_TRIALS:
        assert (bits[t] != (agg > pairs[t, 0])).sum() > 100 and (bits[t] != (agg > pairs[t, 1])).sum() > 100
        assert np.array_equal(bits[t], hc.loop_bits(cache, agg, pairs[t]))
    host, got, again = (cache.evaluate(pairs, backend="host"), cache.evaluate(pairs, backend="gpu"),
                        cache.evaluate(pairs, backend="gpu"))
    bars = _bars(cache, host.per_file)
    print(f"{kind}: max |gpu - host| / bar = {(np.abs(got.per_file - host.per_file) / bars[..., None]).max():.3g}")
    assert (np.abs(got.per_file - host.per_file) <= bars[..., None]).all()
    assert np.array_equal(got.per_file, again.per_file) and np.array_equal(got.rate, again.rate)
    # (T,): today's kernels, and what (T, 2) with equal columns gives, bit for bit
    plain = cache.evaluate(pairs[:, 0], backend="gpu")
    equal = cache.evaluate(np.stack([pairs[:, 0], pairs[:, 0]], axis=1), backend="gpu")
    assert np.array_equal(plain.per_file, equal.per_file)
    assert (np.abs(plain.per_file - cache.evaluate(pairs[:, 0], backend="host").per_file) <= bars[..., None]).all()
    assert np.array_equal(cache.replay(pairs[:, 0], backend="gpu")[1], cache.replay(pairs[:, 0], backend="host")[1])


# ---------------------------------------------------------------------------------------------------- 6. engines
@pytest.fixture(scope="module")
def state():
    return synth_segmentation_state(seed=31)


def tracks(ann):
    return sorted((s.start, s.end, str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


def blocks_pipeline(kind, state, gpu, tau_offset, max_batch=1, **kw):
    pipeline_class, config_class = KINDS[kind][:2]
    return pipeline_class(config_class(segmentation=M.SegmentationModel.from_state(state, max_batch=max_batch),
                                       tau_active=PAIRS[kind][0], tau_offset=tau_offset, device=gpu, **kw))


def chunk(x, t, hop, start):
    return SlidingWindowFeature(x[t * hop:t * hop + W, None], SlidingWindow(start=start, duration=1 / SR, step=1 / SR))


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_engine_equals_per_stream_pipelines(gpu, state, kind):
    """4 streams x 12 steps with tau_offset, reset(slot) of stream 1 midway: every step's turns equal those of the
    stream's own blocks pipeline at batch 1 (for stream 1, of a pipeline that is reset and starts over at time 0)."""
    n, steps, hop, restart = 4, 12, 8000, 6
    on, off = PAIRS[kind]
    audio = synth_streams(n, (W + (steps - 1) * hop) / SR, seed0=600)
    dev = torch.from_numpy(audio).to(gpu)
    engine_class, label = KINDS[kind][2:]
    engine = engine_class(M.HipSegmentation(state, max_batch=n), n, tau_active=on, device=gpu, lanes=2, tau_offset=off)
    plain = engine_class(M.HipSegmentation(state, max_batch=n), n, tau_active=on, device=gpu, lanes=2)
    assert engine.tau_offset == off and plain.tau_offset is None
    got, without = [], []
    for t in range(steps):
        if t == restart:
            engine.reset(1)
            plain.reset(1)
        got.append(engine.detect(dev[:, t * hop:t * hop + W]))
        without.append(plain.detect(dev[:, t * hop:t * hop + W]))
    turns = differ = 0
    for i in range(n):
        ref = blocks_pipeline(kind, state, gpu, off)
        for t in range(steps):
            if i == 1 and t == restart:
                ref.reset()
            first = restart if i == 1 and t >= restart else 0
            (want, _), = ref([chunk(audio[i], t, hop, (t - first) * 0.5)])
            assert tracks(got[t][i]) == tracks(want), (i, t)
            assert all(lab == label for lab in got[t][i].labels())
            turns += len(tracks(want))
            differ += tracks(got[t][i]) != tracks(without[t][i])
    print(f"{kind}: {turns} turns, {differ} (stream, step) outputs changed by tau_offset")
    assert turns > 0 and differ > 0, "tau_offset changes no turn: the comparison shows nothing"


def test_stream_server_with_tau_offset_and_a_late_join(gpu, state):
    """StreamServer(pipeline="vad", tau_offset=): streams join late (the state of a joining stream is off) and push
    irregular amounts; each stream's stitched output is that of its own VoiceActivityDetection with tau_offset."""
    from diart_amd.inference import PredictionAccumulator, rolling_windows
    from diart_amd.serve import StreamServer
    on, off = PAIRS["vad"]
    audio = {k: synth_streams(1, v, seed0=820 + i)[0] for i, (k, v) in enumerate({"ann": 11.0, "ben": 8.5}.items())}

    def serve(tau_offset):
        srv = StreamServer(M.HipSegmentation(state, max_batch=4), None, max_streams=2, device=gpu, tau_active=on,
                           pipeline="vad", tau_offset=tau_offset)
        assert isinstance(srv.batch, VadBatch) and srv.batch.tau_offset == tau_offset
        rng = np.random.default_rng(5)
        pos, join_at, tick = {k: 0 for k in audio}, {"ann": 0, "ben": 3}, 0
        while any(pos[k] < len(audio[k]) for k in audio):
            for k in audio:
                if tick == join_at[k]:
                    srv.open(k)
                if tick >= join_at[k] and pos[k] < len(audio[k]):
                    m = int(rng.integers(SR // 8, SR * 2))
                    srv.push(k, audio[k][pos[k]:pos[k] + m])
                    pos[k] += m
            srv.step()
            tick += 1
        srv.drain()
        return {k: srv.close(k) for k in audio}

    got, without = serve(off), serve(None)
    assert any(got[k].to_rttm() != without[k].to_rttm() for k in audio), "tau_offset changes nothing here"
    for k in audio:
        pipe, acc = blocks_pipeline("vad", state, gpu, off), PredictionAccumulator(k)
        usable = len(audio[k]) // 8000 * 8000
        for w in rolling_windows((audio[k][None, i:i + 8000] for i in range(0, usable, 8000)), 5.0, 0.5, SR):
            for out in pipe([w]):
                acc.on_next(out)
        want = acc.get_prediction()
        assert want is not None and len(want) > 0 and got[k].to_rttm() == want.to_rttm(), k


def test_file_batch_and_benchmark_with_tau_offset(gpu, state, tmp_path):
    """Benchmark(VoiceActivityDetection) with tau_offset in the configuration on two short files: the file batch writes
    the RTTM files of the one-file-at-a-time loop byte for byte — on both paths the offset is the configuration's —
    and they are not those of the single threshold."""
    from diart_amd.inference import Benchmark, write_wav
    speech = tmp_path / "wav"
    speech.mkdir()
    for name, seed, dur in (("a", 11, 12.3), ("b", 12, 9.05)):
        write_wav(speech / f"{name}.wav", synth_stream(seed, dur), SR)

    def run(tag, tau_offset, k):
        cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel.from_state(state, max_batch=32),
                                           tau_active=PAIRS["vad"][0], tau_offset=tau_offset, device=gpu)
        out = tmp_path / tag
        b = Benchmark(speech, None, out, show_report=False, batch_size=32, concurrent_files=k)
        b(VoiceActivityDetection, cfg)
        path = b.last_path
        del b
        gc.collect()
        return path, {p.name: p.read_text() for p in sorted(out.iterdir())}

    off = PAIRS["vad"][1]
    loop_path, loop = run("loop", off, 0)
    batch_path, batch = run("batch", off, 2)
    _, single = run("single", None, 2)
    assert (loop_path, batch_path) == ("one_file_at_a_time", "file_batch")
    assert sorted(loop) == ["a.rttm", "b.rttm"] and any(len(t) > 0 for t in loop.values())
    assert batch == loop
    assert batch != single, "tau_offset changes nothing here"
    # FileBatch itself takes it, for both one-track forms
    from diart_amd.pipeline import FileBatch
    fb = FileBatch(M.HipSegmentation(state, max_batch=8), None, rows=8, max_files=2, pipeline="osd", tau_active=0.5,
                   tau_offset=0.2, device=gpu)
    assert fb.tau_offset == 0.2 and fb.engine.tau_offset is None      # (the files' tails carry it, not the engine's)
