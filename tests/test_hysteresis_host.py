"""Hysteresis (tau_offset) for VoiceActivityDetection and OverlappedSpeechDetection, without a GPU: the host tail
(dz_tail_set_offset), Binarize and the blocks, the tuner's host backends, the refusals, the Optimizer's bookkeeping and
the command line.  The yardstick of every test is the Python loop of tests/hysteresis_cases.py."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hysteresis_cases as hc  # noqa: E402
import tune_cases as tc  # noqa: E402
from tune_cases import scenarios  # noqa: E402

from diart_amd import _lib  # noqa: E402
from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.aggregation import BatchedOutputTail, DelayedAggregation  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.blocks.osd import OverlappedSpeechDetection, OverlappedSpeechDetectionConfig  # noqa: E402
from diart_amd.blocks.utils import Binarize  # noqa: E402
from diart_amd.blocks.vad import VoiceActivityDetection, VoiceActivityDetectionConfig  # noqa: E402
from diart_amd.features import Annotation, Segment, SlidingWindow, SlidingWindowFeature  # noqa: E402
from diart_amd.inference import PredictionAccumulator  # noqa: E402
from diart_amd.metrics import COMPONENTS, DetectionErrorRate, OverlapDetectionErrorRate  # noqa: E402
from diart_amd.optim import Optimizer, OsdTuneCache, TuneCache, VadTuneCache  # noqa: E402

SR = 16                      # the chunks only carry their time axis: 80 samples of 5 s
BATCH = 7
PIPELINES = {"vad": (VoiceActivityDetection, VoiceActivityDetectionConfig, DetectionErrorRate),
             "osd": (OverlappedSpeechDetection, OverlappedSpeechDetectionConfig, OverlapDetectionErrorRate)}


def _config(kind, latency=hc.LATENCY, tau=hc.ON, tau_offset=None):
    return PIPELINES[kind][1](segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()), latency=latency,
                              tau_active=tau, tau_offset=tau_offset, device=torch.device("cpu"))


def _chunks(starts):
    return [SlidingWindowFeature(np.zeros((int(tc.DURATION * SR), 1), dtype=np.float32),
                                 SlidingWindow(start=float(s), duration=1.0 / SR, step=1.0 / SR)) for s in starts]


def _scores(kind, track):
    """Segmentation scores (batch, frames, speakers) whose track is ``track``: one speaker for the max, the same score
    twice for the second largest."""
    t = torch.from_numpy(np.ascontiguousarray(track))[:, :, None]
    return t if kind == "vad" else torch.cat([t, t], dim=2)


# ---------------------------------------------------------------------------------------------------- 1. the tail
def _signal(t, g):
    """Slow waves around the band, one per speaker column: a score stays inside (0.4, 0.6] for many frames in a row."""
    return 0.5 + 0.3 * np.sin(2 * np.pi * t / (3.1 + 1.7 * g) + 0.9 * g)


def _stream(F, G, steps, seed, nan_step=None):
    rng = np.random.default_rng(seed)
    res = tc.DURATION / F
    out = []
    for c in range(steps):
        start = tc.STEP * c
        t = start + (np.arange(F) + 0.5) * res
        s = np.stack([_signal(t, g) for g in range(G)], axis=1) + 0.02 * rng.standard_normal((F, G))
        if c == nan_step:
            s[:] = np.nan
        out.append((start, np.ascontiguousarray(s, dtype=np.float64)))
    return out, res


def _run_tail(tail, stream, res):
    """Per step: (the aggregated rows, t0, res, the turns as a list of tuples)."""
    out = []
    for start, scores in stream:
        agg, rows, t0, r, turns, nturns = tail(scores[None], start, res)
        out.append((agg[0, :rows[0]].copy(), float(t0[0]), float(r[0]), [tuple(x) for x in turns[0, :nturns[0]]]))
    return out


@pytest.mark.parametrize("latency", [0.5, 2.5, 5.0])
def test_tail_rule(latency):
    """dz_tail_step with an offset against the loop applied to the tail's own aggregated rows: the turns are equal as
    (start, end, speaker), bit for bit, over 3 speaker columns, the first chunk's prepended rows, a NaN step in the
    middle and dz_tail_reset; a step ends while a column is on and the next one starts inside the band."""
    F, G, steps = 32, 3, 40
    stream, res = _stream(F, G, steps, seed=int(10 * latency), nan_step=17)
    tail = BatchedOutputTail(1, F, G, tc.STEP, latency, threshold=hc.ON, offset=hc.OFF, num_threads=1)
    plain = BatchedOutputTail(1, F, G, tc.STEP, latency, threshold=hc.ON, num_threads=1)
    got, base_ = _run_tail(tail, stream, res), _run_tail(plain, stream, res)
    state = [False] * G
    carried = held = differ = 0
    assert len(got[0][0]) > len(got[1][0]) or latency == tc.DURATION     # the first chunk's prepend (none at the full latency)
    for c, ((agg, t0, r, turns), (agg0, _, _, turns0)) in enumerate(zip(got, base_)):
        assert np.array_equal(agg, agg0, equal_nan=True)
        want = []
        for g in range(G):
            first_in_band = hc.OFF < agg[0, g] <= hc.ON
            carried += state[g] and first_in_band
            on, state[g] = hc.hysteresis(agg[:, g], hc.ON, hc.OFF, state[g])
            held += state[g]
            want += hc.turns_of(on, t0, r, g)
        assert turns == want, c
        differ += turns != turns0
    assert np.isnan(got[17][0]).all() and not any(got[17][3])    # the NaN step: off, and the state is off behind it
    assert carried >= 3 and held >= 10 and differ >= 5, (carried, held, differ)
    # dz_tail_reset: the states are cleared and the offset is kept — the same stream again gives the same turns
    tail.reset()
    assert [x[3] for x in _run_tail(tail, stream, res)] == [x[3] for x in got]
    # reset(slot) in the middle of a held turn: the next step starts a stream, with the state off
    tail.reset()
    _run_tail(tail, stream[:8], res)
    tail.reset(0)
    assert [x[3] for x in _run_tail(tail, stream[:3], res)] == [x[3] for x in got[:3]]


def test_tail_offset_equal_to_threshold_and_untouched():
    """offset == threshold is `score > threshold`, row for row: the turns of a tail on which dz_tail_set_offset was never
    called, which in turn runs the code it always ran."""
    F, G = 32, 3
    stream, res = _stream(F, G, 30, seed=5, nan_step=9)
    make = lambda **kw: BatchedOutputTail(1, F, G, tc.STEP, 2.5, threshold=hc.ON, num_threads=1, **kw)
    untouched, equal = _run_tail(make(), stream, res), _run_tail(make(offset=hc.ON), stream, res)
    assert [x[3] for x in equal] == [x[3] for x in untouched] and sum(len(x[3]) for x in untouched) > 20
    for a, b in zip(equal, untouched):
        assert np.array_equal(a[0], b[0], equal_nan=True)


def test_tail_refusals():
    lib = _lib.load()
    h = _lib.vp()
    ham = np.hamming(8)
    assert lib.dz_tail_create(8, 2, 0.5, 0.5, 0.6, 0, 1, ham.ctypes.data, C_byref(h)) == 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert lib.dz_tail_set_offset(h, bad) == 2
        assert "dz_tail_set_offset" in lib.dz_last_error().decode()
    assert lib.dz_tail_set_offset(None, 0.4) == 2 and "dz_tail_set_offset" in lib.dz_last_error().decode()
    assert lib.dz_tail_set_offset(h, 0.4) == 0 and lib.dz_tail_set_offset(h, 0.9) == 0      # above the threshold: defined
    lib.dz_tail_destroy(h)
    for bad in (float("nan"), float("inf"), "low", [0.4]):
        with pytest.raises(ValueError, match="tau_offset"):
            BatchedOutputTail(1, 8, 1, 0.5, 0.5, offset=bad)
        with pytest.raises(ValueError, match="tau_offset"):
            Binarize(0.6, offset=bad)
        with pytest.raises(ValueError, match="tau_offset"):
            _config("vad", tau_offset=bad)
        with pytest.raises(ValueError, match="tau_offset"):
            _config("osd", tau_offset=bad)


def C_byref(x):
    import ctypes
    return ctypes.byref(x)


# ---------------------------------------------------------------------------------------------------- 2. the blocks
def test_binarize_offset():
    rng = np.random.default_rng(3)
    sw = SlidingWindow(start=1.25, duration=0.02, step=0.02)
    binarize, state, carried = Binarize(hc.ON, offset=hc.OFF), [False, False, False], 0
    assert Binarize(hc.ON).offset is None
    for call in range(6):
        t = call * 50 + np.arange(50)
        data = np.stack([0.5 + 0.3 * np.sin(t / (7.0 + 3 * g) + g) for g in range(3)], axis=1) + 0.02 * rng.standard_normal((50, 3))
        if call == 3:
            data[10:20, 1] = np.nan
        ann = binarize(SlidingWindowFeature(data, sw))
        want = []
        for g in range(3):
            on, state[g] = hc.hysteresis(data[:, g], hc.ON, hc.OFF, state[g])
            want += [(s, e, f"speaker{g}") for s, e, _ in hc.turns_of(on, sw.start, sw.step, g)]
        got = [(seg.start, seg.end, label) for seg, _, label in ann.itertracks(yield_label=True)]
        assert sorted(got) == sorted(want) and (call == 0 or len(want) > 0)
        carried += sum(state)                       # columns whose state crosses into the next call switched on
    assert carried >= 3
    band = np.full((5, 3), hc.BAND)
    binarize(SlidingWindowFeature(np.full((5, 3), hc.HIGH), sw))
    assert len(binarize(SlidingWindowFeature(band, sw))) == 3     # inside the band behind a call that ended on: held
    binarize.reset()
    assert len(binarize(SlidingWindowFeature(band, sw))) == 0     # inside the band from a cleared state: off
    # offset == threshold: the stateless rule
    both = Binarize(hc.ON, offset=hc.ON)(SlidingWindowFeature(data, sw)), Binarize(hc.ON)(SlidingWindowFeature(data, sw))
    assert [(s.start, s.end, l) for s, _, l in both[0].itertracks(yield_label=True)] == \
        [(s.start, s.end, l) for s, _, l in both[1].itertracks(yield_label=True)]


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_blocks_finalise_with_tau_offset(kind):
    """finalise with tau_offset against the loop on the rows of a DelayedAggregation of its own; reset() clears the state."""
    pipeline_class = PIPELINES[kind][0]
    track = hc.tracks(kind)[2][:90]                 # rise, band, the NaN chunk, band
    chunks = _chunks(tc.starts_for(len(track)))
    pipeline = pipeline_class(_config(kind, tau_offset=hc.OFF))
    assert pipeline.binarize.offset == hc.OFF and [p.name for p in pipeline.hyper_parameters()] == ["tau_active"]
    aggregation = DelayedAggregation(tc.STEP, hc.LATENCY, strategy="hamming", cropping_mode="loose")
    buffer, state, held, outputs = [], False, 0, []
    for i in range(0, len(chunks), BATCH):
        outputs += pipeline.finalise(chunks[i:i + BATCH], _scores(kind, track[i:i + BATCH]))
    res = chunks[0].extent.duration / hc.F
    for c, (ann, _) in enumerate(outputs):
        sw = SlidingWindow(start=chunks[c].extent.start, duration=res, step=res)
        buffer.append(SlidingWindowFeature(track[c][:, None], sw))
        agg = aggregation(buffer)
        if len(buffer) == aggregation.num_overlapping_windows:
            buffer = buffer[1:]
        on, state = hc.hysteresis(agg.data[:, 0].astype(np.float64), hc.ON, hc.OFF, state)
        held += state
        want = [(agg.sliding_window[int(a)].middle, agg.sliding_window[int(b)].middle) for a, b in
                [(round((s - agg.sliding_window.start) / agg.sliding_window.step - 0.5),
                  round((e - agg.sliding_window.start) / agg.sliding_window.step - 0.5))
                 for s, e, _ in hc.turns_of(on, agg.sliding_window.start, agg.sliding_window.step)]]
        got = [(seg.start, seg.end) for seg, _, label in ann.itertracks(yield_label=True)]
        assert got == want, c
        assert {label for _, _, label in ann.itertracks(yield_label=True)} <= {pipeline_class.LABEL}
    assert 40 <= held < 70 and not state            # held by state alone up to the NaN chunk, off behind it
    # reset() clears the state: a stream that begins inside the band stays off; without reset() it would not
    band = np.full((1, hc.F), hc.BAND, dtype=np.float32)
    held_pipeline = pipeline_class(_config(kind, tau_offset=hc.OFF))
    held_pipeline.finalise(chunks[:20], _scores(kind, track[:20]))
    assert held_pipeline.binarize._state.all()
    held_pipeline.reset()
    assert len(held_pipeline.finalise(chunks[:1], _scores(kind, band))[0][0]) == 0


# ---------------------------------------------------------------------------------------------------- 3. the tuner
def _python_path(kind, f, pair):
    """The existing path: finalise on the cached tracks, batch by batch, then PredictionAccumulator."""
    pipeline = PIPELINES[kind][0](_config(kind, tau=float(pair[0]), tau_offset=float(pair[1])))
    pipeline.set_timestamp_shift(f["shift"])
    acc = PredictionAccumulator(f["uri"])
    chunks = _chunks(f["starts"])
    for i in range(0, len(chunks), BATCH):
        for out in pipeline.finalise(chunks[i:i + BATCH], _scores(kind, f["track"][i:i + BATCH])):
            acc.on_next(out)
    return acc.get_prediction()


def _table(ann):
    return sorted((seg.start, seg.end, str(label)) for seg, _, label in ann.support().itertracks(yield_label=True))


def _reference(f):
    ann = Annotation(uri=f["uri"])
    for n, (s, e, label) in enumerate(f["reference"]):
        ann[Segment(s, e), n] = label
    return ann


def _bars(cache, per_file):
    """1e-9 x total per file; where a file's total is 0, 1e-9 x the sum of its cells' durations."""
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


def _files_with_batch_resolution(kind):
    """hc.files with the frame resolution finalise computes: from the first chunk of every batch."""
    files = hc.files(kind)
    for f in files:
        chunks, res = _chunks(f["starts"]), []
        for i in range(0, len(chunks), BATCH):
            res += [chunks[i].extent.duration / hc.F] * len(chunks[i:i + BATCH])
        f["res"] = np.array(res)
    return files


def check_case(cache, agg, pairs, bits):
    """The conditions without which the case shows nothing: for the band trials the masks differ from the plain masks at
    tau_active and from those at tau_offset; a turn is held across dozens of lanes by state alone; a file begins inside
    the band and stays off; a NaN step lies inside a held turn; both thresholds of the tie trial meet a score."""
    for t in hc.BAND_TRIALS:
        assert (bits[t] != (agg > pairs[t, 0])).sum() > 100 and (bits[t] != (agg > pairs[t, 1])).sum() > 100
    assert (agg == pairs[1, 0]).any() and (agg == pairs[1, 1]).any()
    ro, co, fro = cache.row_off, cache.chunk_off, cache.file_row_off
    in_band = (agg > hc.OFF) & (agg <= hc.ON)
    full = lambda s: bool(in_band[ro[s]:ro[s + 1]].all() and bits[0][ro[s]:ro[s + 1]].all())
    run = best = start = 0
    for s in range(int(co[3]), int(co[4])):
        run = run + 1 if full(s) else 0
        if run > best:
            best, start = run, s - run + 1
    assert best >= 40 * 3                            # 120 steps: at three steps per lane, 40 lanes
    assert (agg[ro[start - 6]:ro[start]] > hc.ON).any()                        # a row above tau_active before them
    end = start + best
    assert (agg[ro[end]:ro[end + 6]] <= hc.OFF).any() and not bits[0][ro[end + 6]]
    b0 = int(fro[1])
    assert in_band[b0:b0 + 60].all() and not bits[0][b0:b0 + 60].any()
    nan_rows = np.nonzero(np.isnan(agg[fro[2]:fro[3]]))[0] + int(fro[2])
    assert len(nan_rows) and bits[0][nan_rows[0] - 1] and not bits[0][nan_rows].any()
    after = int(nan_rows[-1]) + 1
    assert in_band[after:after + 60].all() and not bits[0][after:after + 60].any()


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_tuner_host_against_python(kind):
    """Per trial and file the "host" backend's hypothesis has the turns of finalise + PredictionAccumulator with that
    (tau_active, tau_offset), and the components are the pipeline's metric's on that prediction within 1e-9 x total;
    "core" — the kernel's text, 256 lanes played in order — has the same masks exactly and the components within the same
    bar; (T, 2) with equal columns gives the per-file results of (T,) bit for bit."""
    cache_class, metric_class = {"vad": VadTuneCache, "osd": OsdTuneCache}[kind], PIPELINES[kind][2]
    files = _files_with_batch_resolution(kind)
    cache = cache_class.from_arrays(files, _config(kind))
    agg = cache.replay(np.array([hc.ON]), backend="host")[0]
    pairs = hc.trials(agg)
    agg_h, bits = cache.replay(pairs, backend="host")
    agg_c, bits_core = cache.replay(pairs, backend="core")
    assert np.array_equal(agg_h, agg, equal_nan=True) and np.array_equal(agg_c, agg, equal_nan=True)
    assert bits.dtype == np.uint32 and bits.shape == (len(pairs), cache.total_rows) and np.array_equal(bits, bits_core)
    for t, pair in enumerate(pairs):
        assert np.array_equal(bits[t], hc.loop_bits(cache, agg, pair)), t
    assert np.array_equal(bits[2], (agg > hc.ON).astype(np.uint32))
    assert not np.array_equal(bits[4], bits[0])
    assert [len(f["track"]) for f in files] == list(hc.CHUNKS)
    check_case(cache, agg, pairs, bits)
    host, core = cache.evaluate(pairs, backend="host"), cache.evaluate(pairs, backend="core")
    assert np.array_equal(host.per_file, cache.score(bits)) and (host.status == -1).all()
    bars = _bars(cache, host.per_file)
    assert (np.abs(host.per_file - core.per_file) <= bars[..., None]).all()
    turns = 0
    for t, pair in enumerate(pairs):
        for n, f in enumerate(files):
            want = _python_path(kind, f, pair)
            assert _table(cache.hypothesis(bits[t], n)) == _table(want), (t, n)
            turns += len(_table(want))
            comp = metric_class().components(_reference(f), want)
            for i, c in enumerate(COMPONENTS):
                assert abs(host.per_file[t, n, i] - comp[c]) <= bars[t, n], (t, n, c, host.per_file[t, n, i], comp[c])
    assert turns > 50
    for backend in ("host", "core"):
        plain = cache.evaluate(pairs[:, 0], backend=backend)
        equal = cache.evaluate(np.stack([pairs[:, 0], pairs[:, 0]], axis=1), backend=backend)
        assert np.array_equal(plain.per_file, equal.per_file) and np.array_equal(plain.rate, equal.rate)


# ---------------------------------------------------------------------------------------------------- 4. refusals, Optimizer
def _dia_config(**kw):
    return SpeakerDiarizationConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                    embedding=M.EmbeddingModel(lambda: scenarios.ToyEmbedding()), latency=2.5,
                                    device=torch.device("cpu"), **kw)


def _small_cache(kind="vad"):
    files = hc.files(kind)[:2]
    return {"vad": VadTuneCache, "osd": OsdTuneCache}[kind].from_arrays(files, _config(kind))


def test_refusals(tmp_path):
    cache = _small_cache()
    for bad in (np.array([[0.6, np.nan]]), np.array([[0.6, np.inf]]), [[0.6, "x"]]):
        for backend in ("host", "core", "gpu"):
            with pytest.raises(ValueError, match="tau_offset|numbers"):
                cache.evaluate(bad, backend=backend)
            with pytest.raises(ValueError, match="tau_offset|numbers"):
                cache.replay(bad, backend=backend)
    with pytest.raises(ValueError, match=r"\(T, 2\)"):
        cache.evaluate(np.zeros((2, 3)), backend="host")
    with pytest.raises(ValueError, match=r"\(T, 2\)"):
        cache.evaluate(np.zeros((0, 2)), backend="host")
    # the C entry points: status 2 and a message that names the function
    lib, taus = _lib.load(), np.array([[0.6, np.nan]])
    import ctypes as C
    d = cache._desc(lambda name: getattr(cache, name).ctypes.data)
    agg, bits = np.empty(cache.total_rows), np.empty((1, cache.total_rows), dtype=np.uint32)
    cells = C.byref(cache._host_cells())
    assert lib.dz_tune_vad_host(C.byref(d), cells, 2, taus.ctypes.data, 1, agg.ctypes.data, bits.ctypes.data, 256, None, 1) == 2
    assert "dz_tune_vad_host: tau_offset" in lib.dz_last_error().decode()
    assert lib.dz_tune_vad_host(C.byref(d), cells, 1, np.array([0.6]).ctypes.data, 1, agg.ctypes.data, bits.ctypes.data,
                                257, None, 1) == 2   # lanes
    assert "dz_tune_vad_host:" in lib.dz_last_error().decode()
    assert lib.dz_tune_vad_replay_tails(C.byref(d), taus.ctypes.data, 1, 0.5, 2.5, cache.starts.ctypes.data,
                                        cache.res.ctypes.data, bits.ctypes.data, 1) == 2
    assert "dz_tune_vad_replay_tails" in lib.dz_last_error().decode()
    # SpeakerDiarization, anywhere
    with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
        _dia_config(tau_offset=0.4)
    config = _dia_config()
    config.tau_offset = 0.4
    with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
        SpeakerDiarization(config)
    with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "a", base_config=config)
    dia = TuneCache.from_arrays([tc.file_of(*tc.random_outputs(1, 5, 16, 3, 8))], tc.config_of(0.6, 0.3, 1.0, 4, 2.5))
    with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "b", base_config=_dia_config(), cache=dia,
                  hparams=[base.TauActive, base.TauOffset])
    with pytest.raises(ValueError, match=r"hparams \(T, 3\)"):
        dia.evaluate(np.zeros((2, 2)), backend="host")
    from diart_amd.pipeline import FileBatch, StreamBatch, WeSpeakerBatch
    from diart_amd.serve import StreamServer
    for engine in (StreamBatch, WeSpeakerBatch):
        with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
            engine(None, None, 4, tau_offset=0.4)
    with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
        FileBatch(None, None, tau_offset=0.4)
    with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
        StreamServer(None, None, tau_offset=0.4)
    for bad in (float("nan"), "low"):
        with pytest.raises(ValueError, match="tau_offset"):
            StreamServer(None, None, pipeline="vad", tau_offset=bad)
        with pytest.raises(ValueError, match="tau_offset"):
            FileBatch(None, None, pipeline="osd", tau_offset=bad)
    assert base.HyperParameter.from_name("tau_offset") is base.TauOffset
    assert (base.TauOffset.name, base.TauOffset.low, base.TauOffset.high) == ("tau_offset", 0, 1)


def _optimizer(tmp_path, cache, kind="vad", **kw):
    kw.setdefault("base_config", _config(kind))
    return Optimizer(PIPELINES[kind][0], None, None, tmp_path / "study", cache=cache, backend="host", **kw)


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_optimizer_bookkeeping(tmp_path, kind):
    cache = _small_cache(kind)
    calls = []
    evaluate = cache.evaluate

    def counting(taus, **kw):
        calls.append(np.array(taus))
        return evaluate(taus, **kw)

    cache.evaluate = counting
    # the default stays tau_active alone, (T, 1) trials: today's kernels
    plain = _optimizer(tmp_path / "plain", cache, kind, seed=3)
    assert [p.name for p in plain.hparams] == ["tau_active"]
    plain(3, show_progress=False)
    assert [c.shape for c in calls] == [(3, 1)]
    calls.clear()
    both = [base.TauActive, base.TauOffset]
    opt = _optimizer(tmp_path, cache, kind, seed=3, trials_per_batch=4, hparams=both)
    opt(10, show_progress=False)
    assert [c.shape for c in calls] == [(4, 2), (4, 2), (2, 2)] and len(opt.trials) == 10
    assert opt.trials[0]["params"] == {"tau_active": hc.ON, "tau_offset": hc.ON}     # kick-start: None is tau_active
    assert all(list(t["params"]) == ["tau_active", "tau_offset"] for t in opt.trials)
    pairs = np.concatenate(calls)
    assert np.array_equal(pairs, np.array([[t["params"]["tau_active"], t["params"]["tau_offset"]] for t in opt.trials]))
    rates = evaluate(pairs, backend="host").rate
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * rates)
    assert opt.best_performance == 100.0 * rates.min() and set(opt.best_hparams) == {"tau_active", "tau_offset"}
    # continuing the stored study; a study of other hyper-parameters is refused
    calls.clear()
    again = _optimizer(tmp_path, cache, kind, seed=3, trials_per_batch=4, hparams=both)
    assert again.trials == opt.trials
    again(3, show_progress=False)
    assert [c.shape for c in calls] == [(3, 2)] and [t["number"] for t in again.trials] == list(range(13))
    assert json.loads((tmp_path / "study" / "study.json").read_text())["hparams"] == ["tau_active", "tau_offset"]
    with pytest.raises(ValueError, match="holds a study of"):
        _optimizer(tmp_path, cache, kind)
    # grid: the largest square of at most num_iter points
    calls.clear()
    grid = _optimizer(tmp_path / "grid", cache, kind, sampler="grid", do_kickstart_hparams=False, hparams=both)
    grid(9, show_progress=False)
    assert sorted({t["params"]["tau_offset"] for t in grid.trials}) == pytest.approx([0.25, 0.5, 0.75]) and len(grid.trials) == 9
    # tau_offset not tuned: every trial's offset is the base configuration's
    calls.clear()
    fixed = _optimizer(tmp_path / "fixed", cache, kind, seed=1, base_config=_config(kind, tau_offset=0.3))
    fixed(4, show_progress=False)
    assert calls[0].shape == (4, 2) and (calls[0][:, 1] == 0.3).all() and calls[0][0, 0] == hc.ON
    assert all(list(t["params"]) == ["tau_active"] for t in fixed.trials)
    # tau_offset alone: tau_active is the base configuration's
    calls.clear()
    alone = _optimizer(tmp_path / "alone", cache, kind, seed=1, hparams=[base.TauOffset])
    alone(3, show_progress=False)
    assert calls[0].shape == (3, 2) and (calls[0][:, 0] == hc.ON).all()


def test_command_line(tmp_path):
    from diart_amd import tune
    _small_cache().save(tmp_path / "vad.npz")
    common = [str(tmp_path), "--reference", str(tmp_path), "--num-iter", "5", "--seed", "2", "--latency", "2.5", "--cpu",
              "--tau-active", "0.6"]
    vad = common + ["--pipeline", "VoiceActivityDetection", "--cache", str(tmp_path / "vad.npz")]
    models = (M.SegmentationModel(lambda: scenarios.ToySegmentation()), None)
    opt = tune.run(tune.parser().parse_args(vad + ["--output", str(tmp_path / "s1"), "--tau-offset", "0.35", "--hparams",
                                                   "tau_active", "tau_offset"]), models=models)
    assert [p.name for p in opt.hparams] == ["tau_active", "tau_offset"] and opt.base_config.tau_offset == 0.35
    assert opt.trials[0]["params"] == {"tau_active": 0.6, "tau_offset": 0.35} and len(opt.trials) == 5
    # --hparams still defaults to tau_active; --tau-offset then holds in every trial
    opt = tune.run(tune.parser().parse_args(vad + ["--output", str(tmp_path / "s2"), "--tau-offset", "0.35"]), models=models)
    assert all(list(t["params"]) == ["tau_active"] for t in opt.trials) and opt.base_config.tau_offset == 0.35
    opt = tune.run(tune.parser().parse_args(vad + ["--output", str(tmp_path / "s3")]), models=models)
    assert opt.base_config.tau_offset is None and [p.name for p in opt.hparams] == ["tau_active"]
    for extra in (["--tau-offset", "0.4"], ["--hparams", "tau_active", "tau_offset"]):
        with pytest.raises(SystemExit, match="tau_offset is not a parameter of SpeakerDiarization"):
            tune.run(tune.parser().parse_args(common + ["--output", str(tmp_path / "s4")] + extra),
                     models=(models[0], M.EmbeddingModel(lambda: scenarios.ToyEmbedding())))


def test_binarize_refuses_a_changed_column_count():
    """The state is per column: a call with another column count than the call before is a caller's mistake."""
    sw = SlidingWindow(start=0.0, duration=0.02, step=0.02)
    binarize = Binarize(hc.ON, offset=hc.OFF)
    binarize(SlidingWindowFeature(np.full((4, 3), hc.HIGH), sw))
    with pytest.raises(ValueError, match="3"):
        binarize(SlidingWindowFeature(np.full((4, 2), hc.HIGH), sw))
    binarize.reset()
    assert len(binarize(SlidingWindowFeature(np.full((4, 2), hc.HIGH), sw))) == 2


def test_tail_status_5_and_the_groups_front_door():
    """More turns than max_turns is status 5 with hysteresis as without; StreamBatch's re-dispatch to GroupsBatch refuses
    tau_offset like the engines themselves."""
    F = 8
    scores = np.ascontiguousarray(np.array([0.9, 0.1] * (F // 2), dtype=np.float64)[:, None])   # four turns
    for offset in (None, hc.OFF):
        tail = BatchedOutputTail(1, F, 1, tc.STEP, tc.STEP, threshold=hc.ON, offset=offset, num_threads=1, max_turns=2)   # (the first chunk: every row)
        with pytest.raises(_lib.DiartAmdError, match="more speech turns than max_turns"):
            tail(scores[None], 0.0, tc.DURATION / F)
    from diart_amd.models import _HipGroupsEmbedding
    from diart_amd.pipeline import GroupsBatch, StreamBatch
    groups = object.__new__(_HipGroupsEmbedding)
    for make in (StreamBatch, GroupsBatch):
        with pytest.raises(ValueError, match="tau_offset is not a parameter of SpeakerDiarization"):
            make(None, groups, 4, tau_offset=0.4)
