"""Minimum durations (min_duration_on / min_duration_off) of VoiceActivityDetection and OverlappedSpeechDetection,
without a GPU: functional.min_duration, the tuner's host backends ("core": the kernel's text with its lanes played in
order; "host": the sequential text behind the dz_tail masks), the refusals, the Optimizer, the command line, the
accumulated prediction and Benchmark's loop, and the host code under AddressSanitizer + UBSan in a program of its own.
The yardstick of every test is the Python loop of tests/min_duration_cases.py."""
import ctypes as C
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hysteresis_cases as hc  # noqa: E402
import min_duration_cases as mc  # noqa: E402
import tune_cases as tc  # noqa: E402
from tune_cases import scenarios  # noqa: E402

from diart_amd import _lib, functional  # noqa: E402
from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.blocks.osd import OverlappedSpeechDetection, OverlappedSpeechDetectionConfig  # noqa: E402
from diart_amd.blocks.vad import VoiceActivityDetection, VoiceActivityDetectionConfig  # noqa: E402
from diart_amd.features import Annotation, Segment  # noqa: E402
from diart_amd.inference import Benchmark, PredictionAccumulator, write_wav  # noqa: E402
from diart_amd.metrics import COMPONENTS, DetectionErrorRate, OverlapDetectionErrorRate  # noqa: E402
from diart_amd.optim import Optimizer, OsdTuneCache, TuneCache, VadTuneCache  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
PIPELINES = {"vad": (VoiceActivityDetection, VoiceActivityDetectionConfig, DetectionErrorRate),
             "osd": (OverlappedSpeechDetection, OverlappedSpeechDetectionConfig, OverlapDetectionErrorRate)}


def _config(kind, **kw):
    return PIPELINES[kind][1](segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()), latency=hc.LATENCY,
                              tau_active=hc.ON, device=torch.device("cpu"), **kw)


def _bars(cache, per_file):
    """1e-9 x total per file; where a file's total is 0, 1e-9 x the sum of its cells' durations."""
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


def _reference(f):
    ann = Annotation(uri=f["uri"])
    for n, (s, e, label) in enumerate(f["reference"]):
        ann[Segment(s, e), n] = label
    return ann


# ---------------------------------------------------------------------------------------------------- 1. the rule
def _random_turns(rng, count):
    """Turns on a 0.01 s grid with gaps of 0 .. 0.3 s, some overlapping, some of zero gap."""
    out, t = [], float(rng.uniform(0, 2))
    for _ in range(count):
        t += float(rng.choice([0.0, 0.01, 0.04, 0.05, 0.06, 0.1, 0.2, 0.3])) - (0.15 if rng.random() < 0.1 else 0.0)
        d = float(rng.choice([0.01, 0.05, 0.1, 0.2, 0.25, 0.5, 1.0]))
        out.append((t, t + d))
        t += d
    return out


def test_functional_min_duration_against_the_loop():
    rng = np.random.default_rng(7)
    changed = 0
    for case in range(300):
        per_label = {label: _random_turns(rng, int(rng.integers(1, 25))) for label in ("a", "b")[:1 + case % 2]}
        ann = Annotation(uri="x", modality="speech")
        for label, turns in per_label.items():
            for n, (s, e) in enumerate(turns):
                ann[Segment(s, e), f"{label}{n}"] = label
        on, off = [float(rng.choice([0.0, 0.05, 0.1, 0.2, 0.25, 0.31, 1.0])) for _ in range(2)]
        got = functional.min_duration(ann, on, off)
        assert type(got) is Annotation and got.uri == "x"
        for label, turns in per_label.items():
            want = mc.min_duration(turns, on, off)
            assert sorted((s.start, s.end) for s, _, l in got.itertracks(yield_label=True) if l == label) == want, (case, label)
            changed += want != mc.support(turns, mc.PATCH_COLLAR)
        if on == 0.0 and off == 0.0:
            assert got.to_rttm() == ann.support(0.05).to_rttm()
    assert changed > 100
    pair = [(0.0, 0.25), (0.5, 0.75)]                                  # strict: a 0.25 s turn and a 0.25 s gap stay
    for rule in (mc.min_duration, lambda t, on, off: mc.turns_of(functional.min_duration(mc.annotation_of(t, "x", "s"), on, off))):
        assert rule(pair, 0.25, 0.25) == pair and rule(pair, 0.26, 0.25) == [] and rule(pair, 0.26, 0.26) == [(0.0, 0.75)]
    for bad in (-0.1, float("nan"), float("inf"), "long"):
        with pytest.raises(ValueError, match="min_duration_on"):
            functional.min_duration(Annotation(), bad, 0.0)
        with pytest.raises(ValueError, match="min_duration_off"):
            functional.min_duration(Annotation(), 0.0, bad)


def test_support_twice_is_support_of_the_maximum():
    rng = np.random.default_rng(11)
    for case in range(500):
        turns = _random_turns(rng, int(rng.integers(1, 30)))
        a, b = float(rng.choice([0.0, 0.05, 0.1, 0.2, 0.31])), float(rng.choice([0.0, 0.04, 0.05, 0.1, 0.25]))
        assert mc.support(mc.support(turns, a), b) == mc.support(turns, max(a, b)), case
        ann = mc.annotation_of(turns, "x", "speech")
        assert mc.turns_of(ann.support(a).support(b)) == mc.turns_of(ann.support(max(a, b))) == mc.support(turns, max(a, b))


# ---------------------------------------------------------------------------------------------------- 2. the tuner
@pytest.fixture(scope="module", params=["vad", "osd"])
def case(request):
    kind = request.param
    cache, files = mc.cache(kind), mc.files(kind)
    quads = mc.trials(cache)
    bits = cache.replay(quads, backend="host")[1]
    return kind, cache, files, quads, bits


def test_trials_show_something(case):
    _, cache, files, quads, bits = case
    assert [len(f["track"]) for f in files] == list(hc.CHUNKS) + [1] and len(quads) == len(mc.NAMES)
    mc.check_trials(cache, quads, bits)


def test_masks_are_those_of_the_first_two_columns(case):
    _, cache, _, quads, bits = case
    assert bits.dtype == np.uint32 and bits.shape == (len(quads), cache.total_rows)
    assert np.array_equal(bits, cache.replay(quads[:, :2], backend="host")[1])
    assert np.array_equal(bits, cache.replay(quads, backend="core")[1])
    assert np.array_equal(bits, cache.replay(quads[:, :2], backend="core")[1])


def test_core_and_host_against_the_python_chain(case):
    """hypothesis() of the masks -> the Python rule -> the metric's components: "core" and "host" agree with it within
    1e-9 x total per component, for every trial and file, the one-chunk file included."""
    kind, cache, files, quads, bits = case
    core, host = cache.evaluate(quads, backend="core"), cache.evaluate(quads, backend="host")
    bars = _bars(cache, host.per_file)
    assert (host.status == -1).all() and host.per_file.shape == (len(quads), 5, 5)
    turns = 0
    for t, (_, _, on, off) in enumerate(quads):
        for n, f in enumerate(files):
            kept = mc.min_duration(mc.turns_of(cache.hypothesis(bits[t], n)), on, off)
            assert mc.turns_of(cache.hypothesis(bits[t], n, on, off)) == kept
            turns += len(kept)
            want = PIPELINES[kind][2]().components(_reference(f), mc.annotation_of(kept, f["uri"], cache.LABEL))
            for i, c in enumerate(COMPONENTS):
                for name, got in (("core", core), ("host", host)):
                    assert abs(got.per_file[t, n, i] - want[c]) <= bars[t, n], (name, t, n, c, got.per_file[t, n, i], want[c])
    assert turns > 100
    for got in (core, host):
        assert (got.per_file[mc.NOTHING, :, 3] == got.per_file[mc.NOTHING, :, 0]).all()     # nothing left: all missed
        assert (got.per_file[mc.NOTHING, :, 1:3] == 0).all()
        assert len(set(np.round(got.rate, 9))) >= 6                     # the trials differ in what they score


def test_zero_durations_are_the_two_column_result(case):
    _, cache, _, quads, _ = case
    zero = np.concatenate([quads[:, :2], np.zeros((len(quads), 2))], axis=1)
    for backend in ("core", "host"):
        two, four = cache.evaluate(quads[:, :2], backend=backend), cache.evaluate(zero, backend=backend)
        assert (np.abs(two.per_file - four.per_file) <= _bars(cache, two.per_file)[..., None]).all(), backend


def test_core_at_1_7_and_256_lanes(case):
    _, cache, _, quads, _ = case
    full = cache.evaluate(quads, backend="core").per_file
    bars = _bars(cache, full)
    try:
        for lanes in (1, 7):
            cache.SCORE_LANES = lanes                     # (an instance attribute over the class's 256)
            assert (np.abs(cache.evaluate(quads, backend="core").per_file - full) <= bars[..., None]).all(), lanes
    finally:
        del cache.SCORE_LANES
    assert cache.SCORE_LANES == 256


# ---------------------------------------------------------------------------------------------------- 3. refusals
def _small_cache(kind="vad"):
    return {"vad": VadTuneCache, "osd": OsdTuneCache}[kind].from_arrays(mc.files(kind)[:2] + mc.files(kind)[4:],
                                                                       _config(kind))


def _dia_config(**kw):
    return SpeakerDiarizationConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                    embedding=M.EmbeddingModel(lambda: scenarios.ToyEmbedding()), latency=2.5,
                                    device=torch.device("cpu"), **kw)


def test_refusals(tmp_path):
    cache = _small_cache()
    for column, name in ((2, "min_duration_on"), (3, "min_duration_off")):
        for bad in (np.nan, np.inf, -0.01):
            quads = np.array([[0.6, 0.4, 0.1, 0.1], [0.6, 0.4, 0.1, 0.1]])
            quads[1, column] = bad
            for backend in ("host", "core", "gpu"):
                with pytest.raises(ValueError, match=f"{name} of trial 1"):
                    cache.evaluate(quads, backend=backend)
                with pytest.raises(ValueError, match=f"{name} of trial 1"):
                    cache.replay(quads, backend=backend)
    with pytest.raises(ValueError, match="tau_offset"):
        cache.evaluate(np.array([[0.6, np.nan, 0.0, 0.0]]), backend="host")
    for shape in ((2, 3), (2, 5), (0, 4)):
        with pytest.raises(ValueError, match=r"\(T,\) or \(T, 1\).*\(T, 2\).*\(T, 4\)"):
            cache.evaluate(np.zeros(shape), backend="host")
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="min_duration_on"):
            cache.hypothesis(np.zeros(cache.total_rows, dtype=np.uint32), 0, bad, 0.0)
    # the C entry points: status 2 and a message that names the function, before anything else happens
    lib = _lib.load()
    d = cache._desc(lambda name: getattr(cache, name).ctypes.data)
    agg, bits = np.empty(cache.total_rows), np.zeros((1, cache.total_rows), dtype=np.uint32)
    out = np.zeros((1, cache.N, 5))
    p = lambda a: a.ctypes.data

    cells = C.byref(cache._host_cells())

    def host_dur(taus, trials=1, lanes=256, desc=d):
        return lib.dz_tune_vad_host(None if desc is None else C.byref(desc), cells, 4, None if taus is None else p(taus),
                                    trials, p(agg), p(bits), lanes, p(out), 1)

    def track_dur(taus, trials=1, masks=bits):
        return lib.dz_tune_track_score_dur(cells, trials, None if masks is None else p(masks),
                                           None if taus is None else p(taus), p(out), 1)

    def score_dur(taus, trials=1, ctx=None):
        # without a context the call is refused before the device is touched: this runs on a machine without a GPU
        return lib.dz_tune_vad_score(ctx, None, 4, trials, None, None if taus is None else p(taus), None, None, None, None)

    good = np.array([[0.6, 0.4, 0.1, 0.2]])
    assert host_dur(good) == 0 and track_dur(good) == 0
    for call, name in ((host_dur, "dz_tune_vad_host"), (track_dur, "dz_tune_track_score_dur"),
                       (score_dur, "dz_tune_vad_score")):
        for column in (2, 3):
            for bad in (np.nan, np.inf, -np.inf, -1e-300):
                quad = good.copy()
                quad[0, column] = bad
                assert call(quad) == 2, (name, column, bad)
                message = lib.dz_last_error().decode()
                assert name in message and ("min_duration_on", "min_duration_off")[column - 2] in message, message
        assert call(None) == 2 and name in lib.dz_last_error().decode()
        assert call(good, trials=0) == 2 and name in lib.dz_last_error().decode()
        assert call(good, trials=-3) == 2 and name in lib.dz_last_error().decode()
    assert score_dur(good) == 2 and "dz_tune_vad_score: NULL" in lib.dz_last_error().decode()     # (no context)
    assert host_dur(good, desc=None) == 2 and "dz_tune_vad_host:" in lib.dz_last_error().decode()
    assert track_dur(good, masks=None) == 2 and "dz_tune_track_score_dur: NULL" in lib.dz_last_error().decode()
    assert host_dur(good, lanes=257) == 2 and "dz_tune_vad_host:" in lib.dz_last_error().decode()
    assert host_dur(np.array([[0.6, np.nan, 0.0, 0.0]])) == 2 and "tau_offset" in lib.dz_last_error().decode()
    # the configurations, the accumulator, the file batch
    for kind in ("vad", "osd"):
        assert (_config(kind).min_duration_on, _config(kind).min_duration_off) == (0.0, 0.0)
        assert _config(kind, min_duration_on=0.25, min_duration_off=1).min_duration_off == 1.0
        for bad in (-0.1, float("nan"), float("inf"), "long", None, True):
            with pytest.raises(ValueError, match=f"{PIPELINES[kind][1].__name__}: min_duration_on"):
                _config(kind, min_duration_on=bad)
            with pytest.raises(ValueError, match=f"{PIPELINES[kind][1].__name__}: min_duration_off"):
                _config(kind, min_duration_off=bad)
    from diart_amd.pipeline import FileBatch, OverlapBatch, VadBatch
    from diart_amd.serve import StreamServer
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="PredictionAccumulator: min_duration_off"):
            PredictionAccumulator("x", min_duration_off=bad)
        with pytest.raises(ValueError, match="FileBatch: min_duration_on"):
            FileBatch(None, None, pipeline="vad", min_duration_on=bad)
    for name in ("min_duration_on", "min_duration_off"):
        refused = f"{name} is not a parameter of SpeakerDiarization"
        with pytest.raises(ValueError, match=refused):
            FileBatch(None, None, **{name: 0.2})
        with pytest.raises(ValueError, match=refused):
            _dia_config(**{name: 0.2})
        config = _dia_config()
        setattr(config, name, 0.0)
        with pytest.raises(ValueError, match=refused):
            SpeakerDiarization(config)
        with pytest.raises(ValueError, match=refused):
            Optimizer(SpeakerDiarization, None, None, tmp_path / "a", base_config=config)
        dia = TuneCache.from_arrays([tc.file_of(*tc.random_outputs(1, 5, 16, 3, 8))], tc.config_of(0.6, 0.3, 1.0, 4, 2.5))
        with pytest.raises(ValueError, match=refused):
            Optimizer(SpeakerDiarization, None, None, tmp_path / "b", base_config=_dia_config(), cache=dia,
                      hparams=[base.TauActive, base.HyperParameter.from_name(name)])
        # live steps have no look-ahead: the engines and the server take no such argument
        for live in (VadBatch, OverlapBatch):
            with pytest.raises(TypeError, match=name):
                live(None, 4, **{name: 0.2})
        with pytest.raises(TypeError, match=name):
            StreamServer(None, None, pipeline="vad", **{name: 0.2})
    with pytest.raises(ValueError, match="Optimizer: base_config: min_duration_on"):
        config = _config("vad")
        config.min_duration_on = -1.0
        Optimizer(VoiceActivityDetection, None, None, tmp_path / "c", base_config=config, cache=cache)
    assert base.HyperParameter.from_name("min_duration_on") is base.MinDurationOn
    assert base.HyperParameter.from_name("min_duration_off") is base.MinDurationOff
    assert [(h.name, h.low, h.high) for h in (base.MinDurationOn, base.MinDurationOff)] == \
        [("min_duration_on", 0, 1), ("min_duration_off", 0, 1)]
    assert [h.name for h in VoiceActivityDetection.hyper_parameters()] == ["tau_active"]


# ---------------------------------------------------------------------------------------------------- 4. Optimizer
def _optimizer(path, cache, kind="vad", **kw):
    kw.setdefault("base_config", _config(kind))
    return Optimizer(PIPELINES[kind][0], None, None, path / "study", cache=cache, backend="host", **kw)


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_optimizer_tunes_the_durations(tmp_path, kind):
    cache = _small_cache(kind)
    calls = []
    evaluate = cache.evaluate

    def counting(taus, **kw):
        calls.append(np.array(taus))
        return evaluate(taus, **kw)

    cache.evaluate = counting
    # the defaults stay what they were: tau_active alone, (T, 1) trials; with tau_offset, (T, 2)
    plain = _optimizer(tmp_path / "plain", cache, kind, seed=3)
    assert [p.name for p in plain.hparams] == ["tau_active"]
    plain(3, show_progress=False)
    pair = _optimizer(tmp_path / "pair", cache, kind, seed=3, hparams=[base.TauActive, base.TauOffset])
    pair(3, show_progress=False)
    assert [c.shape for c in calls] == [(3, 1), (3, 2)]
    calls.clear()
    four = [base.TauActive, base.MinDurationOn, base.MinDurationOff]
    opt = _optimizer(tmp_path, cache, kind, seed=3, trials_per_batch=8, hparams=four)
    opt(20, show_progress=False)
    assert [c.shape for c in calls] == [(8, 4), (8, 4), (4, 4)] and len(opt.trials) == 20
    assert opt.trials[0]["params"] == {"tau_active": hc.ON, "min_duration_on": 0.0, "min_duration_off": 0.0}   # kick-start
    quads = np.concatenate(calls)
    assert np.array_equal(quads[:, 0], quads[:, 1])                   # no hysteresis: tau_offset == tau_active
    assert np.array_equal(quads[:, [0, 2, 3]], np.array([[t["params"][p.name] for p in four] for t in opt.trials]))
    assert ((quads[1:, 2:] > 0) & (quads[1:, 2:] < 1)).all()
    rates = evaluate(quads, backend="host").rate
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * rates)
    assert opt.best_performance == 100.0 * rates.min() and opt.best_performance <= opt.trials[0]["value"]
    assert set(opt.best_hparams) == {"tau_active", "min_duration_on", "min_duration_off"}
    # the kick-start is what a study without durations gives for the same tau_active, within the bound between texts
    assert abs(opt.trials[0]["value"] - 100.0 * evaluate(np.array([hc.ON]), backend="host").rate[0]) <= 1e-7
    # the study file round-trips and resumes; a study of other hyper-parameters is refused
    stored = json.loads((tmp_path / "study" / "study.json").read_text())
    assert stored["hparams"] == ["tau_active", "min_duration_on", "min_duration_off"] and stored["trials"] == opt.trials
    calls.clear()
    again = _optimizer(tmp_path, cache, kind, seed=3, trials_per_batch=8, hparams=four)
    assert again.trials == opt.trials
    again(5, show_progress=False)
    assert [c.shape for c in calls] == [(5, 4)] and [t["number"] for t in again.trials] == list(range(25))
    assert again.trials[:20] == opt.trials
    with pytest.raises(ValueError, match="holds a study of"):
        _optimizer(tmp_path, cache, kind)
    with pytest.raises(ValueError, match="holds a study of"):
        _optimizer(tmp_path, cache, kind, hparams=[base.TauActive, base.MinDurationOn])
    # a duration that is not tuned is the base configuration's in every trial; one alone carries four columns too
    calls.clear()
    fixed = _optimizer(tmp_path / "fixed", cache, kind, seed=1, base_config=_config(kind, min_duration_off=0.3))
    fixed(4, show_progress=False)
    assert calls[0].shape == (4, 4) and (calls[0][:, 3] == 0.3).all() and (calls[0][:, 2] == 0.0).all()
    assert all(list(t["params"]) == ["tau_active"] for t in fixed.trials)
    calls.clear()
    alone = _optimizer(tmp_path / "alone", cache, kind, seed=1, hparams=[base.MinDurationOn],
                       base_config=_config(kind, tau_offset=hc.OFF))
    alone(3, show_progress=False)
    assert calls[0].shape == (3, 4) and (calls[0][:, :2] == [hc.ON, hc.OFF]).all() and (calls[0][:, 3] == 0).all()
    # grid: the largest cube of at most num_iter points
    grid = _optimizer(tmp_path / "grid", cache, kind, sampler="grid", do_kickstart_hparams=False,
                      hparams=[base.MinDurationOn, base.MinDurationOff])
    grid(9, show_progress=False)
    assert sorted({t["params"]["min_duration_off"] for t in grid.trials}) == pytest.approx([0.25, 0.5, 0.75])


def test_command_line(tmp_path):
    from diart_amd import tune
    _small_cache().save(tmp_path / "vad.npz")
    common = [str(tmp_path), "--reference", str(tmp_path), "--num-iter", "5", "--seed", "2", "--latency", "2.5", "--cpu",
              "--tau-active", "0.6"]
    vad = common + ["--pipeline", "VoiceActivityDetection", "--cache", str(tmp_path / "vad.npz")]
    models = (M.SegmentationModel(lambda: scenarios.ToySegmentation()), None)
    opt = tune.run(tune.parser().parse_args(vad + ["--output", str(tmp_path / "s1"), "--min-duration-on", "0.2",
                                                   "--min-duration-off", "0.1", "--hparams", "tau_active",
                                                   "min_duration_on", "min_duration_off"]), models=models)
    assert [p.name for p in opt.hparams] == ["tau_active", "min_duration_on", "min_duration_off"]
    assert (opt.base_config.min_duration_on, opt.base_config.min_duration_off) == (0.2, 0.1)
    assert opt.trials[0]["params"] == {"tau_active": 0.6, "min_duration_on": 0.2, "min_duration_off": 0.1}
    opt = tune.run(tune.parser().parse_args(vad + ["--output", str(tmp_path / "s2"), "--min-duration-off", "0.3"]), models=models)
    assert all(list(t["params"]) == ["tau_active"] for t in opt.trials) and opt.base_config.min_duration_off == 0.3
    opt = tune.run(tune.parser().parse_args(vad + ["--output", str(tmp_path / "s3")]), models=models)
    assert (opt.base_config.min_duration_on, opt.base_config.min_duration_off) == (0.0, 0.0) and not opt._durations()
    for extra in (["--min-duration-on", "0.4"], ["--hparams", "tau_active", "min_duration_off"]):
        with pytest.raises(SystemExit, match="is not a parameter of SpeakerDiarization"):
            tune.run(tune.parser().parse_args(common + ["--output", str(tmp_path / "s4")] + extra),
                     models=(models[0], M.EmbeddingModel(lambda: scenarios.ToyEmbedding())))


# ---------------------------------------------------------------------------------------------------- 5. files
class _BurstConfig(base.PipelineConfig):
    def __init__(self, min_duration_on=0.0, min_duration_off=0.0):
        self.min_duration_on, self.min_duration_off = min_duration_on, min_duration_off

    duration = property(lambda self: 5.0)
    step = property(lambda self: 0.5)
    latency = property(lambda self: 0.5)
    sample_rate = property(lambda self: 16000)


class _BurstVAD(base.Pipeline):
    """Speech = the newest `step` seconds of the window have RMS > 0.05: one turn per chunk, on the CPU."""

    def __init__(self, config=None):
        self._config = _BurstConfig() if config is None else config
        self.shift = 0.0

    get_config_class = staticmethod(lambda: _BurstConfig)
    suggest_metric = staticmethod(lambda: DetectionErrorRate())
    hyper_parameters = staticmethod(lambda: [])
    config = property(lambda self: self._config)

    def reset(self):
        self.shift = 0.0

    def set_timestamp_shift(self, shift):
        self.shift = shift

    def __call__(self, waveforms):
        out = []
        for w in waveforms:
            ann = Annotation("x", "speech")
            if float(np.sqrt(np.mean(np.square(w.data[-8000:])))) > 0.05:
                ann[Segment(w.extent.end - 0.5 + self.shift, w.extent.end + self.shift), 0] = "speech"
            out.append((ann, w))
        return out


def _bursts(seconds, on, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(int(seconds * 16000), dtype=np.float32)
    for a, b in on:
        x[int(a * 16000):int(b * 16000)] = 0.3 * rng.standard_normal(int(b * 16000) - int(a * 16000)).astype(np.float32)
    return x


def test_accumulator_and_benchmark_loop(tmp_path):
    """PredictionAccumulator and Benchmark's one-file-at-a-time loop on a CPU pipeline: the RTTM is the yardstick rule
    on the zero-duration run's turns; the per-step outputs do not change."""
    speech = tmp_path / "wav"
    speech.mkdir()
    # turns of 0.5 .. 4 s and gaps of 0.5 .. 2 s, on the 0.5 s grid of the stub
    write_wav(speech / "a.wav", _bursts(24.0, [(6.0, 6.5), (7.0, 9.0), (10.5, 11.0), (13.0, 17.0), (17.5, 18.0), (20.0, 21.0)], 1), 16000)
    write_wav(speech / "b.wav", _bursts(15.0, [(5.5, 6.5), (8.5, 9.0), (9.5, 10.0), (12.0, 14.5)], 2), 16000)

    def run(tag, **kw):
        preds = Benchmark(speech, None, tmp_path / tag, show_report=False, batch_size=4)(_BurstVAD, _BurstConfig(**kw))
        return preds, {p.name: p.read_text() for p in sorted((tmp_path / tag).iterdir())}

    zero, zero_text = run("zero")
    assert sum(len(p) for p in zero) >= 9
    for on, off in ((0.75, 0.0), (0.0, 0.75), (0.75, 0.75), (1.0, 1.6), (0.5, 0.5), (100.0, 0.0)):
        got, text = run(f"run_{on}_{off}", min_duration_on=on, min_duration_off=off)
        changed = 0
        for before, after in zip(zero, got):
            want = mc.annotation_of(mc.min_duration(mc.turns_of(before), on, off), before.uri, "speech")
            assert after.to_rttm() == want.to_rttm() and text[f"{before.uri}.rttm"] == want.to_rttm()
            changed += after.to_rttm() != before.to_rttm()
        assert changed == (0 if (on, off) == (0.5, 0.5) else 2), (on, off)        # (0.5 s turns and gaps stay: strict <)
    # the accumulator itself: the accumulated turns stay, so that a later step can still bridge a gap
    acc, plain = PredictionAccumulator("u", min_duration_on=0.75, min_duration_off=0.75), PredictionAccumulator("u")
    for s, e in ((0.0, 0.5), (1.0, 1.5)):
        for a in (acc, plain):
            a.on_next(mc.annotation_of([(s, e)], "u", "speech"))
    assert mc.turns_of(acc.get_prediction()) == [(0.0, 1.5)] and mc.turns_of(plain.get_prediction()) == [(0.0, 0.5), (1.0, 1.5)]
    acc.on_next(mc.annotation_of([(5.0, 5.5)], "u", "speech"))
    assert mc.turns_of(acc.get_prediction()) == [(0.0, 1.5)]               # the new 0.5 s turn is dropped for now ...
    acc.on_next(mc.annotation_of([(6.0, 6.5)], "u", "speech"))
    assert mc.turns_of(acc.get_prediction()) == [(0.0, 1.5), (5.0, 6.5)]   # ... and kept once a later one joins it
    assert PredictionAccumulator("u", min_duration_on=1.0).get_prediction() is None


# ---------------------------------------------------------------------------------------------------- 6. sanitizers
def test_host_texts_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/native/min_duration_sanitize.cpp, a program of its own, compiled with g++ -fsanitize=address,undefined
    together with the host sources: dz_tune_vad_host (four columns) and dz_tune_track_score_dur on a generated cache.  No Python
    runs under the sanitizer."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    src = [ROOT / "tests" / "native" / "min_duration_sanitize.cpp"] + \
        [ROOT / "diart_amd" / "csrc" / f for f in ("cluster.cpp", "tail.cpp", "hostpool.cpp", "filebatch.cpp", "tune_score.cpp")]
    exe = tmp_path / "min_duration_sanitize"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *map(str, src), "-o", str(exe), "-lpthread"],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("sanitizer runtime not installed: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr[-2000:]
    import os
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    if "unexpected memory mapping" in run.stderr or "ReExec" in run.stderr:
        pytest.skip("the sanitizer runtime cannot map its shadow memory on this kernel: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0 and "min_duration_sanitize ok" in run.stdout, (run.stdout[-500:] + run.stderr[-3000:])
    assert "ERROR: " not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
