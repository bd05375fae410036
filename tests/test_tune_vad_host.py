"""Tuning VoiceActivityDetection without a GPU (diart_amd/optim.py VadTuneCache, csrc/tune_core.h, csrc/tune_score.cpp):
the host backend against the existing Python path (VoiceActivityDetection.finalise -> PredictionAccumulator ->
metrics.DetectionErrorRate), the scoring kernel's text run on the host against dz_tune_score, the cache file, the
refusals, the Optimizer's bookkeeping and the command line.  Synthetic inputs and the toy models of
tests/golden/scenarios.py only."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_vad_cases as vc  # noqa: E402
from tune_cases import scenarios  # noqa: E402

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.blocks.vad import VoiceActivityDetection, VoiceActivityDetectionConfig  # noqa: E402
from diart_amd.features import Annotation, Segment, SlidingWindow, SlidingWindowFeature  # noqa: E402
from diart_amd.inference import PredictionAccumulator  # noqa: E402
from diart_amd.metrics import COMPONENTS, DetectionErrorRate, DiarizationErrorRate  # noqa: E402
from diart_amd.optim import Optimizer, TuneCache, VadTuneCache, trial_config  # noqa: E402

F = 32
SR = 16                      # the chunks only carry their time axis: 80 samples of 5 s
BATCH = 7                    # finalise computes the frame resolution from the first chunk of every batch


def _config(latency, tau=0.6):
    return VoiceActivityDetectionConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                        latency=latency, tau_active=tau, device=torch.device("cpu"))


def _dia_config(latency=2.5):
    return SpeakerDiarizationConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                    embedding=M.EmbeddingModel(lambda: scenarios.ToyEmbedding()), latency=latency,
                                    device=torch.device("cpu"))


def _chunks(starts):
    return [SlidingWindowFeature(np.zeros((int(tc.DURATION * SR), 1), dtype=np.float32),
                                 SlidingWindow(start=float(s), duration=1.0 / SR, step=1.0 / SR)) for s in starts]


def _files(shifts=(0.0, -1.75, 0.0)):
    """60 and 23 chunks with a three-speaker reference, and 9 chunks whose reference is empty (total = 0)."""
    files = []
    for n, (count, shift) in enumerate(zip((60, 23, 9), shifts)):
        f = vc.file_of(vc.track_of(40 + n, count, F), shift=shift, uri=f"file{n}", reference=[] if n == 2 else None)
        chunks, res = _chunks(f["starts"]), []
        for i in range(0, count, BATCH):
            res += [chunks[i].extent.duration / F] * len(chunks[i:i + BATCH])
        f["res"] = np.array(res)
        files.append(f)
    return files


def _python_path(f, config):
    """The existing path: VoiceActivityDetection.finalise on the cached tracks, batch by batch, then
    PredictionAccumulator."""
    vad = VoiceActivityDetection(config)
    vad.set_timestamp_shift(f["shift"])
    acc = PredictionAccumulator(f["uri"])
    chunks = _chunks(f["starts"])
    for i in range(0, len(chunks), BATCH):
        for out in vad.finalise(chunks[i:i + BATCH], torch.from_numpy(f["track"][i:i + BATCH, :, None])):
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


@pytest.mark.parametrize("latency", [0.5, 2.5, 5.0])
def test_host_backend_is_the_python_path(latency):
    """Per file and tau the host backend's hypothesis has the turns of VoiceActivityDetection.finalise +
    PredictionAccumulator on the cached tracks, and its components are metrics.DetectionErrorRate's on that
    prediction within 1e-9 x total (the two differ in the order in which a file's durations are summed).  Trials: the
    base value, a tau equal to an aggregated score that occurs (`>` meets it exactly), 0.35 and 0.85; shifts 0 and
    -1.75; a file with an empty reference."""
    files = _files()
    cache = VadTuneCache.from_arrays(files, _config(latency))
    agg = cache.replay(np.array([0.6]), backend="host")[0]
    first = agg[:int(cache.file_row_off[1])]
    tau_tie = float(np.sort(first[(first > 0.5) & (first < 0.8)])[3])
    taus = np.array([0.6, tau_tie, 0.35, 0.85])
    agg, bits = cache.replay(taus, backend="host")
    assert agg.shape == (cache.total_rows,) and bits.shape == (4, cache.total_rows) and bits.dtype == np.uint32
    assert (agg == tau_tie).any() and not np.array_equal(bits[1], (agg >= tau_tie).astype(np.uint32))
    result = cache.evaluate(taus[:, None], backend="host")                    # (T, 1) as well as (T,)
    assert np.array_equal(result.per_file, cache.score(bits)) and (result.status == -1).all()
    assert result.status.shape == (4, 3) and result.per_file.shape == (4, 3, 5) and (result.per_file[..., 4] == 0).all()
    bars = _bars(cache, result.per_file)
    turns = 0
    for t, tau in enumerate(taus):
        metric = DetectionErrorRate()
        for n, f in enumerate(files):
            want = _python_path(f, _config(latency, tau))
            got = cache.hypothesis(bits[t], n)
            assert _table(got) == _table(want), (t, n)
            assert {label for _, _, label in _table(got)} <= {"speech"}
            turns += len(_table(want))
            comp = metric.components(_reference(f), want)
            assert (comp["total"] == 0) == (n == 2)
            for i, c in enumerate(COMPONENTS):
                assert abs(result.per_file[t, n, i] - comp[c]) <= bars[t, n], (t, n, c, result.per_file[t, n, i], comp[c])
            metric(_reference(f), want)
        assert abs(result.rate[t] - abs(metric)) <= 3e-9, (t, result.rate[t], abs(metric))
    assert turns > 20
    only = VadTuneCache.from_arrays(files[2:], _config(latency)).evaluate(taus, backend="host")
    # _Accumulating._rate without a total: 1 where there is an error, 0 where there is none
    assert (only.components[:, 0] == 0).all() and np.array_equal(only.rate, (only.components[:, 2] > 0).astype(float))
    assert only.rate[0] == 1.0


@pytest.mark.parametrize("name", list(vc.EDGES) + ["collar", "carry", "degenerate", "files"])
def test_kernel_text_on_the_host_is_the_host_backend(name):
    """What tune_vad_score_kernel computes (csrc/tune_core.h, its 256 lanes played in order on the host) against
    dz_tune_score on the masks, on the caches of tests/test_gpu_tune_vad.py: the five components within 1e-9 x
    total."""
    if name in vc.EDGES:
        cache, taus = vc.edge_cache(name)
    elif name == "files":
        cache, taus = VadTuneCache.from_arrays(_files(), _config(2.5)), vc.taus_of(17, 3)
    else:
        cache = getattr(vc, f"{name}_cache")()
        cache = cache[0] if isinstance(cache, tuple) else cache
        taus = np.concatenate([vc.taus_of(33, 11), [0.5]])
    host, core = cache.evaluate(taus, backend="host"), cache.evaluate(taus, backend="core")
    assert cache.sorted_steps
    assert (np.abs(host.per_file - core.per_file) <= _bars(cache, host.per_file)[..., None]).all()
    assert np.array_equal(np.isnan(host.rate), np.isnan(core.rate)) and np.abs(host.rate - core.rate).max() <= 3e-9


def test_collar_case_is_what_it_says():
    """The hand-made track gives the rows it was made for, and each inactive run is patched or kept by its length."""
    cache, on = vc.collar_cache()
    bits = cache.replay(np.array([0.5]), backend="host")[1]
    assert np.array_equal(bits[0].astype(bool), on)
    kept = 0
    step_of = np.repeat(np.arange(len(cache.step_rows)), cache.step_rows)
    for start, frames in vc.collar_runs(cache):
        c = int(step_of[start])
        close = cache.mids[start + c - 1] if start == cache.row_off[c] else cache.mids[start + c]
        gap = cache.mids[start + frames + int(step_of[start + frames])] - close
        patched = gap <= 1e-6 or gap < 0.05
        assert patched == (frames <= 2) or frames == 3, (start, frames, gap)
        assert min(abs(gap - frames / 60.0), abs(gap - frames * 5.0 / 293)) < 1e-9      # (the first step's rows: 5 / 293 s)
        kept += not patched
    assert kept >= 3 and len(_table(cache.hypothesis(bits[0], 0))) == 1 + kept
    # steps whose grids are not sorted by time: the scoring kernel's text refuses, the host backend sorts
    f = vc.file_of(vc.track_of(1, 6, 16))
    f["starts"] = f["starts"][::-1].copy()
    backwards = vc.cache_of([f], 0.5)
    assert not backwards.sorted_steps
    with pytest.raises(ValueError, match="not sorted by time"):
        backwards.evaluate(np.array([0.5]), backend="core")
    backwards.evaluate(np.array([0.5]), backend="host")


def test_cache_round_trip_and_refusals(tmp_path):
    files = _files()
    cache = VadTuneCache.from_arrays(files, _config(2.5))
    cache.save(tmp_path / "vad.npz")
    again = VadTuneCache.load(tmp_path / "vad.npz")
    taus = vc.taus_of(5)
    a, b = cache.evaluate(taus, backend="host"), again.evaluate(taus, backend="host")
    assert np.array_equal(a.per_file, b.per_file) and np.array_equal(a.rate, b.rate)
    assert a.rate.shape == (5,) and a.components.shape == (5, 5) and a.per_file.shape == (5, 3, 5) and a.status.shape == (5, 3)
    c = cache.evaluate(taus, backend="host", memory_budget=2 * cache.bytes_per_trial)      # two trials per batch
    assert np.array_equal(a.per_file, c.per_file)
    assert again.meta == cache.meta and [f["turns"] for f in again.files] == [f["turns"] for f in cache.files]
    # (C, F, 1), what model_outputs returns, is the same cache
    wide = [dict(f, track=f["track"][:, :, None]) for f in files]
    assert np.array_equal(VadTuneCache.from_arrays(wide, _config(2.5)).evaluate(taus, backend="host").per_file, a.per_file)
    # a cache file of the other kind is refused by name, both ways
    seg, emb = tc.random_outputs(1, 5, 16, 3, 8)
    TuneCache.from_arrays([tc.file_of(seg, emb)], tc.config_of(0.6, 0.3, 1.0, 4, 2.5)).save(tmp_path / "dia.npz")
    with pytest.raises(ValueError, match="holds a TuneCache.*not a VadTuneCache"):
        VadTuneCache.load(tmp_path / "dia.npz")
    with pytest.raises(ValueError, match="holds a VadTuneCache"):
        TuneCache.load(tmp_path / "vad.npz")
    TuneCache.load(tmp_path / "dia.npz")
    # the pipelines and their caches
    with pytest.raises(ValueError, match="VoiceActivityDetection.*VadTuneCache"):
        TuneCache.collect(VoiceActivityDetection, _config(2.5), tmp_path, tmp_path)
    with pytest.raises(ValueError, match="SpeakerDiarization"):
        VadTuneCache.collect(SpeakerDiarization, _dia_config(), tmp_path, tmp_path)
    with pytest.raises(ValueError, match=r"taus \(T,\) or \(T, 1\)"):
        cache.evaluate(np.zeros((2, 3)), backend="host")
    with pytest.raises(ValueError, match="backend 'core'"):
        cache.replay(taus, backend="core")
    with pytest.raises(ValueError, match="share the frames"):
        VadTuneCache.from_arrays([files[0], vc.file_of(vc.track_of(1, 3, 16))], _config(2.5))


def test_model_outputs_is_the_model_half():
    """VoiceActivityDetection.model_outputs is what finalise computes as voice_detection: __call__ on a batch equals
    finalise on its chunks and scores, and a cache collected through it replays to the pipeline's own prediction."""
    config = _config(2.5)
    chunks = [SlidingWindowFeature(np.random.default_rng(i).standard_normal((80000, 1)).astype(np.float32),
                                   SlidingWindow(start=0.5 * i, duration=1.0 / 16000, step=1.0 / 16000)) for i in range(4)]
    vad = VoiceActivityDetection(config)
    track = vad.model_outputs(chunks)
    seg = vad.segmentation(torch.from_numpy(np.stack([c.data for c in chunks])))
    assert track.dtype == torch.float32 and track.device.type == "cpu" and track.shape == (4, seg.shape[1], 1)
    assert torch.equal(track, torch.max(seg, dim=-1, keepdim=True)[0])
    want = [a for a, _ in VoiceActivityDetection(config)(chunks)]
    got = [a for a, _ in VoiceActivityDetection(config).finalise(chunks, track)]
    assert [_table(a) for a in got] == [_table(a) for a in want]


def _optimizer(tmp_path, cache, **kw):
    kw.setdefault("base_config", _config(2.5))
    return Optimizer(VoiceActivityDetection, None, None, tmp_path / "study", cache=cache, backend="host", **kw)


def test_optimizer_bookkeeping(tmp_path):
    cache = VadTuneCache.from_arrays(_files(), _config(2.5))
    calls = []
    evaluate = cache.evaluate

    def counting(taus, **kw):
        calls.append(np.array(taus))
        return evaluate(taus, **kw)

    cache.evaluate = counting
    opt = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4)
    assert [p.name for p in opt.hparams] == ["tau_active"]
    opt(10, show_progress=False)
    assert [c.shape for c in calls] == [(4, 1), (4, 1), (2, 1)] and len(opt.trials) == 10
    assert opt.trials[0]["params"] == {"tau_active": 0.6}                       # kick-start: the base configuration
    assert all(list(t["params"]) == ["tau_active"] and 0 <= t["params"]["tau_active"] <= 1 for t in opt.trials)
    taus = np.concatenate(calls)
    rates = evaluate(taus, backend="host").rate
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * rates)
    best = int(np.argmin(rates))
    assert opt.best_performance == 100.0 * rates[best] and opt.best_hparams == opt.trials[best]["params"]
    assert json.loads((tmp_path / "study" / "study.json").read_text())["trials"] == opt.trials
    # resume: the stored trials are loaded, the numbering continues, nothing stored is evaluated again
    calls.clear()
    again = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4)
    assert again.trials == opt.trials
    again(3, show_progress=False)
    assert [len(c) for c in calls] == [3] and [t["number"] for t in again.trials] == list(range(13))
    fresh = _optimizer(tmp_path / "other", cache, seed=3)
    fresh(13, show_progress=False)
    assert [t["params"] for t in fresh.trials] == [t["params"] for t in again.trials]
    # grid: num_iter equally spaced interior values of the one axis
    grid = _optimizer(tmp_path / "grid", cache, sampler="grid", do_kickstart_hparams=False)
    grid(4, show_progress=False)
    assert [t["params"]["tau_active"] for t in grid.trials] == pytest.approx([0.2, 0.4, 0.6, 0.8], abs=1e-12)
    grid(4, show_progress=False)
    assert len(grid.trials) == 4
    cfg = trial_config(_config(2.5), grid.trials[0]["params"])
    assert cfg.tau_active == grid.trials[0]["params"]["tau_active"] and cfg.latency == 2.5
    # a metric of its kind is accepted; without a base configuration there is no kick-start
    _optimizer(tmp_path / "metric", cache, metric=DetectionErrorRate())


def test_optimizer_refusals(tmp_path):
    cache = VadTuneCache.from_arrays(_files(), _config(2.5))
    dia = TuneCache.from_arrays([tc.file_of(*tc.random_outputs(1, 5, 16, 3, 8))], tc.config_of(0.6, 0.3, 1.0, 4, 2.5))
    with pytest.raises(ValueError, match="VoiceActivityDetection: cache must be a VadTuneCache"):
        Optimizer(VoiceActivityDetection, None, None, tmp_path / "study", base_config=_config(2.5), cache=dia)
    with pytest.raises(ValueError, match="SpeakerDiarization: cache must be a TuneCache"):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "study", base_config=_dia_config(), cache=cache)
    with pytest.raises(ValueError, match="rho_update changes the model outputs: only tau_active"):
        _optimizer(tmp_path, cache, hparams=[base.TauActive, base.RhoUpdate])
    with pytest.raises(ValueError, match="DiarizationErrorRate.*VoiceActivityDetection"):
        _optimizer(tmp_path, cache, metric=DiarizationErrorRate())
    with pytest.raises(ValueError, match="DetectionErrorRate"):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "study", base_config=_dia_config(),
                  metric=DetectionErrorRate())

    class Custom(VoiceActivityDetection):
        pass

    with pytest.raises(ValueError, match="Custom"):
        Optimizer(Custom, None, None, tmp_path / "study", base_config=_config(2.5), cache=cache)


def test_exports_and_command_line(tmp_path):
    import diart_amd
    assert diart_amd.VadTuneCache is VadTuneCache and diart_amd.TuneCache is TuneCache
    from diart_amd import tune
    VadTuneCache.from_arrays(_files(), _config(2.5)).save(tmp_path / "vad.npz")
    seg, emb = tc.random_outputs(1, 5, 16, 3, 8)
    TuneCache.from_arrays([tc.file_of(seg, emb)], tc.config_of(0.6, 0.3, 1.0, 4, 2.5)).save(tmp_path / "dia.npz")
    common = [str(tmp_path), "--reference", str(tmp_path), "--num-iter", "6", "--seed", "2", "--trials-per-batch", "4",
              "--latency", "2.5", "--cpu", "--pipeline", "VoiceActivityDetection"]
    models = (M.SegmentationModel(lambda: scenarios.ToySegmentation()), None)
    # --embedding and the clustering arguments are ignored, --hparams defaults to tau_active
    args = tune.parser().parse_args(common + ["--output", str(tmp_path / "study"), "--cache", str(tmp_path / "vad.npz"),
                                              "--embedding", "no-such-file", "--delta-new", "0.2", "--max-speakers", "99"])
    opt = tune.run(args, models=models)
    assert opt.pipeline_class is VoiceActivityDetection and isinstance(opt.cache, VadTuneCache)
    assert len(opt.trials) == 6 and all(list(t["params"]) == ["tau_active"] for t in opt.trials)
    assert (tmp_path / "study" / "study.json").exists()
    with pytest.raises(ValueError, match="holds a TuneCache.*not a VadTuneCache"):
        tune.run(tune.parser().parse_args(common + ["--output", str(tmp_path / "s2"), "--cache", str(tmp_path / "dia.npz")]),
                 models=models)
    with pytest.raises(SystemExit, match="tau_active"):
        tune.run(tune.parser().parse_args(common + ["--output", str(tmp_path / "s3"), "--hparams", "delta_new"]),
                 models=models)
    assert tune.parser().parse_args(common[:3] + ["--output", "x"]).pipeline == "SpeakerDiarization"
