"""Tuning OverlappedSpeechDetection without a GPU (diart_amd/optim.py OsdTuneCache): its plans and scoring cells against
VadTuneCache given the overlap regions as its reference, the host backend and the scoring kernel's text against the
existing Python path (OsdTuneCache.hypothesis -> metrics.OverlapDetectionErrorRate on the speaker reference), the cache
file, one diarization cache feeding both detection tuners, the Optimizer (error rate and F-measure), the refusals and
the command line.  Synthetic inputs (tests/tune_osd_cases.py) only."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_osd_cases as oc  # noqa: E402
import tune_vad_cases as vc  # noqa: E402
from tune_cases import scenarios  # noqa: E402

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.blocks.osd import OverlappedSpeechDetection, OverlappedSpeechDetectionConfig  # noqa: E402
from diart_amd.blocks.vad import VoiceActivityDetection, VoiceActivityDetectionConfig  # noqa: E402
from diart_amd.features import Annotation, Segment  # noqa: E402
from diart_amd.metrics import (COMPONENTS, DetectionErrorRate, DiarizationErrorRate, OverlapDetectionErrorRate,  # noqa: E402
                               OverlapDetectionFMeasure, detection_prf, overlap_reference)
from diart_amd.optim import Optimizer, OsdTuneCache, TuneCache, VadTuneCache, _pipeline_kind  # noqa: E402

PLAN_ARRAYS = ("plan", "t0", "out_res", "step_rows", "row_off", "row_chunk", "file_row_off", "chunk_off", "hamming", "mids",
               "starts", "res")
CELL_ARRAYS = ("mid_cell", "cell_dur", "cell_ref", "file_cell_off", "dur_prefix", "ref_prefix", "seg")


def _annotation(turns, uri="file"):
    ann = Annotation(uri=uri)
    for n, (s, e, label) in enumerate(turns):
        ann[Segment(s, e), n] = label
    return ann


def _bars(cache, per_file):
    """1e-9 x total per file; where a file's total is 0, 1e-9 x the sum of its cells' durations."""
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


def _same_arrays(a, b, names):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


@pytest.mark.parametrize("name", list(oc.CRAFTED))
def test_cells_are_the_vad_caches_on_the_overlap_regions(name):
    """The existing class is the yardstick: every plan and cell array of an OsdTuneCache equals, bit for bit, that of a
    VadTuneCache given the same track and overlap_reference(reference)'s turns as its reference — for the reference as
    tuples and as an Annotation, beside a second file with the three-speaker reference."""
    turns = oc.CRAFTED[name]
    regions = overlap_reference(_annotation(turns))
    assert [(seg.start, seg.end) for seg, _ in regions.itertracks()] == oc.CRAFTED_REGIONS[name]
    track, other = oc.track_of(11, 20, 16), oc.track_of(12, 9, 16)
    other_ref = tc.reference_for(9, -0.75)
    for reference in (turns, _annotation(turns)):
        osd = oc.cache_of([oc.file_of(track, uri="crafted", reference=reference),
                           oc.file_of(other, shift=-0.75, uri="other")], 2.5)
        vad = vc.cache_of([vc.file_of(track, uri="crafted", reference=regions),
                           vc.file_of(other, shift=-0.75, uri="other", reference=overlap_reference(_annotation(other_ref)))], 2.5)
        _same_arrays(osd, vad, PLAN_ARRAYS + CELL_ARRAYS)
        assert osd.max_cells == vad.max_cells and osd.sorted_steps == vad.sorted_steps and osd.nwin == vad.nwin
        assert osd.ref_labels[0] == (["overlap"] if oc.CRAFTED_REGIONS[name] else []) and osd.ref_labels[1] == ["overlap"]
        total = osd.evaluate(np.array([0.5]), backend="host").per_file[0, 0, 0]
        want = sum(e - s for s, e in oc.CRAFTED_REGIONS[name])
        assert abs(total - want) <= 1e-9 * max(want, 1.0)
        # the speaker turns are kept as given
        assert osd.files[0]["stored"] == [(s, e, l) for s, e, l in turns]


_PYTHON = {}


def _python_components(key, cache, files, taus):
    """(T, N, 5): OverlapDetectionErrorRate().components(speaker reference, cache.hypothesis(masks of the host backend)),
    computed once per case and shared by the backends."""
    if key not in _PYTHON:
        bits = cache.replay(taus, backend="host")[1]
        out = np.zeros((taus.shape[0], cache.N, 5))
        refs = [_annotation(f["reference"], f["uri"]) for f in files]
        metric = OverlapDetectionErrorRate()
        for t in range(taus.shape[0]):
            for n in range(cache.N):
                hyp = cache.hypothesis(bits[t], n)
                assert set(hyp.labels()) <= {"overlap"}
                comp = metric.components(refs[n], hyp)
                out[t, n] = [comp[c] for c in COMPONENTS]
        _PYTHON[key] = out
    return _PYTHON[key]


def _case(name):
    """(cache, files as given, taus, the file that has to see both kinds of error or None)"""
    if name in oc.EDGES:
        files, latency, taus = oc.edge_files(name)
        return oc.cache_of(files, latency), files, taus, 1
    cache = getattr(oc, f"{name}_cache")()
    files = [dict(uri=f["uri"], reference=f["stored"]) for f in cache.files]
    return cache, files, oc.taus_of(*oc.CARRY_TAUS) if name == "carry" else oc.taus_of(33, 9), 0 if name == "carry" else None


@pytest.mark.parametrize("backend", ["host", "core"])
@pytest.mark.parametrize("name", list(oc.EDGES) + ["carry", "degenerate"])
def test_rates_are_the_python_paths(name, backend):
    """Per trial and file the five components are within 1e-9 x total (a file without overlap: 1e-9 x the sum of its
    cells' durations) of OverlapDetectionErrorRate().components(reference, cache.hypothesis(bits_row, n)), the reference
    being the SPEAKER annotation.  On the long file at least half of the trials have false alarm and missed detection,
    and its overlap total is positive."""
    cache, files, taus, busy = _case(name)
    want = _python_components(name, cache, files, taus)
    got = cache.evaluate(taus, backend=backend)
    assert got.per_file.shape == want.shape and (got.status == -1).all() and (got.per_file[..., 4] == 0).all()
    if busy is not None:
        both = float(((want[:, busy, 2] > 0) & (want[:, busy, 3] > 0)).mean())
        assert both >= 0.5 and (want[:, busy, 0] > 0).all(), (name, both, want[0, busy, 0])
    err, bars = np.abs(got.per_file - want), _bars(cache, want)[..., None]
    worst = np.unravel_index(np.argmax(err - bars), err.shape)
    assert (err <= bars).all(), (name, backend, worst, got.per_file[worst], want[worst])
    if name == "carry":
        assert cache.nwin == 10 and int(cache.chunk_off[1]) == 300 and not cache.files[0]["track"][40:251].any()
    if name == "degenerate":
        positive = taus > 0
        assert (got.per_file[positive, 0, 3] == got.per_file[positive, 0, 0]).all() and (got.per_file[:, 0, 0] > 0).all()
        assert (got.per_file[:, 1, 0] == 0).all() and (got.per_file[:-1, 1, 2] > 0).any()      # speech, but no overlap
        assert np.isnan(cache.replay(taus, backend="host")[0]).any()
        # _Accumulating._rate without a total: 1 where there is an error, 0 where there is none
        alone = OsdTuneCache.from_arrays([dict(cache.files[1], reference=oc.NO_OVERLAP)], oc.config_of(2.5))
        rate = alone.evaluate(taus, backend=backend).rate
        assert set(rate.tolist()) == {0.0, 1.0}


def _files():
    return [oc.file_of(oc.track_of(40, 60, 32), uri="file0"), oc.file_of(oc.track_of(41, 23, 32), shift=-1.75, uri="file1"),
            oc.file_of(oc.track_of(42, 9, 32), uri="file2", reference=oc.NO_OVERLAP)]


def _dia_cache(K=3, chunks=(5, 12)):
    files = []
    for n, c in enumerate(chunks):
        seg, emb = tc.random_outputs(1 + n, c, 16, K, 8)
        if n == 1:
            seg[3] = np.nan
            seg[5, 2, 0] = np.nan
        files.append(tc.file_of(seg, emb, shift=-0.5 * n, uri=f"dia{n}"))
    return TuneCache.from_arrays(files, tc.config_of(0.6, 0.3, 1.0, 4, 2.5))


def test_cache_round_trip_and_the_three_kinds_of_file(tmp_path):
    cache = OsdTuneCache.from_arrays(_files(), oc.config_of(2.5, 0.5))
    cache.save(tmp_path / "osd.npz")
    again = OsdTuneCache.load(tmp_path / "osd.npz")
    _same_arrays(cache, again, PLAN_ARRAYS + CELL_ARRAYS)
    assert again.meta == cache.meta == dict(step=0.5, latency=2.5, tau_active=0.5)
    assert [f["stored"] for f in again.files] == [f["stored"] for f in cache.files]
    assert [f["turns"] for f in again.files] == [f["turns"] for f in cache.files]
    assert {l for f in cache.files for _, _, l in f["stored"]} == {"ref0", "ref1", "ref2", "a", "b"}     # the speakers
    with np.load(tmp_path / "osd.npz") as z:
        assert str(z["kind"]) == "OsdTuneCache" and set(z["ref_labels_0"].tolist()) == {"ref0", "ref1", "ref2"}
    taus = oc.taus_of(5)
    a, b = cache.evaluate(taus, backend="host"), again.evaluate(taus, backend="host")
    assert np.array_equal(a.per_file, b.per_file) and np.array_equal(a.rate, b.rate)
    c = cache.evaluate(taus, backend="host", memory_budget=2 * cache.bytes_per_trial)      # two trials per batch
    assert np.array_equal(a.per_file, c.per_file) and cache.bytes_per_trial == 4 * cache.total_rows
    assert np.array_equal(cache.score(cache.replay(taus, backend="host")[1]), a.per_file)
    # each kind of file is refused by the two other loaders
    VadTuneCache.from_arrays([vc.file_of(vc.track_of(1, 5, 16))], vc.config_of(2.5)).save(tmp_path / "vad.npz")
    _dia_cache().save(tmp_path / "dia.npz")
    with pytest.raises(ValueError, match="holds a VadTuneCache, not an OsdTuneCache"):
        OsdTuneCache.load(tmp_path / "vad.npz")
    with pytest.raises(ValueError, match=r"holds a TuneCache \(SpeakerDiarization\), not an OsdTuneCache"):
        OsdTuneCache.load(tmp_path / "dia.npz")
    with pytest.raises(ValueError, match="not a VadTuneCache"):
        VadTuneCache.load(tmp_path / "osd.npz")
    with pytest.raises(ValueError, match="holds a OsdTuneCache"):
        TuneCache.load(tmp_path / "osd.npz")
    with pytest.raises(ValueError, match="not a VadTuneCache"):
        VadTuneCache.load(tmp_path / "dia.npz")
    with pytest.raises(ValueError, match="holds a VadTuneCache"):
        TuneCache.load(tmp_path / "vad.npz")
    # the pipelines and their caches
    seg = M.SegmentationModel(lambda: scenarios.ToySegmentation())
    vad_config = VoiceActivityDetectionConfig(segmentation=seg, latency=2.5, device=torch.device("cpu"))
    osd_config = OverlappedSpeechDetectionConfig(segmentation=seg, latency=2.5, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="VoiceActivityDetection: OsdTuneCache collects OverlappedSpeechDetection"):
        OsdTuneCache.collect(VoiceActivityDetection, vad_config, tmp_path, tmp_path)
    with pytest.raises(ValueError, match="OverlappedSpeechDetection: VadTuneCache collects VoiceActivityDetection"):
        VadTuneCache.collect(OverlappedSpeechDetection, osd_config, tmp_path, tmp_path)
    with pytest.raises(ValueError, match="OverlappedSpeechDetection.*OsdTuneCache is the cache"):
        TuneCache.collect(OverlappedSpeechDetection, osd_config, tmp_path, tmp_path)

    class Custom(OverlappedSpeechDetection):
        pass

    with pytest.raises(ValueError, match="Custom"):
        OsdTuneCache.collect(Custom, osd_config, tmp_path, tmp_path)
    with pytest.raises(ValueError, match="OsdTuneCache needs at least one file"):
        OsdTuneCache.from_arrays([], oc.config_of(2.5))
    with pytest.raises(ValueError, match=r"taus \(T,\) or \(T, 1\)"):
        cache.evaluate(np.zeros((2, 3)), backend="host")


def test_one_diarization_cache_feeds_both_detection_tuners():
    """from_tune_cache equals the torch statement on the cache's own scores (NaN equal to NaN), takes the starts, the
    resolutions, the shifts and the references over, and replays like a cache made from those arrays."""
    dia = _dia_cache()
    osd, vad = OsdTuneCache.from_tune_cache(dia), VadTuneCache.from_tune_cache(dia)
    assert osd.meta == dict(step=0.5, latency=2.5, tau_active=0.5) and vad.meta == dict(step=0.5, latency=2.5, tau_active=0.6)
    assert OsdTuneCache.from_tune_cache(dia, tau_active=0.3).meta["tau_active"] == 0.3
    assert VadTuneCache.from_tune_cache(dia, tau_active=0.3).meta["tau_active"] == 0.3
    for f, o, v in zip(dia.files, osd.files, vad.files):
        scores = torch.from_numpy(f["seg"])
        want_o = torch.sort(scores, dim=-1, descending=True).values[..., 1].numpy()
        want_v = torch.max(scores, dim=-1)[0].numpy()
        assert o["track"].dtype == v["track"].dtype == np.float32 and o["track"].shape == f["seg"].shape[:2]
        assert np.array_equal(o["track"], want_o, equal_nan=True) and np.array_equal(v["track"], want_v, equal_nan=True)
        for k in ("starts", "res"):
            assert np.array_equal(o[k], f[k]) and np.array_equal(v[k], f[k])
        assert o["shift"] == v["shift"] == f["shift"] and o["uri"] == v["uri"] == f["uri"]
        assert o["stored"] == [(s, e, str(l)) for s, e, l in f["turns"]] and v["turns"] == f["turns"]
    assert np.isnan(osd.files[1]["track"][3]).all() and np.isnan(vad.files[1]["track"][5, 2])
    assert np.isnan(osd.files[1]["track"][5, 2]) == bool(np.isnan(np.sort(dia.files[1]["seg"][5, 2])[-2]))
    _same_arrays(osd, vad, PLAN_ARRAYS)
    taus = oc.taus_of(9, 4)
    direct = OsdTuneCache.from_arrays([dict(uri=f["uri"], track=o["track"], starts=f["starts"], res=f["res"], shift=f["shift"],
                                            reference=f["turns"]) for f, o in zip(dia.files, osd.files)], oc.config_of(2.5, 0.5))
    assert np.array_equal(osd.evaluate(taus, backend="host").per_file, direct.evaluate(taus, backend="host").per_file)
    assert (osd.evaluate(taus, backend="host").per_file[:, :, 0] > 0).all()
    with pytest.raises(ValueError, match="1 local speaker"):
        OsdTuneCache.from_tune_cache(_dia_cache(K=1))
    VadTuneCache.from_tune_cache(_dia_cache(K=1))
    with pytest.raises(ValueError, match="takes a TuneCache, got a VadTuneCache"):
        OsdTuneCache.from_tune_cache(vad)


def _config(latency=2.5, tau=0.5):
    return OverlappedSpeechDetectionConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                           latency=latency, tau_active=tau, device=torch.device("cpu"))


def _optimizer(tmp_path, cache, **kw):
    kw.setdefault("base_config", _config())
    return Optimizer(OverlappedSpeechDetection, None, None, tmp_path / "study", cache=cache, backend="host", **kw)


def test_optimizer_on_a_ready_cache(tmp_path):
    cache = OsdTuneCache.from_arrays(_files(), oc.config_of(2.5, 0.5))
    calls = []
    evaluate = cache.evaluate

    def counting(taus, **kw):
        calls.append(np.array(taus))
        return evaluate(taus, **kw)

    cache.evaluate = counting
    opt = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4)
    assert opt.kind == "osd" and [p.name for p in opt.hparams] == ["tau_active"]
    opt(10, show_progress=False)
    assert [c.shape for c in calls] == [(4, 1), (4, 1), (2, 1)] and len(opt.trials) == 10
    assert opt.trials[0]["params"] == {"tau_active": 0.5}                       # kick-start: the base configuration
    taus = np.concatenate(calls)
    result = evaluate(taus, backend="host")
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * result.rate)
    assert len(set(result.rate.tolist())) > 3
    best = int(np.argmin(result.rate))
    assert opt.best_performance == 100.0 * result.rate[best] and opt.best_hparams == opt.trials[best]["params"]
    assert json.loads((tmp_path / "study" / "study.json").read_text())["trials"] == opt.trials
    # a second call continues the study: the stored trials are loaded and never evaluated again
    calls.clear()
    again = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4, metric=OverlapDetectionErrorRate())
    assert again.trials == opt.trials
    again(3, show_progress=False)
    assert [len(c) for c in calls] == [3] and [t["number"] for t in again.trials] == list(range(13))
    # the F-measure, maximised: 100 x F of the components summed over the files
    calls.clear()
    fm = Optimizer(OverlappedSpeechDetection, None, None, tmp_path / "f", cache=cache, backend="host", base_config=_config(),
                   metric=OverlapDetectionFMeasure(), direction="maximize", seed=3, trials_per_batch=16)
    fm(12, show_progress=False)
    assert [t["params"] for t in fm.trials[:10]] == [t["params"] for t in opt.trials]
    result = evaluate(np.concatenate(calls), backend="host")
    f = detection_prf(result.components)[2]
    assert np.array_equal(np.array([t["value"] for t in fm.trials]), 100.0 * f) and len(set(f.tolist())) > 3
    best = int(np.argmax(f))
    assert fm.best_performance == 100.0 * f[best] and fm.best_hparams == fm.trials[best]["params"] and f[best] > 0
    calls.clear()
    more = Optimizer(OverlappedSpeechDetection, None, None, tmp_path / "f", cache=cache, backend="host", base_config=_config(),
                     metric=OverlapDetectionFMeasure(), direction="maximize", seed=3)
    more(2, show_progress=False)
    assert [len(c) for c in calls] == [2] and len(more.trials) == 14 and more.best_performance >= fm.best_performance
    with pytest.raises(ValueError, match="maximize.*not of.*minimize"):                # the stored study's direction
        Optimizer(OverlappedSpeechDetection, None, None, tmp_path / "f", cache=cache, base_config=_config())


def test_optimizer_refusals(tmp_path):
    cache = OsdTuneCache.from_arrays(_files(), oc.config_of(2.5, 0.5))
    vad = VadTuneCache.from_arrays([vc.file_of(vc.track_of(1, 5, 16))], vc.config_of(2.5))
    dia = _dia_cache()
    for other in (vad, dia):
        with pytest.raises(ValueError, match=f"OverlappedSpeechDetection: cache must be a OsdTuneCache, got a {type(other).__name__}"):
            _optimizer(tmp_path, other)
    vad_config = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                              latency=2.5, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="VoiceActivityDetection: cache must be a VadTuneCache, got a OsdTuneCache"):
        Optimizer(VoiceActivityDetection, None, None, tmp_path / "study", base_config=vad_config, cache=cache)
    with pytest.raises(ValueError, match="rho_update changes the model outputs: only tau_active"):
        _optimizer(tmp_path, cache, hparams=[base.TauActive, base.RhoUpdate])
    for scoring in ("host", "device"):
        with pytest.raises(ValueError, match="scoring: OverlappedSpeechDetection is scored where it is replayed"):
            _optimizer(tmp_path, cache, scoring=scoring)
    for metric in (DetectionErrorRate(), DiarizationErrorRate()):
        with pytest.raises(ValueError, match=f"metric {type(metric).__name__}: the replay of OverlappedSpeechDetection "
                                             "scores the overlap detection error rate"):
            _optimizer(tmp_path, cache, metric=metric)
    with pytest.raises(ValueError, match="OverlapDetectionFMeasure.*minimize.*maximize"):
        _optimizer(tmp_path, cache, metric=OverlapDetectionFMeasure())
    with pytest.raises(ValueError, match="OverlapDetectionFMeasure"):
        Optimizer(VoiceActivityDetection, None, None, tmp_path / "study", base_config=vad_config, cache=vad,
                  metric=OverlapDetectionFMeasure(), direction="maximize")

    class Custom(OverlappedSpeechDetection):
        pass

    with pytest.raises(ValueError, match="Custom"):
        Optimizer(Custom, None, None, tmp_path / "study", base_config=_config(), cache=cache)
    # the question "which of the two original caches" keeps its answer
    with pytest.raises(ValueError):
        _pipeline_kind(OverlappedSpeechDetection)
    assert _pipeline_kind(SpeakerDiarization) == "dia" and _pipeline_kind(VoiceActivityDetection) == "vad"
    assert not (tmp_path / "study").exists()


def test_detection_prf_by_hand():
    # total, correct, false alarm, missed detection, confusion
    p, r, f = detection_prf(np.array([10.0, 6.0, 2.0, 4.0, 0.0]))
    assert (p, r) == (0.75, 0.6) and abs(f - 2 * 0.75 * 0.6 / 1.35) <= 1e-15 and abs(f - 2.0 / 3.0) <= 1e-15
    table = np.array([[[10.0, 6.0, 2.0, 4.0, 0.0],          # the plain case
                       [10.0, 0.0, 0.0, 10.0, 0.0],         # nothing retrieved: precision 1, recall 0 -> F 0
                       [0.0, 0.0, 3.0, 0.0, 0.0]],          # nothing relevant: recall 1, precision 0 -> F 0
                      [[0.0, 0.0, 0.0, 0.0, 0.0],           # neither: precision 1, recall 1 -> F 1
                       [10.0, 0.0, 5.0, 10.0, 0.0],         # precision 0, recall 0: F 0, not 0 / 0
                       [8.0, 8.0, 0.0, 0.0, 0.0]]])         # perfect
    p, r, f = detection_prf(table)
    assert p.shape == r.shape == f.shape == (2, 3)
    assert np.array_equal(p, [[0.75, 1.0, 0.0], [1.0, 0.0, 1.0]]) and np.array_equal(r, [[0.6, 0.0, 1.0], [1.0, 0.0, 1.0]])
    assert np.allclose(f, [[2.0 / 3.0, 0.0, 0.0], [1.0, 0.0, 1.0]], rtol=0, atol=1e-15) and not np.isnan(f).any()
    assert detection_prf(dict(zip(COMPONENTS, table[0, 0])))[2] == f[0, 0]
    with pytest.raises(ValueError, match="components"):
        detection_prf(np.zeros((3, 4)))
    # the metric: the components of OverlapDetectionErrorRate, summed over the files before F is taken
    ref = _annotation([(0.0, 10.0, "a"), (2.0, 6.0, "b")])                         # overlap (2, 6)
    hyp = _annotation([(3.0, 7.0, "overlap")])                                    # correct 3, false alarm 1, missed 1
    metric, rate = OverlapDetectionFMeasure(), OverlapDetectionErrorRate()
    assert metric.components(ref, hyp) == rate.components(ref, hyp)
    assert metric(ref, hyp) == 0.75 and abs(metric) == 0.75                        # P = R = 3 / 4
    second = _annotation([(0.0, 4.0, "a"), (0.0, 4.0, "b")])                       # overlap (0, 4), nothing retrieved
    assert metric(second, Annotation()) == 0.0
    assert abs(abs(metric) - 2 * 0.75 * 0.375 / 1.125) <= 1e-15                   # correct 3 of 4 retrieved, of 8 relevant
    assert "overlap detection f-measure" in metric.report() and " 50.00 " in metric.report()
    metric.reset()
    assert abs(metric) == 1.0 and metric.accumulated["total"] == 0.0


def test_exports_and_command_line(tmp_path):
    import diart_amd
    assert diart_amd.OsdTuneCache is OsdTuneCache and diart_amd.VadTuneCache is VadTuneCache
    from diart_amd import tune
    OsdTuneCache.from_arrays(_files(), oc.config_of(2.5, 0.5)).save(tmp_path / "osd.npz")
    VadTuneCache.from_arrays([vc.file_of(vc.track_of(1, 5, 16))], vc.config_of(2.5)).save(tmp_path / "vad.npz")
    common = [str(tmp_path), "--reference", str(tmp_path), "--num-iter", "6", "--seed", "2", "--trials-per-batch", "4",
              "--latency", "2.5", "--cpu"]
    osd = common + ["--pipeline", "OverlappedSpeechDetection"]
    models = (M.SegmentationModel(lambda: scenarios.ToySegmentation()), None)
    parsed = tune.parser().parse_args(osd + ["--output", "x"])
    assert parsed.pipeline == "OverlappedSpeechDetection" and parsed.objective == "der" and parsed.hparams is None
    assert tune.parser().parse_args(osd + ["--output", "x", "--objective", "fmeasure"]).objective == "fmeasure"
    with pytest.raises(SystemExit):
        tune.parser().parse_args(osd + ["--output", "x", "--objective", "recall"])
    # --embedding and the clustering arguments are ignored, --hparams defaults to tau_active
    args = tune.parser().parse_args(osd + ["--output", str(tmp_path / "study"), "--cache", str(tmp_path / "osd.npz"),
                                           "--embedding", "no-such-file", "--delta-new", "0.2", "--max-speakers", "99"])
    opt = tune.run(args, models=models)
    assert opt.pipeline_class is OverlappedSpeechDetection and isinstance(opt.cache, OsdTuneCache) and opt.direction == "minimize"
    assert len(opt.trials) == 6 and all(list(t["params"]) == ["tau_active"] for t in opt.trials)
    assert opt.trials[0]["params"] == {"tau_active": 0.5} and (tmp_path / "study" / "study.json").exists()
    fm = tune.run(tune.parser().parse_args(osd + ["--output", str(tmp_path / "f"), "--cache", str(tmp_path / "osd.npz"),
                                                  "--objective", "fmeasure"]), models=models)
    assert fm.direction == "maximize" and fm.fmeasure and [t["params"] for t in fm.trials] == [t["params"] for t in opt.trials]
    assert fm.best_performance == max(t["value"] for t in fm.trials)
    with pytest.raises(ValueError, match="holds a VadTuneCache, not an OsdTuneCache"):
        tune.run(tune.parser().parse_args(osd + ["--output", str(tmp_path / "s2"), "--cache", str(tmp_path / "vad.npz")]),
                 models=models)
    with pytest.raises(SystemExit, match="tau_active"):
        tune.run(tune.parser().parse_args(osd + ["--output", str(tmp_path / "s3"), "--hparams", "delta_new"]), models=models)
    for pipeline in ("VoiceActivityDetection", "SpeakerDiarization"):
        with pytest.raises(SystemExit, match="--objective fmeasure.*OverlappedSpeechDetection"):
            tune.run(tune.parser().parse_args(common + ["--pipeline", pipeline, "--output", str(tmp_path / "s4"),
                                                        "--objective", "fmeasure"]), models=models)
