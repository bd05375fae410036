"""Tuning OverlappedSpeechDetection on the GPU (the VAD tuner's kernels, csrc/k_tune_vad.hip, fed the overlap track and
the prefix sums of the reference's overlap regions) against the host backend on the same cache: the aggregated scores
and the masks are EQUAL, the components agree within 1e-9 x total (tests/test_gpu_tune_vad.py's rule: the kernel adds
differences of prefix sums where the host adds the cells' durations one by one).  Synthetic tracks
(tests/tune_osd_cases.py); end to end with the synthetic segmentation last."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_osd_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu


def _bars(cache, per_file):
    """1e-9 x total per file; where a file's total is 0, 1e-9 x the sum of its cells' durations."""
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


def _compare(cache, taus, what, busy_file=None):
    host_agg, host_bits = cache.replay(taus, backend="host")
    host = cache.evaluate(taus, backend="host")
    if busy_file is not None:         # the comparison is not vacuous: the yardstick itself sees both kinds of error
        both = float(((host.per_file[:, busy_file, 2] > 0) & (host.per_file[:, busy_file, 3] > 0)).mean())
        assert both >= 0.5 and (host.per_file[:, busy_file, 0] > 0).all(), (what, both)
    agg, bits = cache.replay(taus, backend="gpu")
    assert agg.dtype == np.float64 and agg.shape == host_agg.shape and bits.dtype == np.uint32 and bits.shape == host_bits.shape
    bad = np.flatnonzero(agg.view(np.int64) != host_agg.view(np.int64))
    assert bad.size == 0, (what, f"{bad.size} of {agg.size} aggregated scores differ, first at {bad[0]}: "
                                 f"host {host_agg[bad[0]]!r}, gpu {agg[bad[0]]!r}")
    bad = np.argwhere(bits != host_bits)
    assert bad.shape[0] == 0, (what, f"{bad.shape[0]} of {bits.size} masks differ, first at {bad[0].tolist()}")
    dev = cache.evaluate(taus, backend="gpu")
    assert dev.per_file.shape == host.per_file.shape and (dev.status == -1).all()
    err, bars = np.abs(dev.per_file - host.per_file), _bars(cache, host.per_file)[..., None]
    print(what, "largest error / bar", float((err / bars).max()))
    worst = np.unravel_index(np.argmax(err - bars), err.shape)
    assert (err <= bars).all(), (what, worst, dev.per_file[worst], host.per_file[worst])
    assert np.abs(dev.rate - host.rate).max() <= 3e-9
    # agg is computed once per cache and device: a second call hands the same values back
    again = cache.replay(taus[:1], backend="gpu")[0]
    assert np.array_equal(again.view(np.int64), agg.view(np.int64)) and len(cache._dev) == 1
    return host, dev


@pytest.mark.parametrize("name", list(oc.EDGES))
def test_edges(gpu, name):
    """A one-chunk file beside a 61-chunk file with shift -1.25: F = 16 at latency 0.5, 2.5 and 5.0; F = 1; T = 1 and
    T = 67."""
    cache, taus = oc.edge_cache(name)
    assert taus.shape[0] == oc.EDGES[name][2]
    _compare(cache, taus, name, busy_file=1)


def test_carry(gpu):
    """300 chunks whose chunks 40 to 250 are all zero beside a file of 3 chunks, fewer than the buffers of latency
    5.0."""
    cache = oc.carry_cache()
    assert cache.nwin == 10 and int(cache.chunk_off[1]) == 300 and cache.N == 2
    _compare(cache, oc.taus_of(*oc.CARRY_TAUS), "carry", busy_file=0)
    silent = cache.replay(np.array([0.3]), backend="gpu")[1][0, int(cache.row_off[52]):int(cache.row_off[250])]
    assert not silent.any()


def test_degenerate(gpu):
    """A file whose track is all zero (every overlap missed), a file whose reference has speech and no overlap (total =
    0: the rate follows _Accumulating._rate), a chunk of NaN (its rows are no overlap)."""
    cache = oc.degenerate_cache()
    taus = oc.taus_of(33, 9)
    host, dev = _compare(cache, taus, "degenerate")
    positive = taus > 0
    assert (dev.per_file[positive, 0, 3] == dev.per_file[positive, 0, 0]).all() and (dev.per_file[positive, 0, 2] == 0).all()
    assert (dev.per_file[:, 0, 0] > 0).all()
    assert (dev.per_file[:, 1, 0] == 0).all() and (dev.per_file[:, 1, 3] == 0).all() and (dev.per_file[:-1, 1, 2] > 0).any()
    assert np.isnan(cache.replay(taus, backend="gpu")[0]).any()
    alone = oc.cache_of([dict(cache.files[1], reference=oc.NO_OVERLAP)], 2.5)
    a, b = alone.evaluate(taus, backend="host"), alone.evaluate(taus, backend="gpu")
    assert np.array_equal(a.rate, b.rate) and set(a.rate.tolist()) == {0.0, 1.0}


def test_from_tune_cache_on_the_device_is_the_host_statement(gpu):
    """OsdTuneCache.from_tune_cache(device=gpu) runs overlap_track_kernel on the diarization cache's raw scores: a
    selection, so the tracks equal the torch statement's on the host, NaN included."""
    from diart_amd.optim import OsdTuneCache, TuneCache
    files = []
    for n, c in enumerate((5, 61)):
        seg, emb = tc.random_outputs(31 + n, c, 16, 3, 8)
        if n == 1:
            seg[3], seg[5, 2, 0] = np.nan, np.nan
        files.append(tc.file_of(seg, emb, shift=-0.5 * n, uri=f"dia{n}"))
    dia = TuneCache.from_arrays(files, tc.config_of(0.6, 0.3, 1.0, 4, 2.5))
    host, dev = OsdTuneCache.from_tune_cache(dia), OsdTuneCache.from_tune_cache(dia, device=gpu)
    assert np.isnan(host.seg).any() and host.seg.tobytes() == dev.seg.tobytes()
    taus = oc.taus_of(9, 4)
    _compare(dev, taus, "from_tune_cache")


def test_optimizer_matches_benchmark_end_to_end(gpu, tmp_path, monkeypatch):
    """Two 40 s files through the synthetic segmentation, speaker references with overlap: Optimizer(
    OverlappedSpeechDetection, ...) collects once, and for the taus at the 10 / 50 / 90 % quantiles of the cache's finite
    aggregated scores the five components are Benchmark(...)(OverlappedSpeechDetection, config at that tau)'s
    OverlapDetectionErrorRate components within 1e-9 x total, hence the rate within 3e-9."""
    import torch
    from diart_amd import models as m
    from diart_amd.blocks.osd import OverlappedSpeechDetection, OverlappedSpeechDetectionConfig
    from diart_amd.features import Annotation, Segment
    from diart_amd.inference import Benchmark, write_wav
    from diart_amd.metrics import COMPONENTS, OverlapDetectionErrorRate
    from diart_amd.optim import Optimizer, OsdTuneCache, trial_config
    from diart_amd.synth import synth_segmentation_state, synth_stream
    speech, refs = tmp_path / "wav", tmp_path / "rttm"
    speech.mkdir()
    refs.mkdir()
    config = OverlappedSpeechDetectionConfig(segmentation=m.SegmentationModel.from_state(synth_segmentation_state(), max_batch=8),
                                             latency=2.5, device=torch.device("cuda", 0))
    for i, seconds in enumerate((40.3, 38.0)):
        write_wav(speech / f"f{i}.wav", synth_stream(900 + i, seconds, num_speakers=2 + i), 16000)
        # three speakers taking turns of different periods over the file: two and three at once, a label overlapping
        # itself, regions that touch
        ann = Annotation(uri=f"f{i}")
        turns = tc.reference_for(int((seconds - 5.0) / 0.5) + 1) + [(1.0, 3.5, "ref0"), (20.0, 21.0, "ref1"), (21.0, 22.5, "ref2")]
        for n, (s, e, label) in enumerate(turns):
            ann[Segment(s, e), n] = label
        (refs / f"f{i}.rttm").write_text(ann.to_rttm())
    collected = []
    collect = OsdTuneCache.collect.__func__
    monkeypatch.setattr(OsdTuneCache, "collect", classmethod(lambda cls, *a, **kw: collected.append(1) or collect(cls, *a, **kw)))
    opt = Optimizer(OverlappedSpeechDetection, speech, refs, tmp_path / "study", batch_size=8, base_config=config, seed=5)
    opt(4, show_progress=False)
    cache = opt.cache
    assert isinstance(cache, OsdTuneCache) and len(opt.trials) == 4 and opt.trials[0]["params"] == {"tau_active": 0.5}
    agg = cache.replay(np.array([0.5]))[0]
    taus = np.quantile(agg[np.isfinite(agg)], [0.1, 0.5, 0.9])
    assert taus[0] < taus[1] < taus[2]
    result = cache.evaluate(taus)
    values = opt.objective([{"tau_active": float(t)} for t in taus])
    assert collected == [1]
    durations = set()
    for t, tau in enumerate(taus):
        bench = Benchmark(speech, refs, show_report=False, batch_size=8, concurrent_files=0)
        metric = bench(OverlappedSpeechDetection, trial_config(config, {"tau_active": float(tau)}))
        assert isinstance(metric, OverlapDetectionErrorRate)
        want = np.array([metric.accumulated[c] for c in COMPONENTS])
        comp = result.components[t]
        print(float(tau), comp, want)
        assert want[0] > 0 and np.abs(comp - want).max() <= 1e-9 * want[0], (tau, comp, want)
        assert abs(values[t] - 100.0 * abs(metric)) <= 3e-7, (tau, values[t], 100.0 * abs(metric))
        durations.add(round(float(comp[1] + comp[2]), 6))                      # correct + false alarm: the hypothesis
    assert len(durations) >= 2, "every trial's hypothesis has the same duration"
