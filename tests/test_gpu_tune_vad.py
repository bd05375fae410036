"""Tuning VoiceActivityDetection on the GPU (csrc/k_tune_vad.hip) against the host backend on the same cache: the
aggregated scores and the masks are EQUAL (both sides compile csrc/tune_core.h: the same fp64 operations in the same
order, no contraction, the quotient correctly rounded), the components of tune_vad_score_kernel agree with
dz_tune_score on the host's masks within 1e-9 x total (the kernel adds differences of prefix sums where the host adds
the cells' durations one by one).  Synthetic tracks (tests/tune_vad_cases.py); end to end with the synthetic
segmentation last."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_vad_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu


def _bars(cache, per_file):
    """1e-9 x total per file; where a file's total is 0, 1e-9 x the sum of its cells' durations."""
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


def _both_errors(host, n):
    """The share of the trials in which file n has false alarm and missed detection."""
    return float(((host.per_file[:, n, 2] > 0) & (host.per_file[:, n, 3] > 0)).mean())


def _compare(cache, taus, what, busy_file=None):
    host_agg, host_bits = cache.replay(taus, backend="host")
    host = cache.evaluate(taus, backend="host")
    if busy_file is not None:         # the comparison is not vacuous: the yardstick itself sees both kinds of error
        assert _both_errors(host, busy_file) >= 0.5, (what, _both_errors(host, busy_file))
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
    return host, dev


@pytest.mark.parametrize("name", list(vc.EDGES))
def test_edges(gpu, name):
    """A one-chunk file beside a 61-chunk file with shift -1.25: F = 16 at latency 0.5 (one buffer per step: the
    first chunk's prepend and plain rows only), 2.5 and 5.0; F = 1; T = 1 and T = 67."""
    cache, taus = vc.edge_cache(name)
    assert taus.shape[0] == vc.EDGES[name][2]
    _compare(cache, taus, name, busy_file=1)


def test_collar(gpu):
    """F = 293 at latency 0.5: inactive runs of 1, 2, 3 and 4 frames inside a step, across a step's end and up to a
    step's last row (tests/tune_vad_cases.py collar_runs).  A wrong merge moves a component by a frame, 0.017 s."""
    cache, on = vc.collar_cache()
    taus = np.concatenate([vc.taus_of(33, 11), [0.5]])
    host, _ = _compare(cache, taus, "collar")
    assert np.array_equal(cache.replay(np.array([0.5]), backend="gpu")[1][0].astype(bool), on)
    assert host.per_file[-1, 0, 2] > 0 and host.per_file[-1, 0, 3] > 0


def test_carry(gpu):
    """300 chunks whose chunks 40 to 250 are all zero (the end of the last turn before them is carried across a
    hundred lanes without a turn) beside a file of 3 chunks, fewer than the buffers of latency 5.0."""
    cache = vc.carry_cache()
    assert cache.nwin == 10 and int(cache.chunk_off[1]) == 300 and cache.N == 2
    host, _ = _compare(cache, vc.taus_of(33, 8), "carry", busy_file=0)
    silent = cache.replay(np.array([0.3]), backend="host")[1][0, int(cache.row_off[52]):int(cache.row_off[250])]
    assert not silent.any()


def test_degenerate(gpu):
    """A file whose track is all zero (everything missed), a file with an empty reference (total = 0: the rate follows
    _Accumulating._rate), a chunk of NaN (its rows are not speech)."""
    cache = vc.degenerate_cache()
    taus = vc.taus_of(33, 9)
    host, dev = _compare(cache, taus, "degenerate")
    positive = taus > 0
    assert (dev.per_file[positive, 0, 3] == dev.per_file[positive, 0, 0]).all() and (dev.per_file[positive, 0, 2] == 0).all()
    assert (dev.per_file[:, 1, 0] == 0).all() and (dev.per_file[:, 1, 3] == 0).all() and (dev.per_file[:-1, 1, 2] > 0).any()
    agg = cache.replay(taus, backend="gpu")[0]
    assert np.isnan(agg).any()
    alone = vc.cache_of([cache.files[1] | dict(reference=[])], 2.5)
    a, b = alone.evaluate(taus, backend="host"), alone.evaluate(taus, backend="gpu")
    assert np.array_equal(a.rate, b.rate) and set(a.rate.tolist()) <= {0.0, 1.0}


def test_optimizer_matches_benchmark_end_to_end(gpu, tmp_path):
    """Two short files through the synthetic segmentation: Optimizer(VoiceActivityDetection, ...)(8) gives, for each
    trial, what Benchmark(...)(VoiceActivityDetection, config of that trial) reports: the five components within
    1e-9 x total, hence the rate within 3e-9 (3e-7 in percent)."""
    import torch
    from diart_amd import models as m
    from diart_amd.blocks.vad import VoiceActivityDetection, VoiceActivityDetectionConfig
    from diart_amd.inference import Benchmark, write_wav
    from diart_amd.metrics import COMPONENTS, DetectionErrorRate
    from diart_amd.optim import Optimizer, VadTuneCache, trial_config
    from diart_amd.synth import synth_segmentation_state, synth_stream
    speech, refs = tmp_path / "wav", tmp_path / "rttm"
    speech.mkdir()
    refs.mkdir()
    config = VoiceActivityDetectionConfig(segmentation=m.SegmentationModel.from_state(synth_segmentation_state(), max_batch=8),
                                          latency=2.5, device=torch.device("cuda", 0))
    for i, seconds in enumerate((17.3, 11.0)):
        write_wav(speech / f"f{i}.wav", synth_stream(900 + i, seconds, num_speakers=2 + i), 16000)
    # the references: the pipeline's own output at the base configuration (as an RTTM file rounds it)
    Benchmark(speech, None, refs, show_report=False, batch_size=8, concurrent_files=0)(VoiceActivityDetection, config)
    opt = Optimizer(VoiceActivityDetection, speech, refs, tmp_path / "study", batch_size=8, base_config=config, seed=5)
    opt(8, show_progress=False)
    assert isinstance(opt.cache, VadTuneCache) and len(opt.trials) == 8 and opt.trials[0]["params"] == {"tau_active": 0.6}
    components = opt.cache.evaluate(np.array([t["params"]["tau_active"] for t in opt.trials])).components
    for trial, comp in zip(opt.trials, components):
        bench = Benchmark(speech, refs, show_report=False, batch_size=8, concurrent_files=0)
        metric = bench(VoiceActivityDetection, trial_config(config, trial["params"]))
        assert isinstance(metric, DetectionErrorRate)
        want = np.array([metric.accumulated[c] for c in COMPONENTS])
        print(trial, comp, want)
        assert want[0] > 0 and np.abs(comp - want).max() <= 1e-9 * want[0], (trial, comp, want)
        assert trial["value"] is not None and abs(trial["value"] - 100.0 * abs(metric)) <= 3e-7, (trial, 100.0 * abs(metric))
    assert len({t["value"] for t in opt.trials}) > 1, "every trial scored the same"
