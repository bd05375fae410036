"""The tuner's GPU replay (csrc/k_tune.hip) against the host replay (dz_clu_step -> dz_tail_step) on the same cache:
the assignments, the statuses and the packed frame masks are EQUAL, not close.  Both sides do the same fp64 operations
in the same order with correctly rounded results (dot2's two partial sums, sqrt, division, no contraction), so there is
no tolerance to choose.  All inputs are synthetic (tests/tune_cases.py); end to end with the synthetic models last."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
from tune_cases import scenarios  # noqa: E402

pytestmark = pytest.mark.gpu


def _both(cache, hp):
    host = cache.replay(hp, backend="host")
    dev = cache.replay(hp, backend="gpu")
    return host, dev


def _assert_equal(host, dev, what):
    for name, h, d in zip(("assign", "status", "bits"), host, dev):
        assert h.dtype == d.dtype and h.shape == d.shape, (what, name, h.dtype, d.dtype, h.shape, d.shape)
        bad = np.argwhere(h != d)
        assert bad.shape[0] == 0, (what, name, f"{bad.shape[0]} of {h.size} differ, first at {bad[0].tolist()}: "
                                               f"host {h[tuple(bad[0])]}, gpu {d[tuple(bad[0])]}")


@pytest.mark.parametrize("name", list(scenarios.CLUSTERING))
def test_golden_scenarios(gpu, name):
    """Each golden scenario as a one-file cache under its own parameters and seven neighbours (F in {16, 32}, K in
    {3, 4}, D in {8, 16, 24}, G in {4, 20}; `crowded` pins the last-bit LSAP ties); the scenario's own parameters
    reproduce the assignments the reference's clustering made (clustering_<name>.npz)."""
    from diart_amd.optim import TuneCache
    z = np.load(tc.GOLD / f"clustering_{name}.npz")
    tau, rho, delta, G = z["params"]
    cache = TuneCache.from_arrays([tc.file_of(z["seg"], z["emb"], shift=-0.75)], tc.config_of(tau, rho, delta, G, 2.5))
    hp = tc.neighbours(tau, rho, delta)
    assert hp.shape == (8, 3)
    host, dev = _both(cache, hp)
    _assert_equal(host, dev, name)
    assert (dev[1] == -1).all()
    assert np.array_equal(dev[0][0], z["assign"].astype(np.int8)), name
    assert len({a.tobytes() for a in dev[0]}) > 1, "the neighbours all made the same assignments"


@pytest.mark.parametrize("seed,K,D,G,tau,rho,delta", scenarios.CLUSTERING_LONG_RANDOM)
def test_long_random(gpu, seed, K, D, G, tau, rho, delta):
    """The first 300 steps of each CLUSTERING_LONG_RANDOM seed (D = 512; K = G = 3 and K = G = 4; NaN embeddings,
    duplicated rows, silent chunks; no seed has G < K: test_edges' K4G3 and K8G5 hold that) under the seed's own parameters and 31 uniform draws.  The seeds differ in K, D and
    max_speakers, which the files of one cache share, so each seed is a cache of its own.  Every chain runs to the end."""
    from diart_amd.optim import TuneCache
    seg, emb = tc.long_random(seed, K, D, G)
    cache = TuneCache.from_arrays([tc.file_of(seg, emb)], tc.config_of(tau, rho, delta, G, 5.0))
    hp = tc.random_trials((tau, rho, delta), 32, seed=0)
    host, dev = _both(cache, hp)
    assert (host[1] == -1).all() and (dev[1] == -1).all()
    _assert_equal(host, dev, seed)
    assert len({a.tobytes() for a in dev[0]}) >= 20, "the trials are copies of each other"


@pytest.mark.parametrize("name", list(tc.EDGES))
def test_edges(gpu, name):
    """D = 1 and D = 15 (dot2's odd tail), K = 1, G = 1, F = 1, 1 < G < K (K = 4 with G = 3, K = 8 with G = 5: the
    transposed assignment problem), a file of one chunk beside one of 61, T = 1 and T = 67, latency = step, 2.5 and 5.0;
    `raises`: a chain that stops at the chunk where the reference raises "Cannot update unknown centers"."""
    cache, hp = tc.edge_cache(name)
    assert hp.shape[0] == tc.EDGES[name][5]
    host, dev = _both(cache, hp)
    _assert_equal(host, dev, name)


def test_evaluate_is_the_same_on_both_backends(gpu):
    """evaluate() batches the trials by its memory budget and scores the masks on the host: same numbers either way."""
    cache, hp = tc.edge_cache("lat_mid")
    a = cache.evaluate(hp, backend="host")
    b = cache.evaluate(hp, backend="gpu", memory_budget=3 * cache.bytes_per_trial)      # three trials per batch
    assert np.array_equal(a.per_file, b.per_file) and np.array_equal(a.status, b.status)
    assert np.array_equal(a.rate, b.rate, equal_nan=True) and np.isfinite(a.rate).any()


def test_optimizer_matches_benchmark_end_to_end(gpu, tmp_path):
    """Two short files through the synthetic models: Optimizer(...)(8) gives, for each trial, what
    Benchmark(...)(SpeakerDiarization, config of that trial) reports: the five components within 1e-9 x total (the bar
    of tests/test_tune_host.py: the two differ only in the order in which the durations of a file are summed), hence
    the rate, a ratio of three of them to the total, within 3e-9, i.e. 3e-7 in percent."""
    import torch
    from diart_amd import models as m
    from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig
    from diart_amd.inference import Benchmark, write_wav
    from diart_amd.metrics import COMPONENTS
    from diart_amd.optim import Optimizer, trial_config
    from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream
    speech, refs = tmp_path / "wav", tmp_path / "rttm"
    speech.mkdir()
    refs.mkdir()
    config = SpeakerDiarizationConfig(segmentation=m.SegmentationModel.from_state(synth_segmentation_state(), max_batch=8),
                                      embedding=m.EmbeddingModel.from_state(synth_embedding_state(), max_batch=8),
                                      latency=2.5, device=torch.device("cuda", 0))
    for i, seconds in enumerate((17.3, 11.0)):
        write_wav(speech / f"f{i}.wav", synth_stream(900 + i, seconds, num_speakers=2 + i), 16000)
    # the references: the pipeline's own output at the base configuration (as an RTTM file rounds it)
    Benchmark(speech, None, refs, show_report=False, batch_size=8, concurrent_files=0)(SpeakerDiarization, config)
    opt = Optimizer(SpeakerDiarization, speech, refs, tmp_path / "study", batch_size=8, base_config=config, seed=5)
    opt(8, show_progress=False)
    assert len(opt.trials) == 8 and opt.trials[0]["params"] == {"tau_active": 0.6, "rho_update": 0.3, "delta_new": 1.0}
    hp = np.array([[t["params"][k] for k in ("tau_active", "rho_update", "delta_new")] for t in opt.trials])
    components = opt.cache.evaluate(hp).components
    for trial, comp in zip(opt.trials, components):
        bench = Benchmark(speech, refs, show_report=False, batch_size=8, concurrent_files=0)
        metric = bench(SpeakerDiarization, trial_config(config, trial["params"]))
        want = np.array([metric.accumulated[c] for c in COMPONENTS])
        print(trial, comp, want)
        assert want[0] > 0 and np.abs(comp - want).max() <= 1e-9 * want[0], (trial, comp, want)
        assert trial["value"] is not None and abs(trial["value"] - 100.0 * abs(metric)) <= 3e-7, (trial, 100.0 * abs(metric))
    assert len({t["value"] for t in opt.trials}) > 1, "every trial scored the same"
