"""The sweep on the GPU (csrc/k_tune_ident.hip) against the host backend on tests/tune_sweep_cases.py's
cases: the stored planes are the bits of the kernels the live engines run, the names of tune_name_kernel are the host's
integers at every point (which tests/test_tune_sweep_host.py holds against gallery.SpeakerNames in Python), the sweep's
components are those of the one-point kernel bit for bit and lie within 1e-9 x the pair's total of the host's, and
they do not depend on the call, the workgroups or the batches."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_cells_cases as cc  # noqa: E402
import tune_ident_cases as ic  # noqa: E402
import tune_sweep_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(gpu):
    """(normalised IdentTuneCache matched on the GPU, hp (16, 3), evaluate_sweep on "gpu"); computed once, never
    changed."""
    cache, hp = sc.normalised_cache(), sc.hp3()
    return cache, hp, cache.evaluate_sweep(hp, sc.THRESHOLDS, backend="gpu")


@pytest.fixture(scope="module")
def stop(gpu):
    cache, _, hp = sc.stop_case()
    return cache, hp


def test_the_planes_are_the_live_kernels_bits(gpu, case):
    cache = case[0]
    assert cache.normalised and cache.top_ns == sc.TOP_NS and cache.plane_index.shape == (2, 120, ic.K)
    for p, tn in enumerate(sc.TOP_NS):
        index, distance, _ = ic.gallery().with_cohort(sc.cohort(), tn).match_normalised(cache.emb)
        assert np.array_equal(cache.plane_index[p], index)
        assert np.array_equal(cache.plane_distance[p], distance, equal_nan=True)
    assert np.array_equal(cache.match_index, cache.plane_index[0])
    assert np.array_equal(cache.match_distance, cache.plane_distance[0], equal_nan=True)
    assert (cache.plane_index < 0).any() and np.isnan(cache.plane_distance[cache.plane_index < 0]).all()


def test_names_are_the_hosts_at_every_point(gpu, case, stop):
    cache, hp, _ = case
    cache.NAME_BLOCKS = 3                         # (on the instance) 480 chains stride over 3 workgroups
    try:
        for c, h, thr in ((cache, hp, sc.THRESHOLDS), (stop[0], stop[1], sc.STOP_THRESHOLDS)):
            host, dev = (c.replay_names_sweep(h, thr, backend=b) for b in ("host", "gpu"))
            for x, y in zip(host, dev):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            assert (dev[3] >= 0).any()
            for p, tn in enumerate(c.top_ns):     # one point at a time: replay_names on the point's plane
                one = c.replay_names(np.concatenate([h, np.full((h.shape[0], 1), thr[1])], axis=1), backend="gpu", top_n=tn)
                assert np.array_equal(one[3], dev[3][:, p, 1])
        assert (dev[1][0] == [-1, 3]).all()       # the stopped chain
    finally:
        del cache.NAME_BLOCKS
    assert cache.NAME_BLOCKS == type(cache).NAME_BLOCKS


def test_the_sweep_is_the_one_point_kernel_and_the_host(gpu, case, stop):
    for (cache, hp, dev), thr in ((case, sc.THRESHOLDS),
                                  ((stop[0], stop[1], stop[0].evaluate_sweep(stop[1], sc.STOP_THRESHOLDS, backend="gpu")),
                                   sc.STOP_THRESHOLDS)):
        # point by point through evaluate(backend="gpu"): bit for bit
        rate, comp, per_file = sc.point_by_point(cache, hp, thr, cache.top_ns, "gpu")
        assert np.array_equal(dev.per_file, per_file) and np.array_equal(dev.components, comp)
        assert np.array_equal(dev.rate, rate, equal_nan=True)
        # the host's sequential text
        host = cache.evaluate_sweep(hp, thr, backend="host")
        worst = np.abs(host.per_file - dev.per_file).max(axis=(0, 1, 2, 3))
        print("largest difference per component", worst, "smallest total", host.per_file[..., 0].min())
        assert (host.per_file[..., 0] > 0).all() and (np.abs(host.per_file - dev.per_file) <= ic.bars(host.per_file)).all()
        assert np.array_equal(host.status, dev.status) and np.array_equal(np.isnan(host.rate), np.isnan(dev.rate))
        # twice; two workgroups; batches of three trials: the same doubles
        assert sc.same_sweep(dev, cache.evaluate_sweep(hp, thr, backend="gpu"))
        cache.IDENT_BLOCKS = 2
        try:
            assert sc.same_sweep(dev, cache.evaluate_sweep(hp, thr, backend="gpu"))
        finally:
            del cache.IDENT_BLOCKS
        points = len(cache.top_ns) * len(thr)
        batched = cache.evaluate_sweep(hp, thr, backend="gpu", memory_budget=3 * cache.sweep_bytes_per_trial(points))
        assert sc.same_sweep(dev, batched)
    assert np.isnan(dev.rate[0]).all() and not np.isnan(dev.rate[1:]).any()       # the stopped trial, at every point
    assert len(np.unique(case[2].components[..., 1])) >= 10


def test_a_raw_cache_sweeps_on_the_gpu(gpu):
    raw, hp, thr = ic.base_cache().with_gallery(ic.gallery()), sc.hp3(), (0.0, 0.2, 0.5, 1.0, 2.0)
    dev = raw.evaluate_sweep(hp, thr, backend="gpu")
    rate, _, per_file = sc.point_by_point(raw, hp, thr, None, "gpu")
    assert dev.rate.shape == (16, 1, 5) and np.array_equal(dev.per_file, per_file) and np.array_equal(dev.rate, rate)


def test_entry_points_refuse_before_the_gpu_is_touched(gpu, case):
    """Status 2 and the function's name: T < 1, points outside 1 .. 256, planes outside 1 .. 8 or not dividing the
    points, G > 32 and a NULL pointer, with a live context and every other pointer NULL-free but never dereferenced."""
    import torch
    from diart_amd import _lib
    lib, ctx = _lib.load(), _lib.context(gpu.index)
    one = torch.zeros(64, dtype=torch.int32, device=gpu).data_ptr()

    def name(T=1, J=10, P=2, G=5, ptr=one):
        return lib.dz_tune_name(ctx, T, J, P, 1, 1, 3, G, 6, one, ptr, one, one, one, one, one, one, None, 64, None)

    for kw in (dict(T=0), dict(J=0), dict(J=257), dict(P=0), dict(P=9), dict(J=10, P=3), dict(G=33), dict(ptr=None)):
        assert name(**kw) == 2 and "dz_tune_name:" in lib.dz_last_error().decode(), kw

    def score(T=1, J=10, G=5, ptr=one):
        return lib.dz_tune_ident_score_gpu(ctx, cc.ref(cc.filled(one, G)), T, J, ptr, one, one, one, 1, one, None)

    for kw in (dict(T=0), dict(J=0), dict(J=257), dict(G=33), dict(ptr=None)):
        assert score(**kw) == 2 and "dz_tune_ident_score_gpu" in lib.dz_last_error().decode(), kw


def test_optimizer_sweep(gpu, case, tmp_path):
    from diart_amd.blocks.diarization import SpeakerDiarization
    from diart_amd.optim import Optimizer
    cache = case[0]
    config = types.SimpleNamespace(**tc.config_of(*ic.OWN, ic.G, ic.LATENCY))
    opts = {}
    for backend in ("host", "gpu"):
        opts[backend] = Optimizer(SpeakerDiarization, None, None, tmp_path / backend, base_config=config, cache=cache,
                                  backend=backend, seed=7, gallery=sc.gallery(), delta_id=-2.0, normalised=True, sweep=3)
        opts[backend](16, show_progress=False)
    a, b = opts["host"].trials, opts["gpu"].trials
    assert len(a) == 16 and [t["params"] for t in a] == [t["params"] for t in b]
    assert all("delta_id" in t["params"] and "top_n" in t["params"] for t in b)
    va, vb = (np.array([t["value"] for t in ts], dtype=np.float64) for ts in (a, b))
    assert not np.isnan(va).any() and (np.abs(va - vb) <= 1e-9 * np.abs(va)).all()
    best = np.sort(va)
    assert best[1] - best[0] > 1e-9 * best[1], "two trials tie for the best: pick another seed"
    assert opts["host"].best_trial["number"] == opts["gpu"].best_trial["number"]
