"""Tuning delta_id on the GPU (csrc/k_tune_ident.hip) against the host backend on tests/tune_ident_cases.py's cases: the
names of tune_name_kernel are the host's integers (which tests/test_tune_ident_host.py holds against
gallery.SpeakerNames in Python), the components of tune_ident_score_kernel lie within 1e-9 x the pair's total of the
host's, two calls give the same doubles, and the stored match is the gallery kernel's."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_cells_cases as cc  # noqa: E402
import tune_ident_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    """(base TuneCache, IdentTuneCache matched on the GPU, hparams (16, 4)); computed once, never changed."""
    base = ic.base_cache()
    return base, base.with_gallery(ic.gallery()), ic.trials()


@pytest.fixture(scope="module")
def stop():
    cache, gallery, hp = ic.stop_cache()
    return cache.with_gallery(gallery), hp


def test_with_gallery_stores_the_kernels_match(gpu, case):
    import torch
    _, cache, _ = case
    index, distance, _ = ic.gallery().match(cache.emb)
    assert np.array_equal(cache.match_index, index) and np.array_equal(cache.match_distance, distance, equal_nan=True)
    x = torch.from_numpy(cache.emb).to(torch.float64).reshape(-1, ic.D)
    g = torch.from_numpy(ic.gallery_rows()).to(torch.float64)
    d64 = (1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None])).numpy().reshape(120, ic.K, -1)
    ok = cache.match_index >= 0
    assert np.array_equal(ok, ~np.isnan(cache.emb).any(axis=2)) and (~ok).any() and np.isnan(cache.match_distance[~ok]).all()
    exact = np.take_along_axis(d64, np.maximum(cache.match_index, 0)[..., None].astype(np.int64), axis=2)[..., 0]
    worst = np.abs(cache.match_distance.astype(np.float64) - exact)[ok].max()
    print("largest distance error", worst / 2.0 ** -24, "x 2^-24")
    assert worst <= (ic.D + 8) * 2.0 ** -24


def test_names_are_the_hosts(gpu, case, stop):
    for cache, hp in ((case[1], case[2]), stop):
        host, dev = cache.replay_names(hp, backend="host"), cache.replay_names(hp, backend="gpu")
        for h, d in zip(host, dev):
            assert h.dtype == d.dtype and np.array_equal(h, d)
    assert (dev[1][0] == [-1, 3]).all()                                   # the stopped chain


def test_evaluate_agrees_with_the_host(gpu, case, stop):
    for cache, hp in ((case[1], case[2]), stop):
        host, dev = cache.evaluate(hp, backend="host"), cache.evaluate(hp, backend="gpu")
        worst = np.abs(host.per_file - dev.per_file).max(axis=(0, 1))
        print("largest difference per component", worst, "smallest total", host.per_file[..., 0].min())
        assert (host.per_file[..., 0] > 0).all() and (np.abs(host.per_file - dev.per_file) <= ic.bars(host.per_file)).all()
        assert np.array_equal(host.status, dev.status) and np.array_equal(np.isnan(host.rate), np.isnan(dev.rate))
        again = cache.evaluate(hp, backend="gpu")
        assert np.array_equal(dev.per_file, again.per_file) and np.array_equal(dev.rate, again.rate, equal_nan=True)
        # trials in batches: the same doubles
        batched = cache.evaluate(hp, backend="gpu", memory_budget=3 * cache.bytes_per_trial)
        assert np.array_equal(dev.per_file, batched.per_file)
    assert np.isnan(dev.rate).tolist() == [True, False, False, False]


def test_the_diarization_tuner_is_untouched(gpu):
    base, hp = ic.base_cache(), ic.trials()
    before = [base.evaluate(hp[:, :3], backend="gpu", scoring=s) for s in (None, "device")]
    base.with_gallery(ic.gallery()).evaluate(hp, backend="gpu")
    after = [base.evaluate(hp[:, :3], backend="gpu", scoring=s) for s in (None, "device")]
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert np.array_equal(x, y, equal_nan=True)


def test_optimizer(gpu, case, tmp_path):
    import types
    from diart_amd.blocks.diarization import SpeakerDiarization
    from diart_amd.metrics import IdentificationErrorRate
    from diart_amd.optim import Optimizer
    _, cache, _ = case
    config = types.SimpleNamespace(**tc.config_of(*ic.OWN, ic.G, ic.LATENCY))
    opts = {}
    for backend in ("host", "gpu"):
        opts[backend] = Optimizer(SpeakerDiarization, None, None, tmp_path / backend, base_config=config, cache=cache,
                                  backend=backend, seed=7, gallery=ic.gallery(), delta_id=0.4,
                                  metric=IdentificationErrorRate())
        opts[backend](32, show_progress=False)
    a, b = opts["host"].trials, opts["gpu"].trials
    assert len(a) == 32 and [t["params"] for t in a] == [t["params"] for t in b]
    assert [t["value"] is None for t in a] == [t["value"] is None for t in b]
    va, vb = (np.array([t["value"] for t in ts if t["value"] is not None]) for ts in (a, b))
    assert va.shape[0] >= 16 and (np.abs(va - vb) <= 1e-9 * np.abs(va)).all()
    best = np.sort(va)
    assert best[1] - best[0] > 1e-9 * best[1], "two trials tie for the best: pick another seed"
    assert opts["host"].best_trial["number"] == opts["gpu"].best_trial["number"]
    assert "delta_id" in opts["gpu"].best_hparams


def test_entry_points_refuse_before_the_gpu_is_touched(gpu, case):
    """Status 2 and the function's name: T < 1, G > 32, V < 1 and a NULL pointer, with a live context and every other
    pointer NULL-free but never dereferenced."""
    import torch
    from diart_amd import _lib
    lib, ctx = _lib.load(), _lib.context(gpu.index)
    one = torch.zeros(64, dtype=torch.int32, device=gpu).data_ptr()

    def name(T=1, G=5, V=6, assign=one):                                 # one point: points = planes = 1
        return lib.dz_tune_name(ctx, T, 1, 1, 1, 1, 3, G, V, one, assign, one, one, one, one, one, one, None, 64, None)

    for kw in (dict(T=0), dict(G=33), dict(V=0), dict(assign=None)):
        assert name(**kw) == 2 and "dz_tune_name" in lib.dz_last_error().decode(), kw

    def score(T=1, G=5, bits=one):
        return lib.dz_tune_ident_score_gpu(ctx, cc.ref(cc.filled(one, G)), T, 1, bits, one, one, one, 1, one, None)

    for kw in (dict(T=0), dict(G=33), dict(bits=None)):
        assert score(**kw) == 2 and "dz_tune_ident_score_gpu" in lib.dz_last_error().decode(), kw
