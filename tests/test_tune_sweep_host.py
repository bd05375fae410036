"""Tuning the cohort-normalised delta_id, swept inside each trial, without a GPU: the planes of a
normalised IdentTuneCache are the float64 statement's, the sweep's names are gallery.SpeakerNames(signed=True) in
Python, evaluate_sweep is evaluate point by point (backend "core": bit for bit; "host", the loop of the sequential
text: within 1e-9 x the pair's total) and metrics.IdentificationErrorRate on the named hypothesis, and the Optimizer
keeps every trial's best point."""
import ctypes as C
import json
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_ident_cases as ic  # noqa: E402
import tune_sweep_cases as sc  # noqa: E402

from diart_amd import _lib  # noqa: E402
from diart_amd import functional as F  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization  # noqa: E402
from diart_amd.optim import IdentTuneCache, Optimizer, SweepResult, TuneCache  # noqa: E402

@pytest.fixture(scope="module")
def case():
    """(cache, hp (16, 3), {backend: replay_names_sweep}, {backend: evaluate_sweep}, python hold (16, 2, 5, chunks, G));
    computed once, never changed."""
    cache, hp = sc.normalised_cache(), sc.hp3()
    replays = {b: cache.replay_names_sweep(hp, sc.THRESHOLDS, backend=b) for b in ("host", "core")}
    sweeps = {b: cache.evaluate_sweep(hp, sc.THRESHOLDS, backend=b) for b in ("host", "core")}
    hold = sc.python_holds(cache, replays["host"][0], sc.THRESHOLDS, (0, 1))
    return cache, hp, replays, sweeps, hold


@pytest.fixture(scope="module")
def raw():
    return ic.base_cache().with_gallery(ic.gallery())


def test_the_planes_are_the_float64_statement(case, raw):
    cache = case[0]
    assert cache.normalised and cache.top_ns == sc.TOP_NS and np.array_equal(cache.cohort, sc.cohort())
    assert cache.plane_index.shape == (2, 120, ic.K) and cache.plane_index.dtype == np.int32
    assert cache.plane_distance.shape == (2, 120, ic.K) and cache.plane_distance.dtype == np.float32
    for p, tn in enumerate(sc.TOP_NS):
        if __import__("torch").cuda.is_available():       # (with a GPU the stored bits are the live kernels')
            index, distance, _ = ic.gallery().with_cohort(sc.cohort(), tn).match_normalised(cache.emb)
        else:
            index, distance, _ = F.gallery_match_normalised(cache.emb, ic.gallery_rows(), sc.cohort(), tn)
        assert np.array_equal(cache.plane_index[p], index)
        assert np.array_equal(cache.plane_distance[p], distance.astype(np.float32), equal_nan=True)
        # the normalisation changes who is nearest: the raw index differs in at least 30 of the 360 rows
        assert (cache.plane_index[p] != raw.match_index).sum() >= 30
    assert np.array_equal(cache.match_index, cache.plane_index[0])
    assert np.array_equal(cache.match_distance, cache.plane_distance[0], equal_nan=True)
    assert not np.array_equal(cache.plane_index[0], cache.plane_index[1])
    lo, hi = cache.delta_range()
    finite = cache.plane_distance[np.isfinite(cache.plane_distance)]
    assert (lo, hi) == (float(finite.min()), float(finite.max())) and lo < -12 and hi > 0.5
    # a raw cache: one plane, no top_n, DeltaId's range
    assert not raw.normalised and raw.top_ns == () and raw.cohort is None and raw.plane_index.shape == (1, 120, ic.K)
    assert raw.delta_range() == (0.0, 2.0)
    # top_n=None: the gallery's own
    own = ic.base_cache().with_gallery(sc.gallery(), normalised=True)
    assert own.top_ns == (12,) and np.array_equal(own.plane_index[0], cache.plane_index[1])


@pytest.mark.parametrize("backend", ["host", "core"])
def test_names_are_the_signed_python_rule(case, backend):
    cache, hp, replays, _, hold = case
    assign, status, bits, got = replays[backend]
    assert got.dtype == np.int32 and got.shape == (16, 2, 5, 120, cache.G) and np.array_equal(got, hold)
    assert (status == -1).all()                                           # no chain of base_cache() stops
    a3, s3, b3 = TuneCache.replay(cache, hp, backend=backend)
    assert np.array_equal(a3, assign) and np.array_equal(s3, status) and np.array_equal(b3, bits)
    # conditions on the inputs: a point that names nobody, and names at the loosest
    assert (hold[:, 1, 0] < 0).all() and sc.TOP_NS[1] == 12 and sc.THRESHOLDS[0] == -12.0
    named = (hold[:, 1, 4] >= 0).mean()
    print("share of named slots at (12, 0.5)", named)
    assert named >= 0.3
    # one point of the sweep is replay_names on that plane
    one = cache.replay_names(np.concatenate([hp, np.full((16, 1), -3.0)], axis=1), backend=backend, top_n=12)
    assert np.array_equal(one[3], got[:, 1, 2])


def test_core_is_evaluate_point_by_point(case):
    cache, hp, _, sweeps, _ = case
    got = sweeps["core"]
    assert isinstance(got, SweepResult) and got.rate.shape == (16, 2, 5) and got.components.shape == (16, 2, 5, 5)
    assert got.per_file.shape == (16, 2, 5, 3, 5) and got.status.shape == (16, 3)
    assert got.top_n.tolist() == [6, 12] and got.delta_id.tolist() == list(sc.THRESHOLDS)
    rate, comp, per_file = sc.point_by_point(cache, hp, sc.THRESHOLDS, sc.TOP_NS, "core")
    assert np.array_equal(got.per_file, per_file) and np.array_equal(got.components, comp)
    assert np.array_equal(got.rate, rate) and not np.isnan(rate).any()
    # conditions on the inputs: the points differ
    assert len(np.unique(got.components[..., 1])) >= 10                    # `correct`
    assert len(np.unique(got.components[..., 4])) >= 10                    # `confusion`
    assert (got.components[:, 1, 0, 1] == 0.0).all()                       # nobody named: nothing correct
    assert ((got.rate[:, 0] != got.rate[:, 1]).any(axis=1)).sum() >= 5     # the planes matter
    # trials in batches that fit the budget: the same doubles
    assert cache.sweep_bytes_per_trial(10) == TuneCache.bytes_per_trial.fget(cache) + 10 * 120 * cache.G
    again = cache.evaluate_sweep(hp, sc.THRESHOLDS, backend="core", memory_budget=3 * cache.sweep_bytes_per_trial(10))
    assert sc.same_sweep(got, again)
    for budget in (1, 8 * cache.sweep_bytes_per_trial(10)):                # a trial per batch; slices inside a batch
        assert sc.same_sweep(got, cache.evaluate_sweep(hp, sc.THRESHOLDS, backend="core", memory_budget=budget))
    # a chosen plane, in the caller's order
    swapped = cache.evaluate_sweep(hp, sc.THRESHOLDS, top_n=(12, 6), backend="core")
    assert swapped.top_n.tolist() == [12, 6] and np.array_equal(swapped.per_file, got.per_file[:, ::-1])
    alone = cache.evaluate_sweep(hp, sc.THRESHOLDS, top_n=12, backend="core")
    assert np.array_equal(alone.per_file, got.per_file[:, 1:])


def test_host_lies_within_the_bars(case):
    _, _, _, sweeps, _ = case
    host, core = sweeps["host"], sweeps["core"]
    worst = np.abs(host.per_file - core.per_file).max(axis=(0, 1, 2, 3))
    print("largest difference per component", worst, "smallest total", core.per_file[..., 0].min())
    assert (core.per_file[..., 0] > 0).all() and (np.abs(host.per_file - core.per_file) <= ic.bars(core.per_file)).all()
    assert np.array_equal(host.status, core.status)


def test_the_sweep_is_the_identification_error_rate(case):
    cache, _, replays, sweeps, hold = case
    bits = replays["host"][2]
    for p in range(2):
        for q in range(5):
            want = ic.metric_components(cache, bits[:4], hold[:4, p, q])
            for backend in ("host", "core"):
                got = sweeps[backend].per_file[:4, p, q]
                assert (np.abs(got - want) <= ic.bars(want)).all(), (backend, p, q, np.abs(got - want).max())


@pytest.mark.parametrize("backend", ["host", "core"])
def test_a_stopped_chain_is_nan_at_every_point(backend):
    """The cohort of the stop case: np.random.default_rng(2001).standard_normal((3, 64)), planes top_n = 2 and 3."""
    cache, _, hp = sc.stop_case()
    got = cache.evaluate_sweep(hp, sc.STOP_THRESHOLDS, backend=backend)
    assert got.status[0].tolist() == [-1, 3] and (got.status[1:] < 0).all()
    assert np.isnan(got.rate[0]).all() and not np.isnan(got.rate[1:]).any() and got.rate.shape == (4, 2, 4)
    # the other trials are what they are without the stopped one beside them
    rest = cache.evaluate_sweep(hp[1:], sc.STOP_THRESHOLDS, backend=backend)
    assert np.array_equal(got.per_file[1:], rest.per_file) and np.array_equal(got.rate[1:], rest.rate)
    # the names: nothing is taken from the status chunk on, as in Python; and the metric on them
    assign, _, bits, hold = cache.replay_names_sweep(hp, sc.STOP_THRESHOLDS, backend=backend)
    want = sc.python_holds(cache, assign, sc.STOP_THRESHOLDS, (0, 1))
    assert np.array_equal(hold, want) and (hold[:, :, 0] < 0).all() and (hold[:, :, 1:] >= 0).any()
    assert (np.diff(got.rate[1:], axis=2) != 0).any(axis=(0, 1)).all()     # every threshold changes a trial's rate
    for p in range(2):
        for q in range(4):
            comp = ic.metric_components(cache, bits[1:], want[1:, p, q])
            assert (np.abs(got.per_file[1:, p, q] - comp) <= ic.bars(comp)).all()


def test_one_point_and_the_limits(case):
    cache, hp, _, _, _ = case
    for backend in ("host", "core"):
        one = cache.evaluate_sweep(hp, [-3.0], top_n=6, backend=backend)
        want = cache.evaluate(np.concatenate([hp, np.full((16, 1), -3.0)], axis=1), backend=backend, top_n=6)
        assert np.array_equal(one.per_file[:, 0, 0], want.per_file) and np.array_equal(one.rate[:, 0, 0], want.rate)
        assert np.array_equal(one.components[:, 0, 0], want.components) and np.array_equal(one.status, want.status)
    full = cache.evaluate_sweep(hp[:2], np.linspace(-12, 0.5, 128), backend="core")           # 2 x 128 = 256 points
    assert full.rate.shape == (2, 2, 128)
    assert np.array_equal(full.per_file[:, :, 0], cache.evaluate_sweep(hp[:2], [-12.0], backend="core").per_file[:, :, 0])
    with pytest.raises(ValueError, match=r"2 planes x 129 thresholds = 258 points \(1 \.\. 256\)"):
        cache.evaluate_sweep(hp[:2], np.linspace(-12, 0.5, 129), backend="core")
    with pytest.raises(ValueError, match=r"1 planes x 257 thresholds = 257 points \(1 \.\. 256\)"):
        cache.evaluate_sweep(hp[:2], np.linspace(-12, 0.5, 257), top_n=6, backend="core")
    with pytest.raises(ValueError, match=r"0 points \(1 \.\. 256\)"):
        cache.evaluate_sweep(hp[:2], [], backend="core")
    # nine planes
    nine = np.random.default_rng(5).standard_normal((12, ic.D)).astype(np.float32)
    with pytest.raises(ValueError, match=r"top_n= of 9 values \(1 \.\. 8 planes\)"):
        ic.base_cache().with_gallery(ic.gallery().with_cohort(nine, 12), normalised=True, top_n=range(1, 10))
    eight = ic.base_cache().with_gallery(ic.gallery().with_cohort(nine, 12), normalised=True, top_n=range(5, 13))
    assert eight.top_ns == tuple(range(5, 13)) and eight.evaluate_sweep(hp[:1], [-1.0], backend="core").rate.shape == (1, 8, 1)


def test_a_raw_cache_sweeps_too(raw):
    hp, thresholds = sc.hp3(), (0.0, 0.2, 0.5, 1.0, 2.0)
    for backend in ("host", "core"):
        got = raw.evaluate_sweep(hp, thresholds, backend=backend)
        assert got.rate.shape == (16, 1, 5) and got.top_n.shape == (0,)
        rate, _, per_file = sc.point_by_point(raw, hp, thresholds, None, backend)
        assert np.array_equal(got.per_file, per_file) and np.array_equal(got.rate, rate)
    with pytest.raises(ValueError, match=r"point 1: delta_id=-0\.5 \(a finite distance >= 0\)"):
        raw.evaluate_sweep(hp, (0.2, -0.5))
    with pytest.raises(ValueError, match="top_n=6 on a raw cache, which has one plane"):
        raw.evaluate_sweep(hp, (0.2,), top_n=6)
    with pytest.raises(ValueError, match=r"trial 0: delta_id=-1\.0 \(a finite distance >= 0\)"):
        raw.evaluate(np.array([[0.5, 0.3, 1.0, -1.0]]))


def test_round_trip(case, raw, tmp_path):
    cache, hp, _, sweeps, _ = case
    cache.save(tmp_path / "norm.npz")
    back = IdentTuneCache.load(tmp_path / "norm.npz")
    assert back.normalised and back.top_ns == sc.TOP_NS and np.array_equal(back.cohort, cache.cohort)
    assert np.array_equal(back.plane_index, cache.plane_index)
    assert np.array_equal(back.plane_distance, cache.plane_distance, equal_nan=True) and back.names == cache.names
    assert sc.same_sweep(back.evaluate_sweep(hp, sc.THRESHOLDS, backend="core"), sweeps["core"])
    raw.save(tmp_path / "raw.npz")
    base_keys = set(ic.base_cache()._payload())
    with np.load(tmp_path / "raw.npz") as z:
        assert set(z.files) == base_keys | {"kind", "gallery_names", "gallery_voiceprints", "match_index", "match_distance"}
    with np.load(tmp_path / "norm.npz") as z:
        assert set(z.files) == base_keys | {"kind", "gallery_names", "gallery_voiceprints", "match_index", "match_distance",
                                           "gallery_cohort", "top_ns", "plane_index", "plane_distance"}
        assert str(z["kind"]) == "IdentTuneCache"
    again = IdentTuneCache.load(tmp_path / "raw.npz")
    assert not again.normalised and again.top_ns == () and np.array_equal(again.match_index, raw.match_index)


def test_refusals(case, raw):
    cache, hp, _, _, _ = case
    base_cache, plain, withc = ic.base_cache(), ic.gallery(), sc.gallery()
    with pytest.raises(ValueError, match="TuneCache.with_gallery: the gallery has a cohort.*normalised=True"):
        base_cache.with_gallery(withc)
    with pytest.raises(ValueError, match="top_n= chooses the planes of the normalised match; it needs normalised=True"):
        base_cache.with_gallery(plain, top_n=6)
    with pytest.raises(ValueError, match=r"with_gallery\(normalised=True\): the gallery has no cohort"):
        base_cache.with_gallery(plain, normalised=True)
    with pytest.raises(ValueError, match=r"top_n=13 \(1 \.\. the cohort's 12 rows\)"):
        base_cache.with_gallery(withc, normalised=True, top_n=(6, 13))
    with pytest.raises(ValueError, match=r"top_n=0 \(1 \.\. the cohort's 12 rows\)"):
        base_cache.with_gallery(withc, normalised=True, top_n=0)
    with pytest.raises(ValueError, match=r"top_n=\[6, 6\] repeats a value"):
        base_cache.with_gallery(withc, normalised=True, top_n=(6, 6))
    with pytest.raises(ValueError, match=r"top_n= of 0 values \(1 \.\. 8 planes\)"):
        base_cache.with_gallery(withc, normalised=True, top_n=())
    # the plane of a call
    hp4 = np.concatenate([hp, np.full((16, 1), -3.0)], axis=1)
    for call in (cache.evaluate, cache.replay_names):
        with pytest.raises(ValueError, match=r"top_n=7 is no plane of this cache \(top_ns = \[6, 12\]\)"):
            call(hp4, backend="core", top_n=7)
    with pytest.raises(ValueError, match=r"top_n=7 is no plane of this cache"):
        cache.evaluate_sweep(hp, sc.THRESHOLDS, top_n=(6, 7))
    with pytest.raises(ValueError, match="top_n=6 on a raw cache"):
        raw.evaluate(np.concatenate([hp, np.full((16, 1), 0.5)], axis=1), top_n=6)
    # thresholds: any finite value on a normalised cache
    assert not np.isnan(cache.evaluate(hp4, backend="core").rate).any()
    with pytest.raises(ValueError, match=r"point 2: delta_id=nan \(a finite threshold\)"):
        cache.evaluate_sweep(hp, (-1.0, 0.0, np.nan))
    with pytest.raises(ValueError, match=r"trial 3: delta_id=inf \(a finite threshold\)"):
        cache.evaluate(np.concatenate([hp, np.where(np.arange(16) == 3, np.inf, -1.0)[:, None]], axis=1))
    with pytest.raises(ValueError, match=r"hparams \(T, 3\)"):
        cache.evaluate_sweep(hp4, sc.THRESHOLDS)
    with pytest.raises(ValueError, match="backend 'cuda': gpu, host or core"):
        cache.evaluate_sweep(hp, sc.THRESHOLDS, backend="cuda")


def test_c_entry_points_refuse_before_anything_runs(case):
    """Status 2 and the function's name from the host entries: a NULL pointer, T < 1, points outside 1 .. 256, planes
    outside 1 .. 8 or not dividing the points, G > 32."""
    cache = case[0]
    lib = _lib.load()
    last_error = lambda: lib.dz_last_error().decode()
    total, p = 120, lambda a: a.ctypes.data
    assign = np.full((1, total, 3), -1, dtype=np.int8)
    status = np.full((1, 3), -1, dtype=np.int32)
    delta = np.zeros((1, 256))
    ident = np.zeros((1, 256, total, 5), dtype=np.int8)
    bits = np.zeros((1, cache.total_rows), dtype=np.uint32)
    out = np.zeros((1, 256, 3, 5))
    bad = (dict(T=0), dict(J=0), dict(J=257), dict(P=0), dict(P=9), dict(J=10, P=3), dict(G=33), dict(ptr=None))

    def cells(G=5, max_cells=cache.max_cells):
        c = _lib.TuneCells.from_buffer_copy(cache._host_cells())
        c.max_speakers, c.max_cells = G, max_cells
        return C.byref(c)

    def name(fn, T=1, J=10, P=2, G=5, ptr=p(assign)):
        args = (T, J, P, 3, total, 3, G, 6, p(cache.chunk_off), ptr, p(status), p(cache.plane_index),
                p(cache.plane_distance), p(cache.vp_ref), p(delta), p(ident), None)
        if fn == "dz_tune_name":
            return lib.dz_tune_name(None, *args, 64, None)
        return lib.dz_tune_name_host(*args, 1)

    def score(fn, T=1, J=10, G=5, ptr=p(bits), max_cells=cache.max_cells, **_):
        if fn == "dz_tune_ident_score_gpu":
            return lib.dz_tune_ident_score_gpu(None, cells(G), T, J, ptr, p(ident), p(out), p(bits), 4, p(status), None)
        return lib.dz_tune_ident_score_core(cells(G, max_cells), T, J, ptr, p(ident), 256, 4, p(out), 1)

    assert name("dz_tune_name_host") == 0 and name("dz_tune_name_host", J=256, P=1) == 0
    assert score("dz_tune_ident_score_core") == 0 and score("dz_tune_ident_score_core", J=256) == 0
    for kw in bad:
        assert name("dz_tune_name_host", **kw) == 2 and "dz_tune_name_host" in last_error(), kw
        if "P" in kw:
            continue                                                      # (the scoring entries take no planes)
        assert score("dz_tune_ident_score_core", **kw) == 2 and "dz_tune_ident_score_core" in last_error(), kw
    # a failure while it runs names the entry too: a scratch slice smaller than a file's cells, at ten points and at one
    for points in (10, 1):
        assert score("dz_tune_ident_score_core", J=points, max_cells=1) == 2
        assert "dz_tune_ident_score_core: a file has more scoring cells" in last_error()
    # the device entries: without a GPU there is no context, and a NULL one is all that can be refused here; their other
    # refusals are held on the GPU (tests/test_gpu_tune_sweep.py), with a live context
    assert name("dz_tune_name") == 2 and "dz_tune_name: NULL argument" in last_error()
    assert score("dz_tune_ident_score_gpu") == 2 and "dz_tune_ident_score_gpu: NULL argument" in last_error()


def _optimizer(tmp_path, cache, **kw):
    kw["base_config"] = types.SimpleNamespace(**tc.config_of(*ic.OWN, ic.G, ic.LATENCY))
    kw.setdefault("gallery", sc.gallery())
    kw.setdefault("delta_id", -2.0)
    kw.setdefault("normalised", True)
    return Optimizer(SpeakerDiarization, None, None, tmp_path / "study", cache=cache, backend="host", **kw)


def test_optimizer_sweep(case, tmp_path):
    cache = case[0]
    opt = _optimizer(tmp_path, cache, seed=3, trials_per_batch=3, sweep=3)
    assert [p.name for p in opt.hparams] == ["tau_active", "rho_update", "delta_new"]
    lo, hi = cache.delta_range()
    thresholds = opt.sweep_thresholds()
    assert np.array_equal(thresholds, np.concatenate([[-2.0], np.linspace(lo, hi, 5)[1:-1]]))
    opt(8, show_progress=False)
    assert len(opt.trials) == 8 and opt.trials[0]["params"].items() >= {"tau_active": 0.5, "rho_update": 0.3,
                                                                        "delta_new": 1.0}.items()
    hp = np.array([[t["params"][k] for k in ("tau_active", "rho_update", "delta_new")] for t in opt.trials])
    sweep = cache.evaluate_sweep(hp, thresholds, backend="host")
    flat = sweep.rate.reshape(8, -1)
    assert not np.isnan(flat).any()
    for t, row in zip(opt.trials, flat):
        j = int(np.argmin(row))                                            # (the first among equals)
        assert t["value"] == 100.0 * row.min()
        assert t["params"]["delta_id"] == thresholds[j % 4] and t["params"]["top_n"] == sc.TOP_NS[j // 4]
        assert list(t["params"]) == ["tau_active", "rho_update", "delta_new", "delta_id", "top_n"]
    assert opt.best_performance == 100.0 * flat.min() and {"delta_id", "top_n"} <= set(opt.best_hparams)
    stored = json.loads((tmp_path / "study" / "study.json").read_text())
    assert (stored["sweep"], stored["top_n"], stored["normalised"]) == (3, [6, 12], True)   # the cache's planes
    # a second call continues the study: the numbering, the sequence, no stored trial again (the kick-start among them)
    again = _optimizer(tmp_path, cache, seed=3, trials_per_batch=3, sweep=3)
    assert again.trials == opt.trials
    again(3, show_progress=False)
    assert [t["number"] for t in again.trials] == list(range(11)) and again.trials[:8] == opt.trials
    fresh = _optimizer(tmp_path / "fresh", cache, seed=3, sweep=3)
    fresh(11, show_progress=False)
    assert [t["params"] for t in fresh.trials] == [t["params"] for t in again.trials]
    # a changed sweep, plane set or kind of match is refused by name
    with pytest.raises(ValueError, match="holds a study with sweep=3, not sweep=4"):
        _optimizer(tmp_path, cache, seed=3, sweep=4)
    assert _optimizer(tmp_path, cache, seed=3, sweep=3, top_n=(6, 12)).trials == again.trials      # the same planes, named
    with pytest.raises(ValueError, match=r"holds a study with top_n=\[6, 12\], not top_n=\[6\]"):
        _optimizer(tmp_path, ic.base_cache(), seed=3, sweep=3, top_n=6)
    with pytest.raises(ValueError, match=r"holds a study with top_n=\[6, 12\], not top_n=\[12\]"):
        _optimizer(tmp_path, ic.base_cache(), seed=3, sweep=3)              # (the gallery's own top_n)
    # one plane: no top_n among the stored parameters
    single = _optimizer(tmp_path / "single", ic.base_cache(), seed=3, sweep=2, top_n=6)
    single(3, show_progress=False)
    assert json.loads((tmp_path / "single" / "study" / "study.json").read_text())["top_n"] == [6]
    assert single.cache.top_ns == (6,) and all("top_n" not in t["params"] and "delta_id" in t["params"] for t in single.trials)


def test_optimizer_normalised_without_a_sweep(case, raw, tmp_path):
    cache = case[0]
    opt = _optimizer(tmp_path, ic.base_cache(), seed=3, top_n=12)
    opt(12, show_progress=False)
    assert opt.cache.normalised and opt.cache.top_ns == (12,) and opt.hparams[3] is base.DeltaId
    lo, hi = opt.cache.delta_range()
    sampled = np.array([t["params"]["delta_id"] for t in opt.trials[1:]])
    assert opt.trials[0]["params"]["delta_id"] == -2.0 and (sampled >= lo).all() and (sampled <= hi).all()
    assert (sampled < 0).any() and lo < -5                                # not DeltaId's (0, 2)
    hp = np.array([opt._values(t["params"]) for t in opt.trials])
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * opt.cache.evaluate(hp, backend="host").rate)
    assert json.loads((tmp_path / "study" / "study.json").read_text())["normalised"] is True
    # a range of the caller's is taken as given
    own = _optimizer(tmp_path / "own", opt.cache, seed=3, hparams=[base.TauActive, base.HyperParameter("delta_id", -4.0, -3.0)])
    own(6, show_progress=False)
    assert all(-4.0 <= t["params"]["delta_id"] <= -3.0 for t in own.trials[1:])
    # a raw study writes the keys it always wrote
    plain = _optimizer(tmp_path / "plain", raw, seed=3, gallery=ic.gallery(), delta_id=0.4, normalised=False)
    plain(2, show_progress=False)
    assert set(json.loads((tmp_path / "plain" / "study" / "study.json").read_text())) == {"direction", "hparams", "trials"}


def test_optimizer_refusals(case, raw, tmp_path):
    cache = case[0]
    with pytest.raises(ValueError, match=r"hyper-parameter delta_id \(DeltaId\) with sweep=3: the sweep covers delta_id"):
        _optimizer(tmp_path, cache, sweep=3, hparams=[base.TauActive, base.DeltaId])
    with pytest.raises(ValueError, match="sweep=0: the number of thresholds per trial, an integer of at least 1"):
        _optimizer(tmp_path, cache, sweep=0)
    with pytest.raises(ValueError, match="this IdentTuneCache holds the raw match, and normalised=True"):
        _optimizer(tmp_path, raw, sweep=3)
    with pytest.raises(ValueError, match="this IdentTuneCache holds the normalised match, and normalised=False"):
        _optimizer(tmp_path, cache, normalised=False, delta_id=0.4)
    with pytest.raises(ValueError, match=r"holds the planes top_ns = \[6, 12\], and top_n=\[12\]"):
        _optimizer(tmp_path, cache, top_n=12)
    with pytest.raises(ValueError, match="normalised=True: gallery= has no cohort"):
        _optimizer(tmp_path, ic.base_cache(), gallery=ic.gallery())
    with pytest.raises(ValueError, match=r"top_n=\[6, 12\]: a trial without sweep= is scored on one plane"):
        _optimizer(tmp_path, ic.base_cache(), top_n=(6, 12))
    with pytest.raises(ValueError, match=r"top_n=\[6, 12\]: a trial without sweep= is scored on one plane"):
        _optimizer(tmp_path, cache)                                        # the planes of the cache count, named or not
    with pytest.raises(ValueError, match="top_n= chooses the planes of the normalised match; it needs normalised=True"):
        _optimizer(tmp_path, ic.base_cache(), normalised=False, top_n=6, delta_id=0.4)
    with pytest.raises(ValueError, match="a finite distance"):
        _optimizer(tmp_path, raw, gallery=ic.gallery(), normalised=False, delta_id=-2.0)
    cfg = types.SimpleNamespace(**tc.config_of(*ic.OWN, ic.G, ic.LATENCY))
    for kw, name in ((dict(normalised=True), "normalised"), (dict(top_n=6), "top_n"), (dict(sweep=3), "sweep")):
        with pytest.raises(ValueError, match=f"{name}= is about the match against gallery=, which is not given"):
            Optimizer(SpeakerDiarization, None, None, tmp_path / "s", base_config=cfg, cache=ic.base_cache(), **kw)
    assert not (tmp_path / "study").exists()


def test_command_line_arguments():
    from diart_amd import tune
    args = tune.parser().parse_args(["audio", "--reference", "rttm", "--output", "study", "--gallery", "g.npz", "--delta-id",
                                     "-2", "--normalised", "--top-n", "100", "300", "--sweep", "16"])
    assert args.normalised is True and args.top_n == [100, 300] and args.sweep == 16 and args.delta_id == -2.0
    plain = tune.parser().parse_args(["audio", "--reference", "rttm", "--output", "study"])
    assert plain.normalised is False and plain.top_n is None and plain.sweep is None
    plain.sweep = 4
    with pytest.raises(SystemExit, match="--normalised, --top-n and --sweep are about the match against --gallery"):
        tune.run(plain, models=(None, None))


def test_the_optimizer_collects_a_normalised_cache(monkeypatch, tmp_path):
    """Without cache=, the Optimizer collects its own: the match it asks for is the constructor's."""
    calls = []

    def collect(cls, pipeline_class, base_config, speech_path, reference_path, batch_size=32):
        calls.append((speech_path, reference_path))
        return ic.base_cache()

    monkeypatch.setattr(TuneCache, "collect", classmethod(collect))
    opt = _optimizer(tmp_path, None, seed=3, top_n=(6, 12), sweep=2)
    assert isinstance(opt.cache, IdentTuneCache) and opt.cache.normalised and opt.cache.top_ns == (6, 12) and len(calls) == 1
    opt(3, show_progress=False)
    assert len(calls) == 1 and all("top_n" in t["params"] for t in opt.trials)
    own = _optimizer(tmp_path / "own", None, seed=3)
    assert own.cache.normalised and own.cache.top_ns == (12,)              # the gallery's own top_n
    plain = _optimizer(tmp_path / "plain", None, seed=3, gallery=ic.gallery(), delta_id=0.4, normalised=False)
    assert not plain.cache.normalised and plain.cache.top_ns == ()


def test_command_line_end_to_end(case, monkeypatch, tmp_path):
    """python -m diart_amd.tune --gallery ... --normalised --top-n ... --sweep Q: first with nothing collected (the
    models' pass is stubbed by the case's outputs, and --cache is written), then again from the file it wrote."""
    from diart_amd import models as M
    from diart_amd import tune
    from tune_cases import scenarios
    monkeypatch.setattr(TuneCache, "collect", classmethod(lambda cls, *a, **kw: ic.base_cache()))
    sc.gallery().save(tmp_path / "staff.npz")
    models = (M.SegmentationModel(lambda: scenarios.ToySegmentation()), M.EmbeddingModel(lambda: scenarios.ToyEmbedding()))
    common = [str(tmp_path), "--reference", str(tmp_path), "--num-iter", "4", "--seed", "2", "--trials-per-batch", "3",
              "--latency", str(ic.LATENCY), "--max-speakers", str(ic.G), "--cpu", "--gallery", str(tmp_path / "staff.npz"),
              "--delta-id", "-2", "--normalised"]
    argv = common + ["--cache", str(tmp_path / "cache.npz"), "--output", str(tmp_path / "study"), "--top-n", "6", "12",
                     "--sweep", "3"]
    opt = tune.run(tune.parser().parse_args(argv), models=models)
    assert (tmp_path / "cache.npz").exists() and opt.cache.top_ns == (6, 12) and len(opt.trials) == 4
    assert all(list(t["params"]) == ["tau_active", "rho_update", "delta_new", "delta_id", "top_n"] for t in opt.trials)
    assert np.array_equal(opt.cache.plane_index, case[0].plane_index)
    monkeypatch.undo()                                                     # from here nothing may collect
    again = tune.run(tune.parser().parse_args(argv), models=models)        # the cache file is loaded, the study continues
    assert again.trials[:4] == opt.trials and len(again.trials) == 8 and again.cache.top_ns == (6, 12)
    # delta_id sampled on one plane, no cache file
    monkeypatch.setattr(TuneCache, "collect", classmethod(lambda cls, *a, **kw: ic.base_cache()))
    one = tune.run(tune.parser().parse_args(common + ["--output", str(tmp_path / "one"), "--top-n", "6"]), models=models)
    assert one.cache.top_ns == (6,) and list(one.best_hparams) == ["tau_active", "rho_update", "delta_new", "delta_id"]
    assert any(t["params"]["delta_id"] < -2.5 for t in one.trials)
    with pytest.raises(SystemExit, match="--sweep covers delta_id at every trial"):
        tune.run(tune.parser().parse_args(argv + ["--hparams", "tau_active", "delta_id"]), models=models)
