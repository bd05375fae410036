"""Tuning delta_id by replay, without a GPU: IdentTuneCache's names on backend "host" and "core" against
gallery.SpeakerNames in Python, its components against metrics.IdentificationErrorRate on the named hypothesis, the
metric on a hand-made example, the file format, the refusals, Optimizer and the command line.  The cases are
tests/tune_ident_cases.py's."""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_ident_cases as ic  # noqa: E402
from tune_cases import scenarios  # noqa: E402

from diart_amd import _lib  # noqa: E402
from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization  # noqa: E402
from diart_amd.features import Annotation, Segment  # noqa: E402
from diart_amd.gallery import SpeakerGallery  # noqa: E402
from diart_amd.metrics import COMPONENTS, DiarizationErrorRate, IdentificationErrorRate  # noqa: E402
from diart_amd.optim import IdentTuneCache, Optimizer, OsdTuneCache, TuneCache, VadTuneCache  # noqa: E402


@pytest.fixture(scope="module")
def case():
    """(cache, hparams (16, 4), {backend: replay_names}, python hold (16, chunks, G)); computed once, never changed."""
    cache, hp = ic.base_cache().with_gallery(ic.gallery()), ic.trials()
    replays = {b: cache.replay_names(hp, backend=b) for b in ("host", "core")}
    assign = replays["host"][0]
    hold = np.stack([ic.python_hold(cache, assign[t], hp[t, 3]) for t in range(hp.shape[0])])
    return cache, hp, replays, hold


@pytest.fixture(scope="module")
def stop():
    cache, gallery, hp = ic.stop_cache()
    return cache.with_gallery(gallery), hp


def test_the_cases_reach_every_branch_of_the_rule(case, stop):
    cache, hp, _, hold = case
    assert cache.sorted_steps and hp.shape == (16, 4) and cache.match_index.shape == (120, 3)
    assert cache.vp_ref.tolist() == [[0, 1, -1, -1, -1, -1]] * 3          # ref0, ref1 enrolled; ref2 is not
    assert (cache.match_index < 0).any() and np.isnan(cache.match_distance[cache.match_index < 0]).all()
    from diart_amd.gallery import SpeakerNames
    assign = case[2]["host"][0]
    losers = 0          # (trial, step) at which two global speakers hold the same voiceprint: the loser reads speaker{g}
    for t in range(hp.shape[0]):
        for n in range(cache.N):
            rule = SpeakerNames(1, cache.G, hp[t, 3])
            for c in range(int(cache.chunk_off[n]), int(cache.chunk_off[n + 1])):
                rule.update(assign[t][c][None], cache.match_index[c][None], cache.match_distance[c][None])
                e = rule.best_e[0][rule.best_e[0] >= 0]
                if len(set(e.tolist())) < e.shape[0]:
                    losers += 1
                    assert ((rule.best_e[0] >= 0) & (hold[t, c] < 0)).any()
    assert losers >= 1
    changes = sum(len(set(h[h >= 0].tolist())) > 1 for t in range(16) for n in range(cache.N) for h in
                  hold[t, int(cache.chunk_off[n]):int(cache.chunk_off[n + 1])].T)
    assert changes >= 1                                                   # a g changes its name over time
    assert (hold[0] < 0).all() and hp[0, 3] == 0.0                        # delta_id = 0 names nothing
    assert (hold[1:] >= 0).any()
    status = stop[0].replay_names(stop[1], backend="host")[1]
    assert status.tolist()[0] == [-1, 3] and (status[1:] < 0).all()       # a chain that stops early


@pytest.mark.parametrize("backend", ["host", "core"])
def test_names_are_the_python_rule(case, stop, backend):
    cache, hp, replays, hold = case
    assign, status, bits, got = replays[backend]
    assert got.dtype == np.int32 and got.shape == (16, 120, cache.G) and np.array_equal(got, hold)
    assert np.array_equal(assign, replays["host"][0]) and np.array_equal(bits, replays["host"][2])
    # the three other outputs are TuneCache.replay's
    a3, s3, b3 = TuneCache.replay(cache, hp[:, :3], backend=backend)
    assert np.array_equal(a3, assign) and np.array_equal(s3, status) and np.array_equal(b3, bits)
    # a chain that stopped: nothing is taken from its status chunk on
    scache, shp = stop
    sa, _, _, sgot = scache.replay_names(shp, backend=backend)
    assert np.array_equal(sgot, np.stack([ic.python_hold(scache, sa[t], shp[t, 3]) for t in range(shp.shape[0])]))


@pytest.mark.parametrize("backend", ["host", "core"])
def test_evaluate_is_the_identification_error_rate(case, stop, backend):
    cache, hp, replays, hold = case
    result = cache.evaluate(hp, backend=backend)
    want = ic.metric_components(cache, replays["host"][2], hold)
    worst = np.abs(result.per_file - want).max(axis=(0, 1))
    print(backend, "largest difference per component", worst, "smallest total", want[..., 0].min())
    assert (want[..., 0] > 0).all() and (np.abs(result.per_file - want) <= ic.bars(want)).all(), worst
    assert (want.sum(axis=(0, 1)) > 0).all()                              # every component occurs
    assert np.array_equal(result.components, result.per_file.sum(axis=1)) and (result.status == -1).all()
    comp = result.components
    assert np.array_equal(result.rate, (comp[:, 2] + comp[:, 3] + comp[:, 4]) / comp[:, 0])
    # delta_id = 0: nobody is named, so nothing is correct
    assert result.components[0, 1] == 0.0
    # trials in batches that fit the memory budget: the same doubles
    assert cache.bytes_per_trial == TuneCache.bytes_per_trial.fget(cache) + 120 * cache.G
    again = cache.evaluate(hp, backend=backend, memory_budget=3 * cache.bytes_per_trial)
    assert np.array_equal(result.per_file, again.per_file)
    # a stopped chain: NaN for its trial alone; the other trials against the metric
    scache, shp = stop
    sres = scache.evaluate(shp, backend=backend)
    assert np.isnan(sres.rate).tolist() == [True, False, False, False] and sres.status[0].tolist() == [-1, 3]
    _, _, sbits, shold = scache.replay_names(shp, backend="host")
    swant = ic.metric_components(scache, sbits[1:], shold[1:])
    assert (np.abs(sres.per_file[1:] - swant) <= ic.bars(swant)).all()


def test_the_diarization_tuner_is_untouched(case):
    cache, hp, _, _ = case
    base_cache = ic.base_cache()
    before = base_cache.evaluate(hp[:, :3], backend="host")
    named = base_cache.with_gallery(ic.gallery())
    after = base_cache.evaluate(hp[:, :3], backend="host")
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    assert named.files is base_cache.files and named.plan is base_cache.plan and named.emb is base_cache.emb


def test_metric_by_hand():
    """reference: alice [0, 4), bob [2, 6).  hypothesis: alice [0, 3) and [5, 6), speaker1 [1, 3), bob [7, 8).
        [0, 1)  R {alice}       H {alice}            total 1  correct 1
        [1, 2)  R {alice}       H {alice, speaker1}  total 1  correct 1  false alarm 1
        [2, 3)  R {alice, bob}  H {alice, speaker1}  total 2  correct 1  confusion 1
        [3, 4)  R {alice, bob}  H {}                 total 2  missed 2
        [4, 5)  R {bob}         H {}                 total 1  missed 1
        [5, 6)  R {bob}         H {alice}            total 1  confusion 1
        [7, 8)  R {}            H {bob}              false alarm 1
    total 8, correct 3, false alarm 2, missed detection 3, confusion 2: rate 7 / 8.  The DER of the same pair maps
    speaker1 -> bob and is lower: the identification error rate maps nothing."""
    ref, hyp = Annotation(uri="hand"), Annotation(uri="hand")
    ref[Segment(0, 4), 0], ref[Segment(2, 6), 1] = "alice", "bob"
    hyp[Segment(0, 3), 0], hyp[Segment(5, 6), 1], hyp[Segment(1, 3), 2], hyp[Segment(7, 8), 3] = "alice", "alice", "speaker1", "bob"
    metric = IdentificationErrorRate()
    got = metric(ref, hyp, detailed=True)
    assert [got[c] for c in COMPONENTS] == [8.0, 3.0, 2.0, 3.0, 2.0] and got["identification error rate"] == 7 / 8
    assert abs(metric) == 7 / 8 and metric.name == "identification error rate"
    assert DiarizationErrorRate()(ref, hyp) < 7 / 8
    with pytest.raises(NotImplementedError):
        IdentificationErrorRate(collar=0.25)
    with pytest.raises(NotImplementedError):
        IdentificationErrorRate(skip_overlap=True)


def test_round_trip_and_the_four_loaders(case, tmp_path):
    cache, hp, _, _ = case
    cache.save(tmp_path / "ident.npz")
    again = IdentTuneCache.load(tmp_path / "ident.npz")
    assert again.names == cache.names and np.array_equal(again.voiceprints, cache.voiceprints)
    assert np.array_equal(again.match_index, cache.match_index)
    assert np.array_equal(again.match_distance, cache.match_distance, equal_nan=True)
    assert np.array_equal(again.vp_ref, cache.vp_ref) and np.array_equal(again.cell_step, cache.cell_step)
    a, b = cache.evaluate(hp[:5], backend="host"), again.evaluate(hp[:5], backend="host")
    assert np.array_equal(a.per_file, b.per_file)
    # the stored match is what is read, whatever the gallery would say now
    with np.load(tmp_path / "ident.npz") as z:
        stored = dict(z)
    stored["match_distance"] = stored["match_distance"] + np.float32(0.25)
    np.savez(tmp_path / "moved.npz", **stored)
    moved = IdentTuneCache.load(tmp_path / "moved.npz")
    assert np.array_equal(moved.match_distance, stored["match_distance"], equal_nan=True)
    # each loader refuses the others' files
    plain = ic.base_cache()
    plain.save(tmp_path / "dia.npz")
    VadTuneCache.from_tune_cache(plain).save(tmp_path / "vad.npz")
    OsdTuneCache.from_tune_cache(plain).save(tmp_path / "osd.npz")
    for loader, own in ((TuneCache, "dia"), (VadTuneCache, "vad"), (OsdTuneCache, "osd"), (IdentTuneCache, "ident")):
        for other in ("dia", "vad", "osd", "ident"):
            if other == own:
                loader.load(tmp_path / f"{other}.npz")
            else:
                with pytest.raises(ValueError, match="holds a"):
                    loader.load(tmp_path / f"{other}.npz")
    with pytest.raises(ValueError, match="holds a IdentTuneCache, not a TuneCache"):
        TuneCache.load(tmp_path / "ident.npz")
    with pytest.raises(ValueError, match=r"holds a TuneCache \(SpeakerDiarization\), not an IdentTuneCache"):
        IdentTuneCache.load(tmp_path / "dia.npz")
    with pytest.raises(ValueError, match="holds a VadTuneCache, not an IdentTuneCache"):
        IdentTuneCache.load(tmp_path / "vad.npz")


def test_refusals(case):
    cache, hp, _, _ = case
    plain = ic.base_cache()
    with pytest.raises(ValueError, match="gallery of dimension 128 against cached embeddings of dimension 64"):
        plain.with_gallery(SpeakerGallery(["a"], np.ones((1, 128), dtype=np.float32)))
    files = [tc.file_of(*ic.outputs(11), uri="reserved")]
    files[0]["reference"] = files[0]["reference"] + [(1.0, 2.0, "speaker12")]
    with pytest.raises(ValueError, match="reference label 'speaker12' is what an unnamed speaker is called"):
        TuneCache.from_arrays(files, tc.config_of(*ic.OWN, ic.G, ic.LATENCY)).with_gallery(ic.gallery())
    with pytest.raises(ValueError, match=r"hparams \(T, 4\)"):
        cache.evaluate(hp[:, :3], backend="host")
    for bad in (np.nan, np.inf, -0.1):
        rows = hp[:4].copy()
        rows[2, 3] = bad
        with pytest.raises(ValueError, match="trial 2: delta_id"):
            cache.evaluate(rows, backend="host")
        with pytest.raises(ValueError, match="trial 2: delta_id"):
            cache.replay_names(rows, backend="core")
    with pytest.raises(ValueError, match="backend 'tpu'"):
        cache.evaluate(hp, backend="tpu")
    # a cache whose steps are not sorted by time is refused by name on every backend
    unsorted = ic.base_cache().with_gallery(ic.gallery())
    unsorted.sorted_steps = False
    for backend in ("host", "core", "gpu"):
        with pytest.raises(ValueError, match="IdentTuneCache.*not sorted by time"):
            unsorted.evaluate(hp, backend=backend)
    with pytest.raises(ValueError, match="not sorted by time"):
        unsorted.hypothesis(np.zeros(unsorted.total_rows, dtype=np.uint32), np.zeros((120, ic.G), dtype=np.int32), 0)


def test_c_entry_points_refuse_before_anything_runs(case):
    """Status 2 and a message that names the function: a NULL pointer, T < 1, G > 32, V < 1 — the GPU entry points
    before a context is looked at (there is none here: ctx is NULL too, the checks that follow never run)."""
    cache, _, _, _ = case
    lib = _lib.load()
    last_error = lambda: lib.dz_last_error().decode()
    total, p = 120, lambda a: a.ctypes.data
    assign = np.full((1, total, 3), -1, dtype=np.int8)
    status = np.full((1, 3), -1, dtype=np.int32)
    delta = np.array([0.5])
    ident = np.zeros((1, total, 33), dtype=np.int8)
    bits = np.zeros((1, cache.total_rows), dtype=np.uint32)
    out = np.zeros((1, 3, 5))

    def cells(G):
        c = _lib.TuneCells.from_buffer_copy(cache._host_cells())
        c.max_speakers = G
        return C.byref(c)

    def name_host(T=1, G=5, V=6, assign_ptr=p(assign)):                  # one point: points = planes = 1
        return lib.dz_tune_name_host(T, 1, 1, 3, total, 3, G, V, p(cache.chunk_off), assign_ptr, p(status),
                                     p(cache.match_index), p(cache.match_distance), p(cache.vp_ref), p(delta), p(ident), None, 1)

    assert name_host() == 0                                              # (hold may be NULL)
    for kw in (dict(T=0), dict(G=33), dict(V=0), dict(assign_ptr=None)):
        assert name_host(**kw) == 2 and "dz_tune_name_host" in last_error(), kw

    def score(fn, T=1, G=5, bits_ptr=p(bits)):
        if fn == "dz_tune_ident_score":
            return lib.dz_tune_ident_score(cells(G), T, bits_ptr, p(ident), p(out), 1)
        return lib.dz_tune_ident_score_core(cells(G), T, 1, bits_ptr, p(ident), 256, 4, p(out), 1)

    for fn in ("dz_tune_ident_score", "dz_tune_ident_score_core"):
        assert score(fn) == 0
        for kw in (dict(T=0), dict(G=33), dict(bits_ptr=None)):
            assert score(fn, **kw) == 2 and fn in last_error(), (fn, kw)
    # the device entry points: every pointer here is host memory or NULL, so they must refuse before touching it
    for kw in (dict(T=0), dict(G=33), dict(V=0), dict(T=1)):
        T, G, V = kw.get("T", 1), kw.get("G", 5), kw.get("V", 6)
        rc = lib.dz_tune_name(None, T, 1, 1, 3, total, 3, G, V, p(cache.chunk_off), p(assign), p(status), p(cache.match_index),
                              p(cache.match_distance), p(cache.vp_ref), p(delta), p(ident), None, 64, None)
        assert rc == 2 and "dz_tune_name" in last_error(), kw
    rc = lib.dz_tune_ident_score_gpu(None, cells(5), 1, 1, p(bits), p(ident), p(out), None, 4, None, None)
    assert rc == 2 and "dz_tune_ident_score_gpu" in last_error()


def _optimizer(tmp_path, cache, **kw):
    kw.setdefault("base_config", tc.config_of(*ic.OWN, ic.G, ic.LATENCY))
    kw["base_config"] = __import__("types").SimpleNamespace(**kw["base_config"])
    kw.setdefault("gallery", ic.gallery())
    kw.setdefault("delta_id", 0.4)
    return Optimizer(SpeakerDiarization, None, None, tmp_path / "study", cache=cache, backend="host", **kw)


def test_optimizer(case, tmp_path):
    cache, _, _, _ = case
    opt = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4, metric=IdentificationErrorRate())
    assert [p.name for p in opt.hparams] == ["tau_active", "rho_update", "delta_new", "delta_id"]
    assert opt.hparams[3] is base.DeltaId and (base.DeltaId.low, base.DeltaId.high) == (0, 2)
    assert base.HyperParameter.from_name("delta_id") is base.DeltaId
    opt(9, show_progress=False)
    assert opt.trials[0]["params"] == {"tau_active": 0.5, "rho_update": 0.3, "delta_new": 1.0, "delta_id": 0.4}
    assert all(0 <= t["params"]["delta_id"] <= 2 for t in opt.trials) and len(opt.trials) == 9
    hp = np.array([opt._values(t["params"]) for t in opt.trials])
    assert hp.shape == (9, 4)
    rates = cache.evaluate(hp, backend="host").rate
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * rates)
    best = int(np.argmin(rates))
    assert opt.best_hparams == opt.trials[best]["params"] and "delta_id" in opt.best_hparams
    # a resumed study continues the numbering and the sequence
    again = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4)
    assert again.trials == opt.trials
    again(3, show_progress=False)
    assert [t["number"] for t in again.trials] == list(range(12)) and again.trials[:9] == opt.trials
    fresh = _optimizer(tmp_path / "fresh", cache, seed=3)
    fresh(12, show_progress=False)
    assert [t["params"] for t in fresh.trials] == [t["params"] for t in again.trials]
    assert json.loads((tmp_path / "study" / "study.json").read_text())["hparams"][-1] == "delta_id"
    # delta_id not tuned: every trial uses the given value
    fixed = _optimizer(tmp_path / "fixed", cache, seed=3, hparams=[base.TauActive, base.DeltaNew], delta_id=0.7)
    fixed(5, show_progress=False)
    assert all(list(t["params"]) == ["tau_active", "delta_new"] for t in fixed.trials)
    fhp = np.array([fixed._values(t["params"]) for t in fixed.trials])
    assert (fhp[:, 3] == 0.7).all() and (fhp[:, 1] == 0.3).all()
    assert np.array_equal(np.array([t["value"] for t in fixed.trials]), 100.0 * cache.evaluate(fhp, backend="host").rate)
    # a plain TuneCache is matched against the gallery on first use
    built = _optimizer(tmp_path / "built", ic.base_cache(), seed=3)
    assert isinstance(built.cache, IdentTuneCache) and np.array_equal(built.cache.match_index, cache.match_index)


def test_optimizer_refusals(case, tmp_path):
    cache, _, _, _ = case
    from diart_amd.blocks.vad import VoiceActivityDetection
    cfg = __import__("types").SimpleNamespace(**tc.config_of(*ic.OWN, ic.G, ic.LATENCY))
    with pytest.raises(ValueError, match="gallery=: VoiceActivityDetection"):
        Optimizer(VoiceActivityDetection, None, None, tmp_path / "s", base_config=cfg, gallery=ic.gallery(), delta_id=0.4)
    with pytest.raises(ValueError, match="delta_id=None.*there is no default"):
        _optimizer(tmp_path, cache, delta_id=None)
    with pytest.raises(ValueError, match="delta_id=-1"):
        _optimizer(tmp_path, cache, delta_id=-1)
    with pytest.raises(ValueError, match="IdentificationErrorRate.*needs gallery="):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "s", base_config=cfg, cache=ic.base_cache(),
                  metric=IdentificationErrorRate())
    with pytest.raises(ValueError, match="DiarizationErrorRate.*with a gallery.*IdentificationErrorRate"):
        _optimizer(tmp_path, cache, metric=DiarizationErrorRate())
    with pytest.raises(ValueError, match="scoring: with gallery="):
        _optimizer(tmp_path, cache, scoring="device")
    with pytest.raises(ValueError, match="delta_id= is the identification distance of gallery="):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "s", base_config=cfg, cache=ic.base_cache(), delta_id=0.4)
    with pytest.raises(ValueError, match="hyper-parameter delta_id.*gallery="):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "s", base_config=cfg, cache=ic.base_cache(),
                  hparams=[base.DeltaId])
    with pytest.raises(ValueError, match="an IdentTuneCache is tuned with gallery="):
        Optimizer(SpeakerDiarization, None, None, tmp_path / "s", base_config=cfg, cache=cache)
    with pytest.raises(ValueError, match="another gallery"):
        _optimizer(tmp_path, cache, gallery=SpeakerGallery(["x"], np.ones((1, 64), dtype=np.float32)))
    # a stored study of other hyper-parameters
    _optimizer(tmp_path / "three", cache, hparams=[base.TauActive, base.RhoUpdate, base.DeltaNew])(2, show_progress=False)
    with pytest.raises(ValueError, match=r"study of \['tau_active', 'rho_update', 'delta_new'\].*not of .*'delta_id'"):
        _optimizer(tmp_path / "three", cache)


def test_command_line(case, tmp_path):
    import diart_amd
    from diart_amd import tune
    assert diart_amd.IdentTuneCache is IdentTuneCache
    cache, _, _, _ = case
    cache.save(tmp_path / "cache.npz")
    ic.gallery().save(tmp_path / "staff.npz")
    common = [str(tmp_path), "--reference", str(tmp_path), "--num-iter", "6", "--seed", "2", "--trials-per-batch", "4",
              "--cache", str(tmp_path / "cache.npz"), "--latency", str(ic.LATENCY), "--max-speakers", str(ic.G), "--cpu"]
    models = (M.SegmentationModel(lambda: scenarios.ToySegmentation()), M.EmbeddingModel(lambda: scenarios.ToyEmbedding()))
    args = tune.parser().parse_args(common + ["--output", str(tmp_path / "study"), "--gallery", str(tmp_path / "staff.npz"),
                                              "--delta-id", "0.4", "--hparams", "delta_new", "delta_id"])
    opt = tune.run(args, models=models)
    assert len(opt.trials) == 6 and all(list(t["params"]) == ["delta_new", "delta_id"] for t in opt.trials)
    assert opt.trials[0]["params"] == {"delta_new": 1.0, "delta_id": 0.4}
    args = tune.parser().parse_args(common + ["--output", str(tmp_path / "all"), "--gallery", str(tmp_path / "staff.npz"),
                                              "--delta-id", "0.4"])
    assert list(tune.run(args, models=models).best_hparams) == ["tau_active", "rho_update", "delta_new", "delta_id"]
    for extra, message in ((["--gallery", str(tmp_path / "staff.npz")], "go together"), (["--delta-id", "0.4"], "go together"),
                           (["--gallery", str(tmp_path / "staff.npz"), "--delta-id", "0.4", "--pipeline",
                             "VoiceActivityDetection"], "has none")):
        with pytest.raises(SystemExit, match=message):
            tune.run(tune.parser().parse_args(common + ["--output", str(tmp_path / "bad")] + extra), models=models)
