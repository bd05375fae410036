"""The hyper-parameter tuner without a GPU (diart_amd/optim.py, csrc/tune_score.cpp, csrc/tune_core.h): the host replay
against the existing Python path, dz_tune_score against metrics.DiarizationErrorRate, the Optimizer's bookkeeping, and the
text the GPU kernels are compiled from (run on the host) against dz_clu_step / dz_tail_step.  Synthetic inputs only."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
from tune_cases import scenarios  # noqa: E402

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import base  # noqa: E402
from diart_amd.blocks.clustering import OnlineSpeakerClustering  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.features import Annotation, Segment, SlidingWindow, SlidingWindowFeature  # noqa: E402
from diart_amd.inference import PredictionAccumulator  # noqa: E402
from diart_amd.metrics import COMPONENTS, DiarizationErrorRate  # noqa: E402
from diart_amd.optim import Optimizer, TuneCache, trial_config  # noqa: E402

F, K, D, G = 32, 3, 24, 20
SR = 16                      # the chunks only carry their time axis: 80 samples of 5 s
BATCH = 7                    # finalise computes the frame resolution from the first chunk of every batch


def _config(latency, tau=0.6, rho=0.3, delta=1.0, max_speakers=G):
    return SpeakerDiarizationConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                    embedding=M.EmbeddingModel(lambda: scenarios.ToyEmbedding()), latency=latency,
                                    tau_active=tau, rho_update=rho, delta_new=delta, max_speakers=max_speakers,
                                    device=torch.device("cpu"))


def _chunks(starts):
    return [SlidingWindowFeature(np.zeros((int(tc.DURATION * SR), 1), dtype=np.float32),
                                 SlidingWindow(start=float(s), duration=1.0 / SR, step=1.0 / SR)) for s in starts]


def _resolutions(chunks, frames):
    res = []
    for i in range(0, len(chunks), BATCH):
        res += [chunks[i].extent.duration / frames] * len(chunks[i:i + BATCH])
    return np.array(res)


def _files(shifts=(0.0, -1.75)):
    files = []
    for n, (count, shift) in enumerate(zip((60, 23), shifts)):
        seg, emb = tc.random_outputs(40 + n, count, F, K, D)
        f = tc.file_of(seg, emb, shift=shift, uri=f"file{n}")
        f["res"] = _resolutions(_chunks(f["starts"]), F)
        files.append(f)
    return files


def _python_path(f, config):
    """The existing path: SpeakerDiarization.finalise on the cached arrays, batch by batch, then PredictionAccumulator."""
    dia = SpeakerDiarization(config)
    dia.set_timestamp_shift(f["shift"])
    acc = PredictionAccumulator(f["uri"])
    chunks = _chunks(f["starts"])
    for i in range(0, len(chunks), BATCH):
        for out in dia.finalise(chunks[i:i + BATCH], torch.from_numpy(f["seg"][i:i + BATCH]),
                                torch.from_numpy(f["emb"][i:i + BATCH])):
            acc.on_next(out)
    return acc.get_prediction()


def _table(ann):
    return sorted((seg.start, seg.end, str(label)) for seg, _, label in ann.support().itertracks(yield_label=True))


def _reference(f):
    ann = Annotation(uri=f["uri"])
    for n, (s, e, label) in enumerate(f["reference"]):
        ann[Segment(s, e), n] = label
    return ann


def _dot2(u, v):
    s0 = s1 = 0.0
    for i in range(0, len(u) - 1, 2):
        s0 += u[i] * v[i]
        s1 += u[i + 1] * v[i + 1]
    s = s0 + s1
    if len(u) % 2:
        s += u[-1] * v[-1]
    return s


def _a_distance_the_base_trial_computed(cache, f, base_hp):
    """A cosine distance (cluster.cpp's expression: dot2's two partial sums, sqrt, one division) between a local
    speaker and the centroid the base trial maps it to, read back from a host run, at which `dist >= delta_new`
    decides: two trials whose delta_new are that distance and the next double above it can only differ where a
    computed distance equals the first bit for bit, so the first candidate at which they do differ is a real tie."""
    tau, rho, delta = base_hp
    assign = cache.replay(np.array([base_hp]), backend="host")[0][0]
    clu = OnlineSpeakerClustering(tau, rho, delta, "cosine", G)
    tried = 0
    for c in range(f["seg"].shape[0]):
        centers, active = clu.centers, clu.active_centers
        clu(SlidingWindowFeature(f["seg"][c], SlidingWindow(start=0.0, duration=0.1, step=0.1)), torch.from_numpy(f["emb"][c]))
        if c < 15:
            continue
        for k in range(K):
            g = int(assign[c, k])
            if g < 0 or g not in active or np.isnan(f["emb"][c, k]).any():
                continue
            u, v = [float(x) for x in f["emb"][c, k]], [float(x) for x in centers[g]]
            dist = 1.0 - _dot2(u, v) / (math.sqrt(_dot2(u, u)) * math.sqrt(_dot2(v, v)))
            if not 0.05 < dist < delta:
                continue
            pair = np.array([(tau, rho, dist), (tau, rho, np.nextafter(dist, 2.0))])
            got = cache.replay(pair, backend="host")[0]
            tried += 1
            if not np.array_equal(got[0], got[1]):
                return dist
    raise AssertionError(f"none of {tried} mapped distances decided anything")


@pytest.mark.parametrize("latency,shifts", [(0.5, (0.0, -1.75)), (5.0, (-2.25, 0.0))])
def test_host_replay_is_the_python_path(latency, shifts):
    """Per trial the host backend's hypothesis equals SpeakerDiarization.finalise + PredictionAccumulator on the cached
    arrays (equal turns after support), its assignments are dz_clu_step's, and dz_tune_score's components are the
    metric's on that hypothesis.  Trials: the base values, tau equal to a score that occurs in seg, delta equal to a
    distance the base trial computed (and the next double above it: the tie is real, the two trials differ)."""
    files = _files(shifts)
    base_hp = (0.6, 0.3, 1.0)
    cache = TuneCache.from_arrays(files, _config(latency))
    peaks = files[0]["seg"].max(axis=1).ravel()                     # a chunk's max: `max >= tau` meets it exactly
    tau_tie = float(np.sort(peaks[(peaks > 0.55) & (peaks < 0.8)])[3])
    dist = _a_distance_the_base_trial_computed(TuneCache.from_arrays(files[:1], _config(latency)), files[0], base_hp)
    hp = np.array([base_hp, (tau_tie, 0.3, 1.0), (0.6, 0.3, dist), (0.6, 0.3, np.nextafter(dist, 2.0))])
    assign, status, bits = cache.replay(hp, backend="host")
    assert (status == -1).all()
    first = int(cache.chunk_off[1])
    assert not np.array_equal(assign[2, :first], assign[3, :first])
    assert (files[0]["seg"] == np.float32(tau_tie)).any() and not np.array_equal(bits[0], bits[1])
    per_file = cache.score(bits)
    result = cache.evaluate(hp, backend="host")
    assert np.array_equal(result.per_file, per_file)
    for t, (tau, rho, delta) in enumerate(hp):
        metric = DiarizationErrorRate()
        for n, f in enumerate(files):
            want = _python_path(f, _config(latency, tau, rho, delta))
            got = cache.hypothesis(bits[t], n)
            assert _table(got) == _table(want), (t, n)
            assert len(_table(want)) > 3
            comp = metric.components(_reference(f), want)
            total = comp["total"]
            for i, c in enumerate(COMPONENTS):
                assert abs(per_file[t, n, i] - comp[c]) <= 1e-9 * total, (t, n, c, per_file[t, n, i], comp[c])
            metric(_reference(f), want)
        assert abs(result.rate[t] - abs(metric)) <= 3e-9, (t, result.rate[t], abs(metric))


def test_kernel_text_on_the_host_is_the_host_replay():
    """csrc/tune_core.h (what the two GPU kernels are compiled from) run on the host gives dz_clu_step's assignments and
    dz_tail_step's masks: the golden scenarios, a long random seed with as many centroids as local speakers (K = G = 4), the edges (among
    them K = 4 with G = 3 and K = 8 with G = 5: fewer centroids than local speakers; and a chain that stops where the
    reference raises "Cannot update unknown centers": the chunk both backends report is the same)."""
    for name in scenarios.CLUSTERING:
        z = np.load(tc.GOLD / f"clustering_{name}.npz")
        tau, rho, delta, g = z["params"]
        cache = TuneCache.from_arrays([tc.file_of(z["seg"], z["emb"], shift=-0.75)], tc.config_of(tau, rho, delta, g, 2.5))
        hp = tc.neighbours(tau, rho, delta)
        host, core = cache.replay(hp, backend="host"), cache.replay(hp, backend="core")
        assert all(np.array_equal(a, b) for a, b in zip(host, core)), name
        assert np.array_equal(host[0][0], z["assign"].astype(np.int8)), name
    seed, k, d, g, tau, rho, delta = scenarios.CLUSTERING_LONG_RANDOM[3]
    cache = TuneCache.from_arrays([tc.file_of(*tc.long_random(seed, k, d, g, steps=120))], tc.config_of(tau, rho, delta, g, 5.0))
    hp = tc.random_trials((tau, rho, delta), 16)
    host, core = cache.replay(hp, backend="host"), cache.replay(hp, backend="core")
    assert all(np.array_equal(a, b) for a, b in zip(host, core)) and (host[1] == -1).all()
    for name in tc.EDGES:
        cache, hp = tc.edge_cache(name)
        host, core = cache.replay(hp[:9], backend="host"), cache.replay(hp[:9], backend="core")
        assert all(np.array_equal(a, b) for a, b in zip(host, core)), name
        if name == "raises":     # the first trial's second file stops at its chunk 3, and both say so
            assert host[1][0].tolist() == [-1, 3] and (host[0][0, 1 + 3:] == -1).all()


def test_a_chain_that_would_raise_is_reported():
    """A zero embedding of an active speaker makes a NaN distance: the reference raises, dz_clu_step returns non-zero;
    the replay reports the chunk, stops that chain, the trial's rate is NaN and the other trials are unaffected."""
    seg, emb = tc.random_outputs(7, 30, 16, 3, 8)
    seg[11, :, 0], emb[11, 0] = 0.9, 0.0
    cache = TuneCache.from_arrays([tc.file_of(seg, emb)], tc.config_of(0.5, 0.3, 1.0, 4, 2.5))
    hp = np.array([[0.5, 0.3, 1.0], [0.95, 0.3, 1.0]])            # the second trial never sees that speaker as active
    for backend in ("host", "core"):
        assign, status, _ = cache.replay(hp, backend=backend)
        assert status.tolist() == [[11], [-1]] and (assign[0, 11:] == -1).all(), backend
    result = cache.evaluate(hp, backend="host")
    assert np.isnan(result.rate[0]) and np.isfinite(result.rate[1])


def _masks_cache():
    """293 frames per chunk: 30 output rows per 0.5 s step, so a gap of three frames is 0.05 s up to the last bit."""
    chunks = 12
    seg = np.zeros((chunks, 293, 1), dtype=np.float32)
    emb = np.ones((chunks, 1, 2), dtype=np.float32)
    reference = [(0.2, 3.1, "a"), (1.0, 2.0, "b"), (1.5, 4.4, "c"), (1.8, 1.9, "d"), (3.0, 3.05, "a"), (4.4, 5.7, "b")]
    f = dict(uri="masks", seg=seg, emb=emb, starts=tc.starts_for(chunks), res=tc.DURATION / 293, shift=-0.3,
             reference=reference)
    return TuneCache.from_arrays([f], tc.config_of(0.5, 0.3, 1.0, 4, 0.5)), f


def GAPS(cache):
    """(first packed row, frames) of the silences in the hand-made speaker: inside a step and across a step's end.  The
    3-frame ones lie behind the first step, whose prepended rows are 5 / 293 s long: 30 rows per 0.5 s start there."""
    return ((20, 2), (int(cache.row_off[4]) + 10, 3), (70, 4), (int(cache.row_off[3]) - 1, 3), (int(cache.row_off[5]) - 2, 3),
            (int(cache.row_off[6]) - 1, 2), (int(cache.row_off[7]) - 3, 4))


def test_score_is_the_diarization_error_rate():
    """dz_tune_score against metrics.DiarizationErrorRate on hand-made masks: the five components within 1e-9 x total
    (the two differ only in the order in which at most ~1e5 non-negative durations are summed: n * 2^-53 * total).  A
    reference with overlapping turns and more speakers than the hypothesis, an empty hypothesis, and a hypothesis
    speaker with gaps of 2, 3 and 4 frames (the 3-frame gap is the patch collar's tie), inside a step and across one."""
    cache, f = _masks_cache()
    rows = cache.total_rows
    assert (cache.step_rows[1:] == 30).all() and rows > 300
    bits = np.zeros((4, rows), dtype=np.uint32)
    on = np.zeros(rows, dtype=bool)
    on[5:600] = True
    for start, gap in GAPS(cache):
        on[start:start + gap] = False
    bits[0] = on.astype(np.uint32)                                   # one speaker with gaps
    bits[1] = 0                                                      # empty hypothesis
    bits[2] = bits[0] | (np.roll(on, 37).astype(np.uint32) << 2)     # two speakers, four in the reference
    bits[3, 100:130] = 0b1011                                        # three speakers at once, briefly
    got = cache.score(bits)
    ref = _reference(f)
    for t in range(4):
        hyp = cache.hypothesis(bits[t], 0)
        comp = DiarizationErrorRate().components(ref, hyp)
        for i, c in enumerate(COMPONENTS):
            assert abs(got[t, 0, i] - comp[c]) <= 1e-9 * comp["total"], (t, c, got[t, 0, i], comp[c])
        assert comp["total"] > 5.0
    assert got[1, 0, 3] == got[1, 0, 0] and got[1, 0, 2] == 0.0      # nothing hypothesised: everything is missed
    # the collar, gap by gap: the time between the turn that closes at the gap's first row and the one that opens
    # behind it, from the same frame middles the turns are made of.  2-frame gaps are patched, 4-frame gaps are not,
    # the 3-frame gaps sit on 0.05 up to the last bits and fall on either side of `gap < 0.05`
    step_of = np.repeat(np.arange(len(cache.step_rows)), cache.step_rows)
    kept, ties = 0, []
    for start, frames in GAPS(cache):
        c = int(step_of[start])
        close = cache.mids[start + c - 1] if start == cache.row_off[c] else cache.mids[start + c]
        gap = cache.mids[start + frames + int(step_of[start + frames])] - close
        patched = gap <= 1e-6 or gap < 0.05
        assert patched == (frames == 2) or frames == 3, (start, frames, gap)
        if frames == 3:
            assert abs(gap - 0.05) < 1e-12, (start, gap)
            ties.append(patched)
        kept += not patched
    assert len(ties) == 3 and kept == 2 + ties.count(False)
    turns = _table(cache.hypothesis(bits[0], 0))
    assert len(turns) == 1 + kept, (turns, ties)


def test_cache_round_trip_and_refusals(tmp_path):
    files = _files()
    cache = TuneCache.from_arrays(files, _config(2.5))
    cache.save(tmp_path / "cache.npz")
    again = TuneCache.load(tmp_path / "cache.npz")
    hp = tc.random_trials((0.6, 0.3, 1.0), 5)
    a, b = cache.evaluate(hp, backend="host"), again.evaluate(hp, backend="host")
    assert np.array_equal(a.per_file, b.per_file) and np.array_equal(a.rate, b.rate, equal_nan=True)
    assert a.rate.shape == (5,) and a.components.shape == (5, 5) and a.per_file.shape == (5, 2, 5) and a.status.shape == (5, 2)
    # trials in batches that fit the memory budget: same numbers
    c = cache.evaluate(hp, backend="host", memory_budget=2 * cache.bytes_per_trial)
    assert np.array_equal(a.per_file, c.per_file)
    with pytest.raises(ValueError, match="max_speakers = 33"):
        TuneCache.from_arrays(files, tc.config_of(0.6, 0.3, 1.0, 33, 2.5))
    from diart_amd.blocks.vad import VoiceActivityDetection
    with pytest.raises(ValueError, match="VoiceActivityDetection"):
        TuneCache.collect(VoiceActivityDetection, _config(2.5), tmp_path, tmp_path)


def _optimizer(tmp_path, cache, **kw):
    kw.setdefault("base_config", _config(2.5))
    return Optimizer(SpeakerDiarization, None, None, tmp_path / "study", cache=cache, backend="host", **kw)


def test_optimizer_bookkeeping(tmp_path):
    cache = TuneCache.from_arrays(_files(), _config(2.5))
    calls = []
    evaluate = cache.evaluate

    def counting(hp, **kw):
        calls.append(np.array(hp))
        return evaluate(hp, **kw)

    cache.evaluate = counting
    opt = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4)
    opt(10, show_progress=False)
    # kick-start: the base configuration's values are trial 0; trials are evaluated trials_per_batch at a time
    assert [len(c) for c in calls] == [4, 4, 2] and len(opt.trials) == 10
    assert opt.trials[0]["params"] == {"tau_active": 0.6, "rho_update": 0.3, "delta_new": 1.0}
    assert [t["number"] for t in opt.trials] == list(range(10))
    for t in opt.trials[1:]:
        assert 0 <= t["params"]["tau_active"] <= 1 and 0 <= t["params"]["rho_update"] <= 1 and 0 <= t["params"]["delta_new"] <= 2
    # the objective is the metric in percent, best_* the arg-min of what evaluate returned
    hp = np.concatenate(calls)
    rates = evaluate(hp, backend="host").rate
    assert np.array_equal(np.array([t["value"] for t in opt.trials]), 100.0 * rates)
    best = int(np.argmin(rates))
    assert opt.best_performance == 100.0 * rates[best] and opt.best_hparams == opt.trials[best]["params"]
    assert list(opt.best_hparams) == ["tau_active", "rho_update", "delta_new"]
    stored = json.loads((tmp_path / "study" / "study.json").read_text())
    assert stored["trials"] == opt.trials
    # resume: the stored trials are loaded, the numbering continues, nothing stored is evaluated again
    calls.clear()
    again = _optimizer(tmp_path, cache, seed=3, trials_per_batch=4)
    assert again.trials == opt.trials
    again(3, show_progress=False)
    assert [len(c) for c in calls] == [3] and [t["number"] for t in again.trials] == list(range(13))
    assert again.trials[:10] == opt.trials
    # the same seed draws the same sequence whether or not the study was interrupted
    fresh = _optimizer(tmp_path / "other", cache, seed=3, trials_per_batch=256)
    fresh(13, show_progress=False)
    assert [t["params"] for t in fresh.trials] == [t["params"] for t in again.trials]
    assert [t["params"] for t in _optimizer(tmp_path / "third", cache, seed=4)(5, show_progress=False).trials][1:] != \
        [t["params"] for t in fresh.trials][1:5]
    # maximize picks the other end
    worst = _optimizer(tmp_path / "worst", cache, seed=3, direction="maximize")
    worst(13, show_progress=False)
    assert worst.best_performance == max(t["value"] for t in fresh.trials)
    # a stored study is continued with its own hyper-parameters and direction only
    with pytest.raises(ValueError, match="study of .*minimize.*not of .*maximize"):
        _optimizer(tmp_path / "other", cache, seed=3, direction="maximize")
    with pytest.raises(ValueError, match=r"study of \['tau_active', 'rho_update', 'delta_new'\].*not of \['tau_active'\]"):
        _optimizer(tmp_path / "other", cache, seed=3, hparams=[base.TauActive])


def test_optimizer_grid_and_defaults(tmp_path):
    cache = TuneCache.from_arrays(_files(), _config(2.5))
    opt = _optimizer(tmp_path, cache, sampler="grid", do_kickstart_hparams=False)
    opt(30, show_progress=False)                 # the largest cube not above 30: 3 x 3 x 3
    assert len(opt.trials) == 27
    assert sorted({t["params"]["delta_new"] for t in opt.trials}) == [0.5, 1.0, 1.5]
    again = _optimizer(tmp_path, cache, sampler="grid", do_kickstart_hparams=False)
    again(30, show_progress=False)
    assert again.trials == opt.trials            # deterministic, and nothing stored is evaluated again
    # a subset of the hyper-parameters: the others keep the base configuration's values
    one = _optimizer(tmp_path / "one", cache, hparams=[base.TauActive], seed=1)
    one(4, show_progress=False)
    assert all(list(t["params"]) == ["tau_active"] for t in one.trials)
    assert one._values(one.trials[1]["params"])[1:] == [0.3, 1.0]
    cfg = trial_config(_config(2.5), one.trials[1]["params"])
    assert cfg.tau_active == one.trials[1]["params"]["tau_active"] and cfg.rho_update == 0.3 and cfg.latency == 2.5


def test_optimizer_refusals(tmp_path):
    cache = TuneCache.from_arrays(_files(), _config(2.5))
    with pytest.raises(ValueError, match="gamma.*changes the model outputs"):
        _optimizer(tmp_path, cache, hparams=[base.TauActive, base.HyperParameter("gamma", 0, 10)])
    from diart_amd.blocks.vad import VoiceActivityDetection
    with pytest.raises(ValueError, match="VoiceActivityDetection"):
        Optimizer(VoiceActivityDetection, None, None, tmp_path / "study", base_config=_config(2.5), cache=cache)

    class Custom(SpeakerDiarization):
        pass

    with pytest.raises(ValueError, match="Custom"):
        Optimizer(Custom, None, None, tmp_path / "study", base_config=_config(2.5), cache=cache)
    with pytest.raises(TypeError, match="path-like.*dict"):
        Optimizer(SpeakerDiarization, None, None, {"study": 1}, base_config=_config(2.5), cache=cache)
    with pytest.raises(ValueError, match="max_speakers = 33"):
        _optimizer(tmp_path, cache, base_config=_config(2.5, max_speakers=33))
    from diart_amd.metrics import DetectionErrorRate
    with pytest.raises(ValueError, match="DetectionErrorRate"):
        _optimizer(tmp_path, cache, metric=DetectionErrorRate())
    _optimizer(tmp_path, cache, metric=DiarizationErrorRate())


def test_exports_and_command_line(tmp_path):
    import diart_amd
    assert diart_amd.Optimizer is Optimizer and diart_amd.TuneCache is TuneCache
    from diart_amd import tune
    cache = TuneCache.from_arrays(_files(), _config(2.5))
    cache.save(tmp_path / "cache.npz")
    args = tune.parser().parse_args([str(tmp_path), "--reference", str(tmp_path), "--output", str(tmp_path / "study"),
                                     "--num-iter", "6", "--hparams", "tau_active", "delta_new", "--sampler", "random",
                                     "--seed", "2", "--trials-per-batch", "4", "--cache", str(tmp_path / "cache.npz"),
                                     "--latency", "2.5", "--cpu"])
    opt = tune.run(args, models=(M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                 M.EmbeddingModel(lambda: scenarios.ToyEmbedding())))
    assert len(opt.trials) == 6 and all(list(t["params"]) == ["tau_active", "delta_new"] for t in opt.trials)
    assert (tmp_path / "study" / "study.json").exists()
