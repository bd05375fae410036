"""Minimum durations (min_duration_on / min_duration_off) on the GPU: the tuner's kernel under its third rule
(tune_vad_score_kernel<TcDurRule>: one walk per lane, the lanes' span summaries composed in lane order) against the
kernel's text on the host, the sequential host text and the Python rule; the file batch and the one-file-at-a-time loop
with durations in the configuration.  The rule and the tuner's cases are tests/min_duration_cases.py's."""
import gc
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import min_duration_cases as mc  # noqa: E402
import test_gpu_track_tuner_golden as golden_gpu  # noqa: E402
from test_track_tuner_golden import golden, recorded  # noqa: E402,F401

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import VoiceActivityDetection, VoiceActivityDetectionConfig  # noqa: E402
from diart_amd.metrics import COMPONENTS, DetectionErrorRate, OverlapDetectionErrorRate  # noqa: E402
from diart_amd.synth import synth_segmentation_state, synth_stream  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 16000
METRICS = {"vad": DetectionErrorRate, "osd": OverlapDetectionErrorRate}


def _bars(cache, per_file):
    """1e-9 x total per file; where a file's total is 0, 1e-9 x the sum of its cells' durations."""
    total = per_file[..., 0]
    span = np.array([cache.cell_dur[a:b].sum() for a, b in zip(cache.file_cell_off[:-1], cache.file_cell_off[1:])])
    return 1e-9 * np.where(total > 0, total, span[None, :])


def _reference(f):
    from diart_amd.features import Annotation, Segment
    ann = Annotation(uri=f["uri"])
    for n, (s, e, label) in enumerate(f["reference"]):
        ann[Segment(s, e), n] = label
    return ann


@pytest.mark.parametrize("kind", ["vad", "osd"])
def test_tuner_on_the_device(gpu, kind):
    """On the five files (9, 60, 300, 520 chunks and one) and every trial: "gpu" equals "core" at 256 lanes bit for bit
    — one text, one order —, is within 1e-9 x total of "host" (the sequential text) and of the Python chain hypothesis()
    -> the rule -> the metric's components, and returns the same doubles on a second call; the (T, 4) masks are the
    (T, 2) masks."""
    cache, files = mc.cache(kind), mc.files(kind)
    quads = mc.trials(cache)
    agg_g, bits = cache.replay(quads, backend="gpu")
    agg_c, bits_core = cache.replay(quads, backend="core")
    assert np.array_equal(agg_g, agg_c, equal_nan=True)
    assert bits.dtype == np.uint32 and np.array_equal(bits, bits_core)
    assert np.array_equal(bits, cache.replay(quads[:, :2], backend="gpu")[1])
    assert np.array_equal(bits, cache.replay(quads, backend="host")[1])
    mc.check_trials(cache, quads, bits)
    got, again = cache.evaluate(quads, backend="gpu"), cache.evaluate(quads, backend="gpu")
    core, host = cache.evaluate(quads, backend="core"), cache.evaluate(quads, backend="host")
    assert np.array_equal(got.per_file, again.per_file) and np.array_equal(got.rate, again.rate)
    assert np.array_equal(got.per_file, core.per_file) and np.array_equal(got.rate, core.rate)
    bars = _bars(cache, host.per_file)
    print(f"{kind}: max |gpu - host| / bar = {(np.abs(got.per_file - host.per_file) / bars[..., None]).max():.3g}")
    assert (np.abs(got.per_file - host.per_file) <= bars[..., None]).all()
    worst = 0.0
    for t, (_, _, on, off) in enumerate(quads):
        for n, f in enumerate(files):
            kept = mc.min_duration(mc.turns_of(cache.hypothesis(bits[t], n)), on, off)
            want = METRICS[kind]().components(_reference(f), mc.annotation_of(kept, f["uri"], cache.LABEL))
            assert mc.turns_of(cache.hypothesis(bits[t], n, on, off)) == kept, (t, n)
            for i, c in enumerate(COMPONENTS):
                worst = max(worst, abs(got.per_file[t, n, i] - want[c]) / bars[t, n])
                assert abs(got.per_file[t, n, i] - want[c]) <= bars[t, n], (t, n, c, got.per_file[t, n, i], want[c])
    print(f"{kind}: max |gpu - python| / bar = {worst:.3g}")
    assert (got.per_file[mc.NOTHING, :, 3] == got.per_file[mc.NOTHING, :, 0]).all()     # nothing left: all missed
    assert (got.per_file[mc.NOTHING, :, 2] == 0).all()
    # zero durations: what (T, 2) gives, within the bar (prefix sums differenced per span, not per turn)
    zero = np.concatenate([quads[:, :2], np.zeros((len(quads), 2))], axis=1)
    pairs = cache.evaluate(quads[:, :2], backend="gpu")
    assert (np.abs(cache.evaluate(zero, backend="gpu").per_file - pairs.per_file) <= bars[..., None]).all()


@pytest.mark.parametrize("name", list(golden.CASES))
def test_one_and_two_columns_are_what_they_were(gpu, recorded, name):  # noqa: F811
    """(T,) and (T, 2): the recorded masks and components of tests/golden/track_tuner.npz, through the existing helper."""
    golden_gpu.test_gpu_returns_the_recorded_bits(gpu, recorded, name)


def _rttm_turns(text):
    """{uri: [(start, end)]} of RTTM text, as printed: three decimals."""
    out = {}
    for line in text.splitlines():
        parts = line.split()
        out.setdefault(parts[1], []).append((float(parts[3]), float(parts[3]) + float(parts[4])))
    return out


def test_file_batch_and_benchmark_with_durations(gpu, tmp_path):
    """Benchmark(VoiceActivityDetection) with min_duration_on / min_duration_off in the configuration on two short
    files: the file batch writes the RTTM files of the one-file-at-a-time loop byte for byte, and they are the rule
    applied to the turns of the zero-duration run's RTTM files.  Those are printed with three decimals, so a start or
    a duration read back is within 5e-4 of its value: the durations are chosen at least 5e-3 from every gap and every
    merged duration, and a turn's start and end are compared within 2e-3 (an end is formed from three such numbers and
    compared with a fourth)."""
    from diart_amd.inference import Benchmark, write_wav
    state = synth_segmentation_state(seed=31)
    speech = tmp_path / "wav"
    speech.mkdir()
    for name, seed, dur in (("a", 11, 12.3), ("b", 12, 9.05)):
        write_wav(speech / f"{name}.wav", synth_stream(seed, dur), SR)

    def run(tag, on, off, k):
        cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel.from_state(state, max_batch=32), tau_active=0.6,
                                           min_duration_on=on, min_duration_off=off, device=gpu)
        out = tmp_path / tag
        b = Benchmark(speech, None, out, show_report=False, batch_size=32, concurrent_files=k)
        b(VoiceActivityDetection, cfg)
        path = b.last_path
        del b
        gc.collect()
        return path, {p.name: p.read_text() for p in sorted(out.iterdir())}

    _, zero = run("zero", 0.0, 0.0, 2)
    turns = {name: _rttm_turns(text).get(name[:-5], []) for name, text in zero.items()}
    gaps = sorted(g for t in turns.values() for g in mc.gaps_of(t))
    assert len(gaps) >= 2, gaps
    # min_duration_off: between two gaps that occur, as far from both as can be; min_duration_on likewise, among the
    # durations of the spans that min_duration_off leaves
    widest = max(range(len(gaps) - 1), key=lambda i: gaps[i + 1] - gaps[i])
    off = 0.5 * (gaps[widest] + gaps[widest + 1])
    durations = sorted(e - s for t in turns.values() for s, e in mc.support(t, off))
    assert len(durations) >= 2, durations
    widest = max(range(len(durations) - 1), key=lambda i: durations[i + 1] - durations[i])
    on = 0.5 * (durations[widest] + durations[widest + 1])
    assert min(abs(g - off) for g in gaps) > 5e-3 and min(abs(d - on) for d in durations) > 5e-3
    assert off > mc.PATCH_COLLAR + 5e-3        # (the collar of the rule is min_duration_off, also on the printed turns)
    loop_path, loop = run("loop", on, off, 0)
    batch_path, batch = run("batch", on, off, 2)
    assert (loop_path, batch_path) == ("one_file_at_a_time", "file_batch")
    assert sorted(loop) == ["a.rttm", "b.rttm"] and batch == loop
    assert batch != zero, "the durations change nothing here"
    for name, text in batch.items():
        want, got = mc.min_duration(turns[name], on, off), _rttm_turns(text).get(name[:-5], [])
        assert len(got) == len(want), (name, got, want)
        assert np.abs(np.array(got) - np.array(want)).max() <= 2e-3 if want else True, (name, got, want)
    # FileBatch itself takes them, for both one-track forms; the engine under the files never sees them
    from diart_amd.pipeline import FileBatch
    fb = FileBatch(M.HipSegmentation(state, max_batch=8), None, rows=8, max_files=2, pipeline="osd", tau_active=0.5,
                   min_duration_on=0.25, min_duration_off=0.1, device=gpu)
    assert (fb.min_duration_on, fb.min_duration_off) == (0.25, 0.1) and not hasattr(fb.engine, "min_duration_on")
