"""What a VoiceActivityDetection tuning trial costs: `VadTuneCache.evaluate` on the GPU and on the host against
`Benchmark` calls.

Synthetic dataset (no checkpoint): `--files` files of `--seconds` seconds, the segmentation with synthetic weights, and
as references the pipeline's own output at the base configuration.  Records the collect time once, the one-time rows
kernel (device events), then for every T of `--trials` the wall time of `evaluate` on the GPU backend and on the host
backend with `--threads` threads (warm runs first, medians of `--reps`), the score kernel alone (device events), and
the wall time of a `Benchmark` call on the blocks path — what a trial costs without the cache — measured
`--benchmark-calls` times and stated per trial (T such calls are T times that: extrapolated, not run).  One JSON line,
`--out FILE`.

`--pipeline osd` measures the OverlappedSpeechDetection tuner (`OsdTuneCache`: the same kernels behind the overlap track)
and the VAD tuner beside it, in one process on the same files: the references are then three made-up speakers whose
turns overlap, `collect` is timed once per cache and every `evaluate` figure is taken for both caches in turn.

`--hysteresis` measures the two-threshold path beside the single threshold, for both caches on the dataset of
`--pipeline osd`: per T the wall time of `evaluate` and the device time of the scoring kernel for `(T,)` taus
(tune_vad_score_kernel, what the parent commit runs: its own `--pipeline osd` rows on the same files are the yardstick,
taken in a child process of their own) and for `(T, 2)` taus (the kernel's stateful form), with a band of 0.2 under
every tau and with equal columns.  EXPECTATION, written before the first run: the new kernel adds one pass over a lane's
rows (two compares per row, no time stamps read) and a fold over at most 255 bytes of LDS to two walks that read the
time stamps and the prefix sums, so its device time should stay well under twice the plain kernel's at every T — a
supposition; the tool reports the ratio whichever way it falls.

`--min-duration` measures the four-column path — `(T, 4)` = (tau_active, tau_offset, min_duration_on, min_duration_off),
tune_vad_score_kernel<TcDurRule> — beside `(T,)` and `(T, 2)` on the same dataset and in the same form as `--hysteresis`
(whose `plain` and `band` rows of the parent commit, taken in a child process of their own, are the yardstick): per T
the wall time of `evaluate` and the device time of the scoring kernel with both durations zero and with durations
drawn from U(0, 1), the range the Optimizer draws from.  EXPECTATION, written before the first run: against the `(T, 2)`
kernel the new one walks a lane's steps once instead of twice (the time stamps and the cells of a turn are read once),
keeps the pass of the state maps, stores eleven words per lane instead of four, and ends with ONE lane composing 256
summaries from LDS — a serial loop of some 256 x 11 LDS reads, a few microseconds during which the other 255 lanes wait —
where the `(T, 2)` kernel has every lane fold up to 255 ends and one lane add 256 sums.  The two should cost about the
same: a device-time ratio between 0.8 and 1.3 at 64 and 1 024 trials, where the kernel is a few hundred workgroups or
more per CU wave, and nearer 1.3 - 1.5 at one trial, where 16 workgroups leave the serial tail exposed.  Large
min_duration_off merges more turns per span and so touches the prefix sums less: random durations should not cost more
than zeros.  A supposition; the tool reports the ratios whichever way they fall."""
import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from tune_bench import events_ms, median_ms  # noqa: E402

from diart_amd import _lib  # noqa: E402
from diart_amd import models as M  # noqa: E402
from diart_amd.blocks.vad import VoiceActivityDetection, VoiceActivityDetectionConfig  # noqa: E402
from diart_amd.inference import Benchmark, write_wav  # noqa: E402
from diart_amd.optim import VadTuneCache  # noqa: E402  (OsdTuneCache: imported where --pipeline osd needs it)
from diart_amd.synth import synth_segmentation_state, synth_stream  # noqa: E402


def speaker_reference(uri: str, seconds: float) -> str:
    """Three speakers taking turns of different periods over the file (two and three of them at once): an RTTM text."""
    from diart_amd.features import Annotation, Segment
    ann, n = Annotation(uri=uri), 0
    for s in range(3):
        t = 0.37 * s
        while t < seconds:
            ann[Segment(t, min(seconds, t + 2.9 + 0.61 * s)), n] = f"ref{s}"
            t, n = t + 4.3 + 0.83 * s, n + 1
    return ann.to_rttm()


def evaluate_rows(cache, trials, reps: int, threads: int, device, rng) -> list:
    rows = []
    for T in trials:
        taus = np.concatenate([[0.6], rng.uniform(0, 1, size=T - 1)])
        row = dict(trials=T)
        gpu = cache.evaluate(taus, backend="gpu")
        row["gpu_evaluate"] = median_ms(lambda: cache.evaluate(taus, backend="gpu"), reps)
        row["kernel_score"] = events_ms(lambda: cache._gpu(taus, False, True, device), device, reps)
        host = cache.evaluate(taus, backend="host", num_threads=threads)
        row["host_evaluate"] = median_ms(lambda: cache.evaluate(taus, backend="host", num_threads=threads), reps,
                                         warm=0)      # (the call above was the warm run)
        total = np.maximum(host.per_file[..., :1], 1e-300)
        row["largest_component_error_over_total"] = float((np.abs(gpu.per_file - host.per_file) / total).max())
        row["best_rate_percent"] = float(100.0 * host.rate.min())
        row["gpu_over_host"] = row["host_evaluate"]["median_ms"] / row["gpu_evaluate"]["median_ms"]
        rows.append(row)
    return rows


def hysteresis_rows(cache, trials, reps: int, device, rng) -> list:
    """Per T: (T,) taus on today's kernel, (T, 2) taus with a band and with equal columns on the hysteresis kernel."""
    rows = []
    for T in trials:
        taus = np.concatenate([[0.6], rng.uniform(0, 1, size=T - 1)])
        forms = dict(plain=taus, band=np.stack([taus, taus - 0.2], axis=1), equal=np.stack([taus, taus], axis=1))
        row = dict(trials=T)
        for name, t in forms.items():
            cache.evaluate(t, backend="gpu")
            row[f"{name}_evaluate"] = median_ms(lambda: cache.evaluate(t, backend="gpu"), reps)
            row[f"{name}_kernel"] = events_ms(lambda: cache._gpu(cache._taus(t), False, True, device), device, reps)
        a, b = cache.evaluate(forms["plain"], backend="gpu"), cache.evaluate(forms["equal"], backend="gpu")
        row["equal_columns_are_plain_bit_for_bit"] = bool(np.array_equal(a.per_file, b.per_file))
        for name in ("band", "equal"):
            row[f"{name}_kernel_over_plain"] = row[f"{name}_kernel"]["median_ms"] / row["plain_kernel"]["median_ms"]
            row[f"{name}_evaluate_over_plain"] = row[f"{name}_evaluate"]["median_ms"] / row["plain_evaluate"]["median_ms"]
        rows.append(row)
    return rows


def min_duration_rows(cache, trials, reps: int, device, rng) -> list:
    """Per T: hysteresis_rows' plain and band forms — (T,) and (T, 2), which must not move — and (T, 4) with both
    durations zero and with durations from U(0, 1), all under the band's thresholds."""
    rows = []
    for T in trials:
        taus = np.concatenate([[0.6], rng.uniform(0, 1, size=T - 1)])
        band = np.stack([taus, taus - 0.2], axis=1)
        forms = dict(plain=taus, band=band, zero=np.concatenate([band, np.zeros((T, 2))], axis=1),
                     drawn=np.concatenate([band, rng.uniform(0, 1, size=(T, 2))], axis=1))
        row = dict(trials=T)
        for name, t in forms.items():
            cache.evaluate(t, backend="gpu")
            row[f"{name}_evaluate"] = median_ms(lambda: cache.evaluate(t, backend="gpu"), reps)
            row[f"{name}_kernel"] = events_ms(lambda: cache._gpu(cache._taus(t), False, True, device), device, reps)
        two, four = cache.evaluate(forms["band"], backend="gpu"), cache.evaluate(forms["zero"], backend="gpu")
        total = np.maximum(two.per_file[..., :1], 1e-300)
        row["zero_durations_against_two_columns_over_total"] = float((np.abs(two.per_file - four.per_file) / total).max())
        row["best_rate_percent"] = {name: float(100.0 * cache.evaluate(forms[name], backend="gpu").rate.min())
                                    for name in ("band", "drawn")}
        for name in ("zero", "drawn"):
            row[f"{name}_kernel_over_band"] = row[f"{name}_kernel"]["median_ms"] / row["band_kernel"]["median_ms"]
            row[f"{name}_evaluate_over_band"] = row[f"{name}_evaluate"]["median_ms"] / row["band_evaluate"]["median_ms"]
        rows.append(row)
    return rows


def both_pipelines(args, device) -> dict:
    """--pipeline osd: the two detection caches collected from the same files, measured side by side."""
    from diart_amd.blocks.osd import OverlappedSpeechDetection, OverlappedSpeechDetectionConfig
    from diart_amd.optim import OsdTuneCache
    out, caches = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        speech, refs = Path(tmp) / "wav", Path(tmp) / "rttm"
        speech.mkdir()
        refs.mkdir()
        for i in range(args.files):
            write_wav(speech / f"f{i:02d}.wav", synth_stream(5000 + i, args.seconds, num_speakers=3 + i % 3), 16000)
            (refs / f"f{i:02d}.rttm").write_text(speaker_reference(f"f{i:02d}", args.seconds))
        seg = M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=args.batch_size)
        kinds = (("vad", VadTuneCache, VoiceActivityDetection, VoiceActivityDetectionConfig),
                 ("osd", OsdTuneCache, OverlappedSpeechDetection, OverlappedSpeechDetectionConfig))
        for warm in (True, False):                # the first pass warms the model and the file cache up
            for name, cache_class, pipeline, config_class in kinds:
                config = config_class(segmentation=seg, latency=args.latency, device=device)
                torch.cuda.synchronize(device)
                t = time.perf_counter()
                caches[name] = cache_class.collect(pipeline, config, speech, refs, batch_size=args.batch_size)
                torch.cuda.synchronize(device)
                out.setdefault(name, {})["collect_warm_s" if warm else "collect_s"] = time.perf_counter() - t
    for name, cache in caches.items():
        out[name]["cache"] = dict(chunks=int(cache.chunk_off[-1]), frames=cache.F, output_rows=cache.total_rows,
                                  cells=int(cache.file_cell_off[-1]), sorted_steps=cache.sorted_steps)
        t = time.perf_counter()
        cache._device(device)
        torch.cuda.synchronize(device)
        out[name]["upload_and_rows_ms"] = 1e3 * (time.perf_counter() - t)
    for name, cache in caches.items():
        if args.min_duration:
            out[name]["rows"] = min_duration_rows(cache, args.trials, args.reps, device, np.random.default_rng(0))
        elif args.hysteresis:
            out[name]["rows"] = hysteresis_rows(cache, args.trials, args.reps, device, np.random.default_rng(0))
        else:
            out[name]["rows"] = evaluate_rows(cache, args.trials, args.reps, args.threads, device, np.random.default_rng(0))
        for row in out[name]["rows"]:
            print(name, json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pipeline", default="vad", choices=("vad", "osd"),
                    help="vad: the VoiceActivityDetection tuner (the default); osd: the OverlappedSpeechDetection tuner "
                         "with the VAD tuner beside it")
    ap.add_argument("--hysteresis", action="store_true",
                    help="(T, 2) taus = (tau_active, tau_offset) beside (T,) taus, for both caches (implies --pipeline osd)")
    ap.add_argument("--min-duration", action="store_true",
                    help="(T, 4) taus = (tau_active, tau_offset, min_duration_on, min_duration_off) beside (T,) and (T, 2) "
                         "taus, for both caches (implies --pipeline osd)")
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--trials", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--benchmark-calls", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--latency", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=None,
                    help="profiles/r20a_tune_vad.json, profiles/r29a_tune_osd.json with --pipeline osd, r32a_tune_hysteresis.json with "
                         "--hysteresis, r34a_tune_min_duration.json with --min-duration")
    args = ap.parse_args()
    if args.hysteresis and args.min_duration:
        raise SystemExit("--hysteresis and --min-duration are two runs")
    if args.hysteresis or args.min_duration:
        args.pipeline = "osd"
    args.out = args.out or str(ROOT / "profiles" / ("r34a_tune_min_duration.json" if args.min_duration else
                                                     "r32a_tune_hysteresis.json" if args.hysteresis else
                                                     "r29a_tune_osd.json" if args.pipeline == "osd" else "r20a_tune_vad.json"))
    if not torch.cuda.is_available():
        raise SystemExit("tune_vad_bench.py measures on a GPU; there is none")
    device = torch.device("cuda", 0)
    if args.pipeline == "osd":
        out = dict(tool="tools/tune_vad_bench.py " + ("--min-duration" if args.min_duration else
                                                      "--hysteresis" if args.hysteresis else "--pipeline osd"), files=args.files, seconds=args.seconds, latency=args.latency,
                   batch_size=args.batch_size, host_threads=args.threads, reps=args.reps, gpu=torch.cuda.get_device_name(0))
        out.update(both_pipelines(args, device))
        line = json.dumps(out)
        print(line, flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
        return
    out = dict(tool="tools/tune_vad_bench.py", files=args.files, seconds=args.seconds, latency=args.latency,
               batch_size=args.batch_size, host_threads=args.threads, gpu=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        speech, refs = Path(tmp) / "wav", Path(tmp) / "rttm"
        speech.mkdir()
        for i in range(args.files):
            write_wav(speech / f"f{i:02d}.wav", synth_stream(5000 + i, args.seconds, num_speakers=3 + i % 3), 16000)
        config = VoiceActivityDetectionConfig(
            segmentation=M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=args.batch_size),
            latency=args.latency, device=device)
        # ---- a Benchmark call on the blocks path: what the reference's Optimizer pays per trial; the first call also
        # writes the references (and warms the model up)
        Benchmark(speech, None, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)(
            VoiceActivityDetection, config)
        scored = Benchmark(speech, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)
        calls = []
        for _ in range(args.benchmark_calls):
            torch.cuda.synchronize(device)
            t = time.perf_counter()
            metric = scored(VoiceActivityDetection, config)
            calls.append(time.perf_counter() - t)
        out["benchmark_call_s"] = dict(median=statistics.median(calls), runs=calls, rate_percent=100.0 * abs(metric),
                                       note="per trial: one call is one trial")
        # ---- the model once
        torch.cuda.synchronize(device)
        t = time.perf_counter()
        cache = VadTuneCache.collect(VoiceActivityDetection, config, speech, refs, batch_size=args.batch_size)
        torch.cuda.synchronize(device)
        out["collect_s"] = time.perf_counter() - t
    out["cache"] = dict(chunks=int(cache.chunk_off[-1]), frames=cache.F, output_rows=cache.total_rows,
                        cells=int(cache.file_cell_off[-1]), sorted_steps=cache.sorted_steps)
    # ---- the rows kernel: once per cache and device (the upload of the cache's arrays is in the first figure only)
    t = time.perf_counter()
    tensors, desc, _ = cache._device(device)
    torch.cuda.synchronize(device)
    out["upload_and_rows_ms"] = 1e3 * (time.perf_counter() - t)
    lib, ctx = _lib.load(), _lib.context(device.index)
    out["kernel_rows"] = events_ms(lambda: _lib.check(lib.dz_tune_vad_rows(
        ctx, C.byref(desc), tensors["agg"].data_ptr(), torch.cuda.current_stream(device).cuda_stream), "dz_tune_vad_rows"),
        device, args.reps)
    rows = evaluate_rows(cache, args.trials, args.reps, args.threads, device, np.random.default_rng(0))
    for row in rows:
        row["benchmark_calls_s_extrapolated"] = row["trials"] * out["benchmark_call_s"]["median"]   # T x one call: not measured
        print(json.dumps(row), flush=True)
    out["rows"] = rows
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
