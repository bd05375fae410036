"""What a tuning trial costs: `TuneCache.evaluate` on the GPU and on the host against `Benchmark` calls.

Synthetic dataset (no checkpoint): `--files` files of `--seconds` seconds, pyannote/embedding with synthetic weights,
and as references the pipeline's own output at the base configuration.  Records the collect time once, then for every
T of `--trials` the wall time of `evaluate` on the GPU backend and on the host backend with `--threads` threads (warm
runs first, medians of `--reps`), the two kernels alone (device events, one phase per launch), the copy of the masks
and the host scoring alone, and the wall time of a `Benchmark` call on the blocks path — what a trial costs without the
cache — measured `--benchmark-calls` times and stated per trial (T such calls are T times that: extrapolated, not
run).  One JSON line, `--out FILE`."""
import argparse
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

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.inference import Benchmark, write_wav  # noqa: E402
from diart_amd.optim import TuneCache  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream  # noqa: E402


def median_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), runs=reps)


def events_ms(fn, device, reps, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(device)
        times.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), runs=reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--trials", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-large-reps", type=int, default=5, help="runs of the host backend at more than 64 trials")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--benchmark-calls", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--latency", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "r18a_tune.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tune_bench.py measures on a GPU; there is none")
    device = torch.device("cuda", 0)
    out = dict(tool="tools/tune_bench.py", files=args.files, seconds=args.seconds, latency=args.latency,
               batch_size=args.batch_size, host_threads=args.threads, gpu=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        speech, refs = Path(tmp) / "wav", Path(tmp) / "rttm"
        speech.mkdir()
        for i in range(args.files):
            write_wav(speech / f"f{i:02d}.wav", synth_stream(5000 + i, args.seconds, num_speakers=3 + i % 3), 16000)
        config = SpeakerDiarizationConfig(
            segmentation=M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=args.batch_size),
            embedding=M.EmbeddingModel.from_state(synth_embedding_state(), max_batch=args.batch_size),
            latency=args.latency, device=device)
        # ---- a Benchmark call on the blocks path: what the reference's Optimizer pays per trial; the first call also
        # writes the references (and warms the models up)
        bench = Benchmark(speech, None, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)
        bench(SpeakerDiarization, config)
        scored = Benchmark(speech, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)
        calls = []
        for _ in range(args.benchmark_calls):
            torch.cuda.synchronize(device)
            t = time.perf_counter()
            metric = scored(SpeakerDiarization, config)
            calls.append(time.perf_counter() - t)
        out["benchmark_call_s"] = dict(median=statistics.median(calls), runs=calls, der_percent=100.0 * abs(metric),
                                       note="per trial: one call is one trial")
        # ---- the models once
        torch.cuda.synchronize(device)
        t = time.perf_counter()
        cache = TuneCache.collect(SpeakerDiarization, config, speech, refs, batch_size=args.batch_size)
        torch.cuda.synchronize(device)
        out["collect_s"] = time.perf_counter() - t
    out["cache"] = dict(chunks=int(cache.chunk_off[-1]), frames=cache.F, local_speakers=cache.K, dim=cache.D,
                        max_speakers=cache.G, output_rows=cache.total_rows, cells=int(cache.file_cell_off[-1]),
                        bytes_per_trial=cache.bytes_per_trial)
    rng = np.random.default_rng(0)
    rows = []
    for T in args.trials:
        hp = np.concatenate([[[0.6, 0.3, 1.0]], rng.uniform([0, 0, 0], [1, 1, 2], size=(T - 1, 3))])
        row = dict(trials=T)
        gpu = cache.evaluate(hp, backend="gpu", num_threads=args.threads)
        row["gpu_evaluate"] = median_ms(lambda: cache.evaluate(hp, backend="gpu", num_threads=args.threads), args.reps)
        arrays = cache._replay_gpu(hp, device)
        torch.cuda.synchronize(device)
        row["kernel_cluster"] = events_ms(lambda: cache._replay_gpu(hp, device, phases=1, into=arrays), device, args.reps)
        row["kernel_masks"] = events_ms(lambda: cache._replay_gpu(hp, device, phases=2, into=arrays), device, args.reps)
        row["copy_masks"] = median_ms(lambda: arrays[2].cpu(), args.reps)
        bits = arrays[2].cpu().numpy().view(np.uint32)
        row["host_scoring"] = median_ms(lambda: cache.score(bits, args.threads), args.reps)
        reps = args.reps if T <= 64 else args.host_large_reps
        host = cache.evaluate(hp, backend="host", num_threads=args.threads)
        row["host_evaluate"] = median_ms(lambda: cache.evaluate(hp, backend="host", num_threads=args.threads), reps,
                                         warm=0)      # (the call above was the warm run)
        row["same_result"] = bool(np.array_equal(gpu.per_file, host.per_file) and np.array_equal(gpu.status, host.status))
        row["trials_that_raise"] = int((host.status >= 0).any(axis=1).sum())
        row["best_der_percent"] = float(100.0 * np.nanmin(host.rate))
        row["gpu_over_host"] = row["host_evaluate"]["median_ms"] / row["gpu_evaluate"]["median_ms"]
        row["benchmark_calls_s_extrapolated"] = T * out["benchmark_call_s"]["median"]      # T x one call: not measured
        rows.append(row)
        print(json.dumps(row), flush=True)
    out["rows"] = rows
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
