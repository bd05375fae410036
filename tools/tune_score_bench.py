"""Where a SpeakerDiarization tuning trial is scored: `TuneCache.evaluate` on the GPU backend with the masks copied to
the host and scored by `dz_tune_score` (scoring="host", the default) against the same call with `tune_score_kernel`
(scoring="device"), in one process on one GPU.

The dataset is tools/tune_bench.py's (`--files` synthetic files of `--seconds` seconds, pyannote/embedding with synthetic
weights, the pipeline's own output at the base configuration as references).  For every T of `--trials`, a warm run of
each leg first, then `--reps` runs of each, the two legs alternating: the wall time of `evaluate` (it ends with the
results on the host, so the device has finished); with host scoring the copy of the masks and `dz_tune_score` on
`--threads` threads alone; with device scoring the score kernel alone (device events) with its scratch bytes and the
bytes it has to read at least (the masks once, the cells' durations and reference masks once per pair) over that time,
against 8 TB/s of HBM.  One JSON line, `--out FILE`."""
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

HBM_BYTES_PER_S = 8.0e12


def stats(times):
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), runs=len(times))


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def event_ms(fn, device):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(device)
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--trials", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--latency", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "r21a_tune_score.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tune_score_bench.py measures on a GPU; there is none")
    device = torch.device("cuda", 0)
    out = dict(tool="tools/tune_score_bench.py", files=args.files, seconds=args.seconds, latency=args.latency,
               batch_size=args.batch_size, host_threads=args.threads, reps=args.reps, gpu=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        speech, refs = Path(tmp) / "wav", Path(tmp) / "rttm"
        speech.mkdir()
        for i in range(args.files):
            write_wav(speech / f"f{i:02d}.wav", synth_stream(5000 + i, args.seconds, num_speakers=3 + i % 3), 16000)
        config = SpeakerDiarizationConfig(
            segmentation=M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=args.batch_size),
            embedding=M.EmbeddingModel.from_state(synth_embedding_state(), max_batch=args.batch_size),
            latency=args.latency, device=device)
        # the references: the pipeline's own output at the base configuration
        Benchmark(speech, None, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)(SpeakerDiarization, config)
        cache = TuneCache.collect(SpeakerDiarization, config, speech, refs, batch_size=args.batch_size)
    cells = int(cache.file_cell_off[-1])
    out["cache"] = dict(chunks=int(cache.chunk_off[-1]), frames=cache.F, local_speakers=cache.K, dim=cache.D,
                        max_speakers=cache.G, output_rows=cache.total_rows, cells=cells, max_cells=cache.max_cells,
                        bytes_per_trial=cache.bytes_per_trial, sorted_steps=cache.sorted_steps)
    rng = np.random.default_rng(0)
    rows = []
    for T in args.trials:
        hp = np.concatenate([[[0.6, 0.3, 1.0]], rng.uniform([0, 0, 0], [1, 1, 2], size=(T - 1, 3))])
        row = dict(trials=T)
        legs = {"host": lambda: cache.evaluate(hp, backend="gpu", num_threads=args.threads),
                "device": lambda: cache.evaluate(hp, backend="gpu", num_threads=args.threads, scoring="device")}
        results = {name: fn() for name, fn in legs.items()}          # the warm runs
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(wall_ms(fn))
        row["evaluate_host_scoring"] = stats(times["host"])
        row["evaluate_device_scoring"] = stats(times["device"])
        host, dev = results["host"], results["device"]
        row["same_status"] = bool(np.array_equal(host.status, dev.status))
        row["largest_difference_over_total"] = float((np.abs(host.per_file - dev.per_file) /
                                                      np.maximum(host.per_file[..., :1], 1e-300)).max())
        row["best_der_percent"] = dict(host=float(100.0 * np.nanmin(host.rate)), device=float(100.0 * np.nanmin(dev.rate)))
        # the parts alone, on the masks of one replay
        arrays = cache._replay_gpu(hp, device)
        torch.cuda.synchronize(device)
        arrays[2].cpu()
        row["copy_masks"] = stats([wall_ms(lambda: arrays[2].cpu()) for _ in range(args.reps)])
        bits = arrays[2].cpu().numpy().view(np.uint32)
        cache.score(bits, args.threads)
        row["host_scoring"] = stats([wall_ms(lambda: cache.score(bits, args.threads)) for _ in range(args.reps)])
        cache._score_gpu(arrays[2])
        torch.cuda.synchronize(device)
        kernel = stats([event_ms(lambda: cache._score_gpu(arrays[2]), device) for _ in range(args.reps)])
        blocks = min(T * cache.N, cache.SCORE_BLOCKS)
        least = 4 * T * cache.total_rows + 16 * T * cells
        kernel.update(scratch_bytes=4 * blocks * (cache.max_cells + 1), workgroups=blocks, bytes_read_at_least=least,
                      bytes_per_s_at_least=least / (1e-3 * kernel["median_ms"]),
                      share_of_hbm=least / (1e-3 * kernel["median_ms"]) / HBM_BYTES_PER_S)
        row["kernel_score"] = kernel
        row["host_over_device_evaluate"] = row["evaluate_host_scoring"]["median_ms"] / row["evaluate_device_scoring"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out["rows"] = rows
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
