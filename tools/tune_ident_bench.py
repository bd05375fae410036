"""What tuning delta_id costs: `IdentTuneCache.evaluate` on the GPU and on the host beside `TuneCache.evaluate`.

The dataset is tools/tune_bench.py's (synthetic, no checkpoint): `--files` files of `--seconds` seconds,
pyannote/embedding with synthetic weights, as references the pipeline's own output at the base configuration with its
labels renamed `person<g>`.  The gallery has `--voiceprints` rows: the mean embedding of every speaker of the first file
under the base trial, named as the references name them, and random rows.  For every T of `--trials`: the wall time of
`IdentTuneCache.evaluate` on the GPU backend and on the host backend with `--threads` threads and of
`TuneCache.evaluate(scoring="device")` in the same process (a warm pass of each first, then medians of `--reps` with the
lowest and the highest), and the name kernel and the ident-score kernel alone by device events.  Both kernels are
latency-sized (a dependent walk per chain; a few thousand cells per pair): no bandwidth figure is formed.

Expectation, written before the first run: the clustering replay is shared and dominates, so the GPU `evaluate` of
both caches should agree within a few percent at every T; the name kernel should cost a few milliseconds at 1 024
trials and the ident-score kernel less than the diarization score kernel (no co-occurrence sweep, no assignment
problem).  One JSON line, `--out FILE`."""
import argparse
import json
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

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.gallery import SpeakerGallery  # noqa: E402
from diart_amd.inference import Benchmark, write_wav  # noqa: E402
from diart_amd.optim import TuneCache  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream  # noqa: E402

BASE = (0.6, 0.3, 1.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--voiceprints", type=int, default=1024)
    ap.add_argument("--trials", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--latency", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "r30a_tune_ident.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tune_ident_bench.py measures on a GPU; there is none")
    device = torch.device("cuda", 0)
    out = dict(tool="tools/tune_ident_bench.py", files=args.files, seconds=args.seconds, latency=args.latency,
               voiceprints=args.voiceprints, host_threads=args.threads, gpu=torch.cuda.get_device_name(0),
               expectation="GPU evaluate of both caches within a few percent; name kernel a few ms at 1 024 trials; "
                           "ident-score kernel below the diarization score kernel")
    with tempfile.TemporaryDirectory() as tmp:
        speech, refs = Path(tmp) / "wav", Path(tmp) / "rttm"
        speech.mkdir()
        for i in range(args.files):
            write_wav(speech / f"f{i:02d}.wav", synth_stream(5000 + i, args.seconds, num_speakers=3 + i % 3), 16000)
        config = SpeakerDiarizationConfig(
            segmentation=M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=args.batch_size),
            embedding=M.EmbeddingModel.from_state(synth_embedding_state(), max_batch=args.batch_size),
            latency=args.latency, device=device)
        Benchmark(speech, None, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)(SpeakerDiarization,
                                                                                                         config)
        collected = TuneCache.collect(SpeakerDiarization, config, speech, refs, batch_size=args.batch_size)
    # the references' labels are the pipeline's own "speaker<g>", which is what unnamed speakers are called: rename them
    files = [dict(f, reference=[(s, e, "person" + str(l)[len("speaker"):]) for s, e, l in f["turns"]]) for f in collected.files]
    base = TuneCache.from_arrays(files, collected.meta)
    assign = base.replay([BASE], backend="gpu")[0][0]
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((args.voiceprints, base.D)).astype(np.float32)
    names = [f"stranger{v}" for v in range(args.voiceprints)]
    c1, enrolled = int(base.chunk_off[1]), 0
    for g in range(base.G):
        own = base.emb[:c1][assign[:c1] == g]
        own = own[~np.isnan(own).any(axis=1)]
        if own.shape[0] and enrolled < args.voiceprints:
            rows[enrolled], names[enrolled] = own.mean(axis=0), f"person{g}"
            enrolled += 1
    gallery = SpeakerGallery(names, rows, device)
    torch.cuda.synchronize(device)
    t = time.perf_counter()
    cache = base.with_gallery(gallery, device)
    out["with_gallery_s"] = time.perf_counter() - t
    out["cache"] = dict(chunks=int(cache.chunk_off[-1]), local_speakers=cache.K, dim=cache.D, max_speakers=cache.G,
                        output_rows=cache.total_rows, cells=int(cache.file_cell_off[-1]), enrolled_speakers=enrolled,
                        bytes_per_trial=cache.bytes_per_trial, bytes_per_trial_diarization=base.bytes_per_trial)
    results = []
    for T in args.trials:
        hp = np.concatenate([[list(BASE) + [0.5]], rng.uniform([0, 0, 0, 0], [1, 1, 2, 2], size=(T - 1, 4))])
        hp3 = np.ascontiguousarray(hp[:, :3])
        row = dict(trials=T)
        gpu = cache.evaluate(hp, backend="gpu")
        row["ident_gpu_evaluate"] = median_ms(lambda: cache.evaluate(hp, backend="gpu"), args.reps, warm=0)
        base.evaluate(hp3, backend="gpu", scoring="device")
        row["diarization_gpu_evaluate_device_scoring"] = median_ms(
            lambda: base.evaluate(hp3, backend="gpu", scoring="device"), args.reps, warm=0)
        a, st, bits = cache._replay_gpu(hp3, device)
        ident, _ = cache._names_gpu(a, st, hp[:, 3])
        torch.cuda.synchronize(device)
        row["kernel_name"] = events_ms(lambda: cache._names_gpu(a, st, hp[:, 3]), device, args.reps)
        row["kernel_ident_score"] = events_ms(lambda: cache._ident_score_gpu(bits, ident), device, args.reps)
        row["kernel_diarization_score"] = events_ms(lambda: base._score_gpu(bits), device, args.reps)
        host = cache.evaluate(hp, backend="host", num_threads=args.threads)
        row["ident_host_evaluate"] = median_ms(lambda: cache.evaluate(hp, backend="host", num_threads=args.threads), args.reps,
                                               warm=0)
        row["largest_difference_over_total"] = float((np.abs(gpu.per_file - host.per_file) / host.per_file[..., :1]).max())
        row["trials_that_raise"] = int((host.status >= 0).any(axis=1).sum())
        row["best_ier_percent"] = float(100.0 * np.nanmin(host.rate))
        row["gpu_over_host"] = row["ident_host_evaluate"]["median_ms"] / row["ident_gpu_evaluate"]["median_ms"]
        results.append(row)
        print(json.dumps(row), flush=True)
    out["rows"] = results
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
