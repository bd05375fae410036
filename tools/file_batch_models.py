#!/usr/bin/env python
"""The file batch against the one-file-at-a-time loop, per model, in one process.

    python tools/file_batch_models.py --model wespeaker --files 16 --seconds 600
    python tools/file_batch_models.py --model ecapa --batch-size 1 --files 16 --seconds 600
    python tools/file_batch_models.py --model vad --files 16 --seconds 600

`Benchmark` runs a directory of files either through `FileBatch` (the next windows of up to `--concurrent-files` open
files share one GPU step) or through the reference-shaped loop (`concurrent_files=0`: one file at a time, batches of
`--batch-size` windows, a per-chunk Python tail).  This tool times both on the same corpus: a warm run of each on a short
file (weights packed, arenas allocated, kernels loaded), then `--repeats` timed runs of each, alternating, and one JSON
line with chunks/s of every run, the medians and the path each took.  Synthetic corpus and seeded random weights, as
`tools/benchmark_files.py` (the RTTM identity of the two paths is gated in tests/test_gpu_file_batch_models.py).  A
groups-form model (`ecapa`) takes the file batch at `--batch-size 1` only: at any other batch size both columns are the
loop and `path` says so."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import (SpeakerDiarization, SpeakerDiarizationConfig, VoiceActivityDetection,  # noqa: E402
                              VoiceActivityDetectionConfig)
from diart_amd.hostinfo import limit_host_threads  # noqa: E402
from diart_amd.inference import Benchmark, wav_duration, write_wav  # noqa: E402
from diart_amd.synth import (synth_ecapa_state, synth_embedding_state, synth_segmentation_state,  # noqa: E402
                             synth_stream, synth_wespeaker_state)

ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=("xvector", "wespeaker", "ecapa", "vad"), required=True)
ap.add_argument("--files", type=int, default=16)
ap.add_argument("--seconds", type=float, default=600.0, help="duration of the first file; file i is 7 %% shorter than i-1")
ap.add_argument("--batch-size", type=int, default=32)
ap.add_argument("--concurrent-files", type=int, default=16)
ap.add_argument("--precision", type=str, default=None, help="f16x3 | f32 (default: the package's)")
ap.add_argument("--latency", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--workdir", type=str, default=None,
                help="corpus and RTTM files (default: file_batch_models under the system's temporary directory)")
args = ap.parse_args()

limit_host_threads()
device = torch.device("cuda", 0)
torch.cuda.set_device(device)
work = Path(args.workdir) if args.workdir else Path(tempfile.gettempdir()) / "file_batch_models"
speech, warm = work / "wav", work / "wav_warm"          # the corpus folder of tools/benchmark_files.py
for folder in (speech, warm):
    folder.mkdir(parents=True, exist_ok=True)
for i in range(args.files):
    p = speech / f"synthetic_{i:02d}.wav"
    if not p.exists():
        write_wav(p, synth_stream(1000 + i, max(6.0, args.seconds * 0.93 ** i)), 16000)
if not (warm / "warm.wav").exists():
    write_wav(warm / "warm.wav", synth_stream(999, 12.0), 16000)

powerset = args.model == "ecapa"                 # BASELINE config 3: powerset segmentation + ECAPA-TDNN
seg_sd = synth_segmentation_state(seed=77, powerset=True) if powerset else synth_segmentation_state()
seg = M.SegmentationModel.from_state(seg_sd, max_batch=args.batch_size, powerset=powerset, precision=args.precision)
if args.model == "vad":
    pipeline = VoiceActivityDetection
    cfg = VoiceActivityDetectionConfig(segmentation=seg, latency=args.latency, device=device)
    names = "pyannote/segmentation (VoiceActivityDetection)"
else:
    pipeline = SpeakerDiarization
    emb_sd, names = {"xvector": (synth_embedding_state, "pyannote/segmentation + pyannote/embedding"),
                     "wespeaker": (synth_wespeaker_state, "pyannote/segmentation + wespeaker-voxceleb-resnet34-LM"),
                     "ecapa": (synth_ecapa_state, "segmentation-3.0 (powerset) + ECAPA-TDNN")}[args.model]
    hp = dict(normalize_embedding_weights=True, tau_active=0.5) if powerset else {}
    cfg = SpeakerDiarizationConfig(
        segmentation=seg, embedding=M.EmbeddingModel.from_state(emb_sd(), max_batch=3 * args.batch_size,
                                                                precision=args.precision),
        latency=args.latency, device=device, **hp)

paths = sorted(speech.glob("*.wav"))[:args.files]
chunks = sum(max(0, int((wav_duration(p) + args.latency - cfg.step - cfg.duration) / cfg.step) + 1) for p in paths)
benches = {"loop": Benchmark(warm, None, work / "rttm_loop", show_report=False, batch_size=args.batch_size,
                             concurrent_files=0),
           "file_batch": Benchmark(warm, None, work / "rttm_file_batch", show_report=False, batch_size=args.batch_size,
                                   concurrent_files=args.concurrent_files)}
for b in benches.values():                        # the warm run; the file batch keeps its engine (Benchmark caches it)
    b(pipeline, cfg)
    b.speech_path = speech
torch.cuda.synchronize()
runs = {name: [] for name in benches}
for _ in range(max(1, args.repeats)):
    for name, b in benches.items():
        t0 = time.perf_counter()
        b(pipeline, cfg)
        torch.cuda.synchronize()
        runs[name].append(round(chunks / (time.perf_counter() - t0), 1))
print(json.dumps({
    "model": args.model, "models": names,
    "workload": f"{len(paths)} synthetic 16 kHz files, {sum(wav_duration(p) for p in paths):.0f} s of audio, {chunks} chunks, "
                f"batch {args.batch_size}, latency {args.latency}, {args.concurrent_files} concurrent files",
    "precision": args.precision or M.default_precision(),
    "path": {name: b.last_path for name, b in benches.items()},
    "chunks_per_second": {name: statistics.median(v) for name, v in runs.items()},
    "runs_chunks_per_second": runs}), flush=True)
