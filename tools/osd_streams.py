#!/usr/bin/env python
"""OverlappedSpeechDetection on the N-stream engine (``OverlapBatch``) beside ``VadBatch``, in one process: N synthetic
streams, 5 s windows every 500 ms, segmentation -> track written by the head kernel (the second largest score, or the
max) -> output tail.  Both engines are built once per (streams, precision), run once to warm up, then measured
``--repeats`` times in turn: the two steps differ by a handful of compares per frame, so the question is whether the
OSD step lies inside the spread of the VAD step's repeats.  The engine that is built first also runs first in every
pair, and that order shows in the figures, so every row is measured in both orders (``--first both``: vad, osd, vad,
osd, ... and osd, vad, osd, vad, ...).  Then the stand-alone kernel
(``dz_overlap_track``) on ``(streams x 293, 3)`` scores, timed by device events over ``--calls`` queued calls.  One JSON
line:

    {"tool": "osd_streams", "runs": [{streams, precision, first, lanes, inflight, recurrence,
      vad: {ms_per_step: [...], median, min, max, xrt}, osd: {...}, osd_inside_vad_spread}, ...],
     "kernel": {rows, speakers, calls, us_per_call}}

xRT = windows per second x step (a stream needs 1 / step windows per second of audio).

    python tools/osd_streams.py [--streams 64,256] [--precision both] [--steps 40] [--warmup 10] [--repeats 5]
                                [--first both] [--out profiles/rNN_osd_streams.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diart_amd.functional import overlap_track  # noqa: E402
from diart_amd.hostinfo import limit_host_threads  # noqa: E402
from diart_amd.models import HipSegmentation  # noqa: E402
from diart_amd.pipeline import OverlapBatch, VadBatch  # noqa: E402
from diart_amd.synth import synth_segmentation_state, synth_streams  # noqa: E402

STEP, S, HOP = 0.5, 80000, 8000


def run(pipe, audio, n, t0, count):
    inflight = []
    for t in range(t0, t0 + count):
        inflight.append(pipe.launch(audio[:n, t * HOP:t * HOP + S]))
        if len(inflight) >= pipe.max_inflight:
            pipe.finish(inflight.pop(0))
    while inflight:
        pipe.finish(inflight.pop(0))


def one(n, precision, first, args, audio, device, state):
    engines = {"vad": VadBatch, "osd": OverlapBatch}
    order = [first] + [name for name in engines if name != first]
    pipes = {name: engines[name](HipSegmentation(state, max_batch=n, precision=precision), n, step=STEP, device=device)
             for name in order}
    for pipe in pipes.values():                 # the warm run
        run(pipe, audio, n, 0, args.warmup)
    torch.cuda.synchronize(device)
    ms = {"vad": [], "osd": []}
    for _ in range(args.repeats):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            run(pipe, audio, n, args.warmup, args.steps)
            torch.cuda.synchronize(device)
            ms[name].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
    out = {"streams": n, "step_s": STEP, "precision": precision, "first": first, "steps": args.steps, "warmup": args.warmup,
           "lanes": pipes["osd"].depth, "inflight": pipes["osd"].max_inflight,
           "recurrence": pipes["osd"].recurrence or "model"}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"ms_per_step": v, "median": round(med, 4), "min": min(v), "max": max(v),
                     "xrt": round(n * STEP / (med / 1e3), 1)}
    out["osd_inside_vad_spread"] = out["vad"]["min"] <= out["osd"]["median"] <= out["vad"]["max"]
    del pipes
    torch.cuda.empty_cache()
    return out


def kernel_time(rows, calls, device):
    """Microseconds per call of the stand-alone overlap kernel on (rows, 3) scores: `calls` calls queued back to back
    between two device events (a latency-sized kernel: the figure is launch-bound, not a bandwidth)."""
    scores = torch.rand(rows, 3, device=device)
    for _ in range(10):
        overlap_track(scores)
    torch.cuda.synchronize(device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        overlap_track(scores)
    b.record()
    b.synchronize()
    return {"rows": rows, "speakers": 3, "calls": calls, "us_per_call": round(1e3 * a.elapsed_time(b) / calls, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", default="64,256")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--precision", default="both", choices=["both", "f16x3", "f32"])
    ap.add_argument("--first", default="both", choices=["both", "vad", "osd"],
                    help="the engine that is built first and runs first in every pair")
    ap.add_argument("--out", default="", help="also write the JSON line to this file (profiles/rNN_osd_streams.json)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("osd_streams.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    limit_host_threads()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    counts = [int(s) for s in args.streams.split(",")]
    seconds = (S + HOP * (args.warmup + args.steps + 1)) / 16000.0
    audio = torch.from_numpy(synth_streams(max(counts), seconds, seed0=4242)).to(device)
    state = synth_segmentation_state()
    precs = ["f16x3", "f32"] if args.precision == "both" else [args.precision]
    runs = []
    for n in counts:
        for p in precs:
            for first in (["vad", "osd"] if args.first == "both" else [args.first]):
                runs.append(one(n, p, first, args, audio, device, state))
                print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"tool": "osd_streams", "window_s": 5.0, "gpu": torch.cuda.get_device_name(device), "runs": runs,
                       "kernel": kernel_time(64 * 293, args.calls, device)})
    if args.out:
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
