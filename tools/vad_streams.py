#!/usr/bin/env python
"""VoiceActivityDetection on the N-stream engine (``VadBatch``): N synthetic streams, 5 s windows every ``step``,
segmentation -> speech track (the max over speakers, written by the head kernel) -> output tail, for every combination
of the stream counts, steps and precisions asked for.  One JSON line:

    {"tool": "vad_streams", "runs": [{streams, step_s, precision, xrt, ms_per_step, lanes, inflight, recurrence,
     host_wait_s, host_work_s, engine_mb, engine_mb_per_lane}, ...]}

xRT = windows per second x step (a stream needs 1 / step windows per second of audio).

    python tools/vad_streams.py [--streams 64,256] [--step 0.5,0.25] [--precision both] [--steps 40] [--warmup 10]
                                [--tau-offset 0.4]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diart_amd.hostinfo import limit_host_threads  # noqa: E402
from diart_amd.models import HipSegmentation  # noqa: E402
from diart_amd.pipeline import VadBatch  # noqa: E402
from diart_amd.synth import synth_segmentation_state, synth_streams  # noqa: E402


def one(n, step, precision, args, audio, device, state, tau_offset=None):
    hop, S = int(round(16000 * step)), 80000
    torch.cuda.synchronize(device)
    free0 = torch.cuda.mem_get_info(device)[0]
    pipe = VadBatch(HipSegmentation(state, max_batch=n, precision=precision), n, step=step, device=device,
                    lanes=args.lanes or None, **({} if tau_offset is None else dict(tau_offset=tau_offset)))

    def run(t0, count):
        inflight = []
        for t in range(t0, t0 + count):
            inflight.append(pipe.launch(audio[:n, t * hop:t * hop + S]))
            if len(inflight) >= pipe.max_inflight:
                pipe.finish(inflight.pop(0))
        while inflight:
            pipe.finish(inflight.pop(0))

    run(0, args.warmup)
    torch.cuda.synchronize(device)
    # device memory the engine took (every lane's handle + the in-flight slots; hipMalloc'd, outside torch's cache)
    engine_mb = (free0 - torch.cuda.mem_get_info(device)[0]) / 2**20
    pipe.host_seconds = {"wait": 0.0, "work": 0.0}
    t0 = time.perf_counter()
    run(args.warmup, args.steps)
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0
    host = dict(pipe.host_seconds)
    out = {"streams": n, "step_s": step, "precision": precision, "tau_offset": tau_offset, "xrt": round(n * args.steps / elapsed * step, 1),
           "ms_per_step": round(1e3 * elapsed / args.steps, 3), "steps": args.steps, "warmup": args.warmup,
           "lanes": pipe.depth, "inflight": pipe.max_inflight, "recurrence": pipe.recurrence or "model",
           "host_wait_s": round(host["wait"], 4), "host_work_s": round(host["work"], 4),
           "engine_mb": round(engine_mb, 1), "engine_mb_per_lane": round(engine_mb / pipe.depth, 1)}
    del pipe
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", default="64,256")
    ap.add_argument("--step", default="0.5,0.25")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lanes", type=int, default=0, help="VadBatch(lanes=) (default: the engine's choice)")
    ap.add_argument("--precision", default="both", choices=["both", "f16x3", "f32"])
    ap.add_argument("--tau-offset", type=float, default=None,
                    help="hysteresis: measure every combination without and with this offset threshold, in this process, "
                         "in both build orders (without, with, with, without)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vad_streams.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    limit_host_threads()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    counts = [int(s) for s in args.streams.split(",")]
    steps = [float(s) for s in args.step.split(",")]
    seconds = (80000 + 16000 * max(steps) * (args.warmup + args.steps + 1)) / 16000.0
    audio = torch.from_numpy(synth_streams(max(counts), seconds, seed0=4242)).to(device)
    state = synth_segmentation_state()
    precs = ["f16x3", "f32"] if args.precision == "both" else [args.precision]
    runs = []
    for n in counts:
        for step in steps:
            for p in precs:
                offsets = [None] if args.tau_offset is None else [None, args.tau_offset, args.tau_offset, None]
                for off in offsets:
                    runs.append(one(n, step, p, args, audio, device, state, off))
                    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "vad_streams", "window_s": 5.0, "gpu": torch.cuda.get_device_name(device),
                      "runs": runs}))


if __name__ == "__main__":
    main()
