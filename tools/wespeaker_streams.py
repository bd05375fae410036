#!/usr/bin/env python
"""The WeSpeaker ResNet34 embedding on the N-stream engine (``WeSpeakerBatch``): N synthetic streams, 5 s windows every
500 ms, segmentation + embedding + clustering + output tail, in both precisions.  In the same process it times the two
things the engine is to be compared with, on the same windows: ``HipWeSpeakerEmbedding.forward_multi`` alone (the
trunk's alone-time; the engine's step cannot be shorter) and the blocks path (``SpeakerDiarization`` with the same
models, one call per N windows; the synchronous form of the same launches).  One JSON line:

    {"tool": "wespeaker_streams", "runs": [{streams, precision, recurrence, lanes, inflight, xrt, ms_per_step,
     ms_per_step_rounds, host_wait_s, host_work_s, engine_mb, engine_mb_per_lane}, ...],
     "forward_multi_alone": {precision: {ms_per_step_median, ms_per_step_wall}},
     "blocks_path": {precision: {ms_per_call, xrt}}}

xRT = windows per second x step.  ``--recurrence`` takes a list ("auto,valu"): the engines of one precision are timed
in alternating rounds, so that two recurrences are compared within one process.

    python tools/wespeaker_streams.py [--streams 64] [--lanes 2] [--recurrence auto,valu] [--precision both]
                                      [--steps 40] [--warmup 6] [--rounds 3] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diart_amd import models as M  # noqa: E402
from diart_amd.features import SlidingWindow, SlidingWindowFeature  # noqa: E402
from diart_amd.hostinfo import limit_host_threads  # noqa: E402
from diart_amd.pipeline import WeSpeakerBatch  # noqa: E402
from diart_amd.synth import synth_segmentation_state, synth_streams, synth_wespeaker_state  # noqa: E402

S, HOP, STEP = 80000, 8000, 0.5


def make_engine(n, precision, recurrence, args, device, states):
    torch.cuda.synchronize(device)
    free0 = torch.cuda.mem_get_info(device)[0]
    pipe = WeSpeakerBatch(M.HipSegmentation(states[0], max_batch=n, precision=precision),
                          M.HipWeSpeakerEmbedding(states[1], max_batch=n, precision=precision), n, tail=True,
                          device=device, lanes=args.lanes or None, recurrence=None if recurrence == "auto" else recurrence)
    return pipe, free0


def run_engine(pipe, audio, t0, count):
    inflight = []
    for t in range(t0, t0 + count):
        inflight.append(pipe.launch(audio[:pipe.n, t * HOP:t * HOP + S]))
        if len(inflight) >= pipe.max_inflight:
            pipe.finish(inflight.pop(0), want_scores=False)
    while inflight:
        pipe.finish(inflight.pop(0), want_scores=False)


def engines(n, precision, recurrences, args, audio, device, states):
    """Every arm's engine built and warmed, then ``rounds`` timed passes per arm, alternating."""
    arms = []
    for rec in recurrences:
        pipe, free0 = make_engine(n, precision, rec, args, device, states)
        run_engine(pipe, audio, 0, args.warmup)
        torch.cuda.synchronize(device)
        # device memory the engine took (every lane's handles + the in-flight slots; hipMalloc'd, outside torch's cache)
        arms.append(dict(pipe=pipe, asked=rec, engine_mb=(free0 - torch.cuda.mem_get_info(device)[0]) / 2**20, ms=[],
                         wait=0.0, work=0.0))
    for _ in range(args.rounds):
        for arm in arms:
            pipe = arm["pipe"]
            pipe.reset()
            pipe.host_seconds = {"wait": 0.0, "work": 0.0}
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run_engine(pipe, audio, args.warmup, args.steps)
            torch.cuda.synchronize(device)
            arm["ms"].append(1e3 * (time.perf_counter() - t0) / args.steps)
            arm["wait"] += pipe.host_seconds["wait"]
            arm["work"] += pipe.host_seconds["work"]
    out = []
    for arm in arms:
        pipe, ms = arm["pipe"], statistics.median(arm["ms"])
        out.append({"streams": n, "step_s": STEP, "precision": precision, "recurrence_asked": arm["asked"],
                    "recurrence": pipe.recurrence or "model", "lanes": pipe.depth, "inflight": pipe.max_inflight,
                    "xrt": round(n * STEP / (ms * 1e-3), 1), "ms_per_step": round(ms, 3),
                    "ms_per_step_rounds": [round(v, 3) for v in arm["ms"]], "steps": args.steps, "warmup": args.warmup,
                    "host_wait_s": round(arm["wait"] / args.rounds, 4), "host_work_s": round(arm["work"] / args.rounds, 4),
                    "engine_mb": round(arm["engine_mb"], 1), "engine_mb_per_lane": round(arm["engine_mb"] / pipe.depth, 1)})
    arms.clear()
    torch.cuda.empty_cache()
    return out


def forward_multi_alone(n, precision, args, audio, device, states):
    """forward_multi of the same n windows with K = 3 weight rows each: device events per call + the wall clock."""
    m = M.HipWeSpeakerEmbedding(states[1], max_batch=n, precision=precision).to(device)
    w = torch.rand(n, 3, 293, generator=torch.Generator().manual_seed(0)).to(device)
    x = audio[:n, None, :S]
    for _ in range(args.warmup):
        m.forward_multi(x, w, normalize=True)
    torch.cuda.synchronize(device)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        m.forward_multi(x, w, normalize=True)
        b.record()
    torch.cuda.synchronize(device)
    wall = 1e3 * (time.perf_counter() - t0) / args.steps
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"ms_per_step_median": round(ms[len(ms) // 2], 3), "ms_per_step_min": round(ms[0], 3),
            "ms_per_step_wall": round(wall, 3), "windows": n, "speakers": 3}


def blocks_path(n, precision, args, audio, device, states):
    """SpeakerDiarization with the same models, n windows per call (one of every synthetic stream, taken as n
    consecutive chunks): segmentation, embedding, then clustering + tail of the n chunks, synchronous."""
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(states[0], max_batch=n, precision=precision),
        embedding=M.EmbeddingModel.from_state(states[1], max_batch=n, precision=precision), latency=STEP, device=device)
    pipe = SpeakerDiarization(cfg)
    host = audio[:n].cpu().numpy()
    calls = args.warmup + args.steps

    def batch(t):
        return [SlidingWindowFeature(host[j, t * HOP:t * HOP + S, None],
                                     SlidingWindow(start=(t * n + j) * STEP, duration=1 / 16000, step=1 / 16000))
                for j in range(n)]

    batches = [batch(t) for t in range(calls)]
    for t in range(args.warmup):
        pipe(batches[t])
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for t in range(args.warmup, calls):
        pipe(batches[t])
    torch.cuda.synchronize(device)
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    return {"ms_per_call": round(ms, 3), "windows_per_call": n, "xrt": round(n * STEP / (ms * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", default="64")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3, help="timed passes per engine, alternating between the engines")
    ap.add_argument("--lanes", type=int, default=0, help="WeSpeakerBatch(lanes=) (default: the engine's choice)")
    ap.add_argument("--recurrence", default="auto", help="list of WeSpeakerBatch(recurrence=): auto | valu | 0 | 3 | 4")
    ap.add_argument("--precision", default="both", choices=["both", "f16x3", "f32"])
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wespeaker_streams.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    limit_host_threads()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    counts = [int(s) for s in args.streams.split(",")]
    seconds = (S + HOP * (args.warmup + args.steps + 1)) / 16000.0
    audio = torch.from_numpy(synth_streams(max(counts), seconds, seed0=4242)).to(device)
    states = (synth_segmentation_state(), synth_wespeaker_state())
    precs = ["f16x3", "f32"] if args.precision == "both" else [args.precision]
    recs = [r.strip() for r in args.recurrence.split(",") if r.strip()]
    runs, alone, blocks = [], {}, {}
    for n in counts:
        for p in precs:
            # (the recurrence is a choice of the split-f16 segmentation only)
            for r in engines(n, p, recs if p == "f16x3" else ["auto"], args, audio, device, states):
                runs.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
            alone[f"{p}/{n}"] = forward_multi_alone(n, p, args, audio, device, states)
            blocks[f"{p}/{n}"] = blocks_path(n, p, args, audio, device, states)
            print(json.dumps({"forward_multi_alone": alone[f"{p}/{n}"], "blocks_path": blocks[f"{p}/{n}"]}),
                  file=sys.stderr, flush=True)
    line = json.dumps({"tool": "wespeaker_streams", "window_s": 5.0, "gpu": torch.cuda.get_device_name(device),
                       "runs": runs, "forward_multi_alone": alone, "blocks_path": blocks})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
