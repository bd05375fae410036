#!/usr/bin/env python
"""Config 3 (powerset segmentation + ECAPA-TDNN, BASELINE.json configs[2]) on the N-stream engine: N synthetic
streams, 5 s windows every 500 ms, through ``StreamBatch`` with a ``HipEcapaEmbedding`` (each stream's K speaker
rows embedded with their own batch geometry, ``HipEcapaEmbedding.forward_groups``) and the output tail, in both
precisions.  One JSON line:

    {"tool": "config3_streams", "streams": N, "runs": [{precision, xrt, ms_per_step, lanes, inflight,
     host_wait_s, host_work_s, mean_group_frames, ...}, ...]}

xRT = windows per second / 2 (a stream needs 2 windows per second of audio).  ``mean_group_frames``: the mean
per-group frame count T_g (``dz_ecapa_peek`` 8) over a few untimed steps after the timed region; every row is
laid out with the handle's 501 frames whatever its T_g.

    python tools/config3_streams.py [--streams 64] [--steps 40] [--warmup 10] [--lanes 0] [--precision both]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diart_amd.hostinfo import limit_host_threads  # noqa: E402
from diart_amd.models import HipEcapaEmbedding, HipSegmentation  # noqa: E402
from diart_amd.pipeline import StreamBatch  # noqa: E402
from diart_amd.synth import synth_ecapa_state, synth_segmentation_state, synth_streams  # noqa: E402


def one(precision, args, audio, device, seg_state, emb_state):
    n, hop, S = args.streams, 8000, 80000
    pipe = StreamBatch(HipSegmentation(seg_state, max_batch=n, powerset=True, precision=precision),
                       HipEcapaEmbedding(emb_state, precision=precision), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=device, tail=True, lanes=args.lanes or None)

    def run(t0, count):
        inflight = []
        for t in range(t0, t0 + count):
            inflight.append(pipe.launch(audio[:, t * hop:t * hop + S]))
            if len(inflight) >= pipe.max_inflight:
                pipe.finish(inflight.pop(0), want_scores=False)
        while inflight:
            pipe.finish(inflight.pop(0), want_scores=False)

    run(0, args.warmup)
    torch.cuda.synchronize(device)
    pipe.host_seconds = {"wait": 0.0, "work": 0.0}
    t0 = time.perf_counter()
    run(args.warmup, args.steps)
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0
    host = dict(pipe.host_seconds)
    # per-group frames of a few steps after the timed region (the peek synchronises: untimed)
    frames = []
    for t in range(args.warmup + args.steps, args.warmup + args.steps + 4):
        lane = pipe._t % pipe.depth
        pipe.finish(pipe.launch(audio[:, t * hop:t * hop + S]), want_scores=False)
        tg, _ = pipe.emb.peek_handle(pipe._sub[(S, lane)][1][0], 8)
        frames += tg.view(n, -1)[:, 0].tolist()
    return {"precision": precision, "xrt": round(n * args.steps / elapsed / 2, 2),
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "steps": args.steps, "warmup": args.warmup,
            "lanes": pipe.depth, "inflight": pipe.max_inflight,
            "host_wait_s": round(host["wait"], 4), "host_work_s": round(host["work"], 4),
            "mean_group_frames": round(sum(frames) / max(1, len(frames)), 1), "row_stride_frames": 1 + S // 160}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lanes", type=int, default=0, help="StreamBatch(lanes=) (default: the engine's choice)")
    ap.add_argument("--precision", default="both", choices=["both", "f16x3", "f32"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("config3_streams.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    limit_host_threads()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    seconds = (80000 + 8000 * (args.warmup + args.steps + 5)) / 16000.0
    audio = torch.from_numpy(synth_streams(args.streams, seconds, seed0=4242)).to(device)
    seg_state, emb_state = synth_segmentation_state(seed=77, powerset=True), synth_ecapa_state()
    precs = ["f16x3", "f32"] if args.precision == "both" else [args.precision]
    runs = [one(p, args, audio, device, seg_state, emb_state) for p in precs]
    print(json.dumps({"tool": "config3_streams", "streams": args.streams, "window_s": 5.0, "step_s": 0.5,
                      "gpu": torch.cuda.get_device_name(device), "runs": runs}))


if __name__ == "__main__":
    main()
