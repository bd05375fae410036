#!/usr/bin/env python
"""What the cohort costs (adaptive s-norm of the gallery match: ``diart_amd.gallery``, ``csrc/k_cohort.hip``), in three
parts; one JSON file.

``kernel``  by device events over ``--calls`` queued calls, at R = 192 rows (64 streams x 3 speakers), D = 256,
            E = 65 536 voiceprints, a cohort of M = 4 096 and top_n = 300: ``dz_gallery_cohort_stats`` alone (the norm,
            the distance tile and the selection), ``dz_gallery_match_norm`` and ``dz_gallery_match`` on the same handle:
            microseconds per call.  The kernels are latency-sized at these shapes (the cohort is 4 MB, the distances of a
            pass 3 MB, all of it cache-resident after the first call): no bandwidth figure is formed.
``engine``  ``StreamBatch`` at ``--streams`` streams without a gallery, with a raw gallery (65 536 x 512) and with the
            same gallery and a cohort of 4 096: three engines in one process, measured in turn, ``--repeats`` runs of
            ``--steps`` steps; median and range of ms per step.
``bench``   ``python bench.py --gpus 1 --steps 20 --warmup 5`` on this tree and on a checkout of the parent commit
            (``--parent DIR``, built beforehand), child processes in turn, ``--bench-runs`` runs each: the default path
            launches nothing new, so this tree's median must lie inside the spread of the parent's own repeats.

Expected, written before the first run and derived from the code, not measured:
  * the statistics alone: three launches of a few microseconds of work each.  The tile kernel runs 3 x 32 = 96
    workgroups of 8 k-tiles (under one wave of the 256 CUs), the selection 192 workgroups that each walk 4 096 LDS
    words five times.  Launch-bound: 20 - 60 us per call.
  * ``match_norm`` = ``match`` + the statistics + an epilogue of seven more float operations and two more loads per
    (row, voiceprint) pair beside 128 MFMAs of 64 cycles per wave: under 5 % of the tile.  With ``match`` at about 85 us
    (profiles/r28a_gallery.json): 110 - 150 us.
  * the engine: the normalised gallery costs the raw gallery's step plus about 0.05 ms (the statistics at D = 512 on the
    stream that carries the results to the host); the plain engine is untouched.

What came of them: profiles/r31a_cohort.json and DESIGN.md 4.20 (the two kernel figures held; the engine's did not: the
normalised engine measured faster than the raw one, in either build order: ``--engine-order``).

    python tools/cohort_bench.py [--parts kernel,engine,bench] [--parent _ab_old/parent] [--out profiles/rNN_cohort.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from gallery_bench import HOP, S, STEP, bench_part, run, spread  # noqa: E402
from diart_amd.gallery import SpeakerGallery  # noqa: E402
from diart_amd.models import HipEmbedding, HipSegmentation  # noqa: E402
from diart_amd.pipeline import StreamBatch  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_streams  # noqa: E402

EXPECTED = {"cohort_stats_us": [20, 60], "match_norm_us": [110, 150], "engine_normalised_minus_raw_ms": 0.05}


def timed(device, calls, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return round(1e3 * start.elapsed_time(stop) / calls, 2)


def kernel_part(device, calls, repeats):
    R, D, E, M, top_n = 192, 256, 65536, 4096, 300
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(R, D, generator=gen).to(device)
    gallery = SpeakerGallery([str(e) for e in range(E)], torch.randn(E, D, generator=gen), device,
                             cohort=torch.randn(M, D, generator=gen), top_n=top_n)
    t0 = time.perf_counter()
    gallery.match_normalised(x)                                # builds the handle: the E voiceprints' statistics
    torch.cuda.synchronize(device)
    set_up = time.perf_counter() - t0
    out = torch.empty((3, R), dtype=torch.int32, device=device)
    h, st = gallery._handle, torch.cuda.current_stream(device).cuda_stream
    o = [out[i].data_ptr() for i in range(3)]
    fns = {"cohort_stats": lambda: h.cohort_stats(x.data_ptr(), D, R, o[0], o[1], st),
           "match_norm": lambda: h.match_norm(x.data_ptr(), D, R, *o, st),
           "match": lambda: h.match(x.data_ptr(), D, R, *o, st)}
    us = {name: [] for name in fns}
    for _ in range(repeats):                                   # in turn, so a drift of the clocks hits all three
        for name, fn in fns.items():
            us[name].append(timed(device, calls, fn))
    res = {"R": R, "D": D, "E": E, "M": M, "top_n": top_n, "calls": calls,
           "handle_with_cohort_seconds": round(set_up, 3)}
    for name, v in us.items():
        res[name + "_us"] = spread(v)
    res["match_norm_minus_match_us"] = round(res["match_norm_us"]["median"] - res["match_us"]["median"], 2)
    return res


def engine_part(device, n, steps, warmup, repeats, order):
    seg_sd, emb_sd = synth_segmentation_state(), synth_embedding_state()
    audio = torch.from_numpy(synth_streams(n, (S + HOP * (warmup + steps)) / 16000.0, seed0=0)).to(device)
    E, D, M = 65536, 512, 4096
    gen = torch.Generator().manual_seed(1)
    raw = SpeakerGallery([str(e) for e in range(E)], torch.randn(E, D, generator=gen), device)
    normalised = raw.with_cohort(torch.randn(M, D, generator=gen), top_n=300)
    pipes = {name: StreamBatch(HipSegmentation(seg_sd, max_batch=n), HipEmbedding(emb_sd, max_batch=n), n, device=device,
                               tail=True) for name in order}
    pipes["raw"].set_gallery(raw, 0.3)                         # the thresholds are parameters of the measurement
    pipes["normalised"].set_gallery(normalised, -5.0)
    for pipe in pipes.values():
        run(pipe, audio, 0, warmup)
    torch.cuda.synchronize(device)
    ms = {name: [] for name in pipes}
    for _ in range(repeats):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            run(pipe, audio, warmup, steps)
            torch.cuda.synchronize(device)
            ms[name].append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
    out = {"streams": n, "steps": steps, "warmup": warmup, "order": list(order), "gallery": {"E": E, "D": D},
           "cohort": {"M": M, "top_n": 300},
           "lanes": pipes["plain"].depth, "inflight": pipes["plain"].max_inflight}
    for name, v in ms.items():
        out[name] = dict(spread(v), xrt=round(n * STEP / (statistics.median(v) / 1e3), 1))
    out["normalised_minus_raw_ms"] = round(out["normalised"]["median"] - out["raw"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,engine,bench")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engine-order", default="plain,raw,normalised",
                    help="the order in which the three engines are built and measured in turn")
    ap.add_argument("--parent", default="_ab_old/parent", help="a built checkout of the parent commit")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    parts = args.parts.split(",")
    device = torch.device("cuda", 0)
    out = {"tool": "cohort_bench", "gpu": torch.cuda.get_device_name(0), "expected_before_the_first_run": EXPECTED}
    if "bench" in parts:                                       # first: child processes, before this one holds the GPU
        out["bench"] = bench_part(args.parent, args.bench_runs)
    if "kernel" in parts:
        out["kernel"] = kernel_part(device, args.calls, args.repeats)
    if "engine" in parts:
        out["engine"] = engine_part(device, args.streams, args.steps, args.warmup, args.repeats,
                                    tuple(args.engine_order.split(",")))
    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
