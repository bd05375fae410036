#!/usr/bin/env python
"""What the speaker gallery costs (``diart_amd.gallery``, ``csrc/k_gallery.hip``), in three parts; one JSON file.

``kernel``  ``dz_gallery_match`` alone (its three launches), timed by device events over ``--calls`` queued calls, for
            R = 192 rows (64 streams x 3 speakers), D in {192, 256, 512}, E in {1 024, 16 384, 65 536}: microseconds per
            call, gallery bytes and multiply-adds per second.  A gallery that fits the 256 MB last-level cache is read
            from there after the first call: ``fits_llc`` says so, and the byte rate of such a row is no HBM rate.
``engine``  ``StreamBatch`` at ``--streams`` streams with and without a 65 536-entry gallery: two engines in one
            process, measured in turn, ``--repeats`` runs of ``--steps`` steps; median and range of ms per step, and
            the host cost of ``SpeakerNames`` (update + labels) per step, timed apart on the arrays of a real step.
``bench``   ``python bench.py --gpus 1 --steps 20 --warmup 5`` on this tree and on a checkout of the parent commit
            (``--parent DIR``, built beforehand), child processes in turn, ``--bench-runs`` runs each: the default path
            (no gallery) against the spread of the parent's own repeats.

    python tools/gallery_bench.py [--parts kernel,engine,bench] [--parent _ab_old/parent] [--out profiles/rNN_gallery.json]
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from diart_amd.gallery import SpeakerGallery, SpeakerNames  # noqa: E402
from diart_amd.models import HipEmbedding, HipSegmentation  # noqa: E402
from diart_amd.pipeline import StreamBatch  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_streams  # noqa: E402

STEP, S, HOP = 0.5, 80000, 8000
LLC_BYTES = 256 << 20


def spread(values):
    return {"runs": values, "median": round(statistics.median(values), 4), "min": min(values), "max": max(values)}


def kernel_part(device, calls):
    rows, R = [], 192
    gen = torch.Generator().manual_seed(0)
    for D in (192, 256, 512):
        x = torch.randn(R, D, generator=gen).to(device)
        for E in (1024, 16384, 65536):
            gallery = SpeakerGallery([str(e) for e in range(E)], torch.randn(E, D, generator=gen), device)
            gallery.match(x)                                   # builds the handle; the first call
            out = torch.empty((3, R), dtype=torch.int32, device=device)
            h, st = gallery._handle, torch.cuda.current_stream(device).cuda_stream
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            start.record()
            for _ in range(calls):
                h.match(x.data_ptr(), D, R, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st)
            stop.record()
            stop.synchronize()
            us = 1e3 * start.elapsed_time(stop) / calls
            gbytes, macs = 4 * E * D, R * E * D
            rows.append({"R": R, "D": D, "E": E, "calls": calls, "us_per_call": round(us, 2),
                         "gallery_bytes": gbytes, "fits_llc": gbytes <= LLC_BYTES,
                         "gallery_gb_per_s": round(gbytes / us / 1e3, 1), "gmac_per_s": round(macs / us / 1e3, 1),
                         "tflop_per_s": round(2 * macs / us / 1e6, 2)})
            del gallery
    return rows


def run(pipe, audio, t0, count, keep=None):
    inflight = []
    for t in range(t0, t0 + count):
        inflight.append(pipe.launch(audio[:, t * HOP:t * HOP + S]))
        if len(inflight) >= pipe.max_inflight:
            ticket = inflight.pop(0)
            res = pipe.finish(ticket, want_scores=False)
            if keep is not None and "match" in ticket:
                keep.append((res[3].copy(), ticket["match"][0].copy(), ticket["match"][1].copy()))
    while inflight:
        pipe.finish(inflight.pop(0), want_scores=False)


def engine_part(device, n, steps, warmup, repeats, delta_id):
    seg_sd, emb_sd = synth_segmentation_state(), synth_embedding_state()
    audio = torch.from_numpy(synth_streams(n, (S + HOP * (warmup + steps)) / 16000.0, seed0=0)).to(device)
    E, D = 65536, 512
    gallery = SpeakerGallery([str(e) for e in range(E)], torch.randn(E, D, generator=torch.Generator().manual_seed(1)),
                             device)
    pipes = {}
    for name in ("plain", "gallery"):
        pipes[name] = StreamBatch(HipSegmentation(seg_sd, max_batch=n), HipEmbedding(emb_sd, max_batch=n), n,
                                  device=device, tail=True)
    pipes["gallery"].set_gallery(gallery, delta_id)
    recorded = []
    for name, pipe in pipes.items():                          # the warm run
        run(pipe, audio, 0, warmup, recorded if name == "gallery" else None)
    torch.cuda.synchronize(device)
    ms = {name: [] for name in pipes}
    for _ in range(repeats):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            run(pipe, audio, warmup, steps)
            torch.cuda.synchronize(device)
            ms[name].append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
    out = {"streams": n, "steps": steps, "warmup": warmup, "gallery_shape": {"E": E, "D": D, "delta_id": delta_id},
           "lanes": pipes["plain"].depth, "inflight": pipes["plain"].max_inflight,
           "handles_mb": round(pipes["plain"].depth * (4 * E * D + 3 * 4096 * (E // 128) * 4) / 2 ** 20, 1)}
    for name, v in ms.items():
        out[name] = dict(spread(v), xrt=round(n * STEP / (statistics.median(v) / 1e3), 1))
    out["gallery_inside_plain_spread"] = out["plain"]["min"] <= out["gallery"]["median"] <= out["plain"]["max"]
    # the host rule alone, on the (assign, index, distance) of real steps
    names = SpeakerNames(n, pipes["gallery"].max_speakers, delta_id)
    us = []
    for _ in range(200):
        assign, index, dist = recorded[len(us) % len(recorded)]
        t0 = time.perf_counter()
        names.update(assign, index, dist)
        names.labels(gallery.names)
        us.append(1e6 * (time.perf_counter() - t0))
    out["speaker_names_host_us_per_step"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1),
                                             "max": round(max(us), 1)}
    return out


def bench_part(parent, runs):
    trees = {"parent": Path(parent).resolve(), "this": ROOT}
    got = {name: [] for name in trees}
    scratch = Path(tempfile.mkdtemp(prefix="gallery_bench_"))       # the children's side files (bench.py --details)
    for i in range(runs):
        for name, tree in trees.items():
            details = scratch / f"{name}_{i}.json"
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--details",
                                str(details)], cwd=tree, capture_output=True, text=True, timeout=600)
            line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
            if r.returncode != 0 or line is None:
                got[name].append({"error": (r.stderr or r.stdout)[-300:]})
                continue
            d = json.loads(line)
            got[name].append({"value": d.get("value"), "ms_per_step": d.get("ms_per_step")})
            print(f"[bench] {name} run {i}: {d.get('value')} xRT", file=sys.stderr, flush=True)
    out = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5, child processes in turn (parent first)"}
    for name, v in got.items():
        vals = [x["value"] for x in v if x.get("value")]
        out[name] = {"runs": v, "median_xrt": statistics.median(vals) if vals else None,
                     "min_xrt": min(vals) if vals else None, "max_xrt": max(vals) if vals else None}
    p, t = out["parent"], out["this"]
    if p["median_xrt"] and t["median_xrt"]:
        out["this_inside_parent_spread"] = p["min_xrt"] <= t["median_xrt"] <= p["max_xrt"]
        out["this_over_parent"] = round(t["median_xrt"] / p["median_xrt"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,engine,bench")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--delta-id", type=float, default=0.3, help="a parameter of the measurement, no recommendation")
    ap.add_argument("--parent", default="_ab_old/parent", help="a built checkout of the parent commit")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    parts = args.parts.split(",")
    device = torch.device("cuda", 0)
    out = {"tool": "gallery_bench", "gpu": torch.cuda.get_device_name(0)}
    if "bench" in parts:                                      # first: child processes, before this one holds the GPU
        out["bench"] = bench_part(args.parent, args.bench_runs)
    if "kernel" in parts:
        out["kernel"] = kernel_part(device, args.calls)
    if "engine" in parts:
        out["engine"] = engine_part(device, args.streams, args.steps, args.warmup, args.repeats, args.delta_id)
    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
