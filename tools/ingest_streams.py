"""What the form of the clients' audio costs a ``StreamServer`` (DESIGN.md "Raw client audio"): 64 streams, 5 s / 500 ms,
the ``pyannote/embedding`` pair, one process.  One row per input form — sample rate, ``input_format``,
``input_channels``, ``device_rings`` — with x real time (seconds of audio per stream x streams / wall seconds),
milliseconds per step and the bytes a step uploads (ring mode: the new block of every stream as the client sent it;
host-window mode: every stream's whole float32 window).  Each figure is the median of ``--runs`` runs of ``--steps``
steps after a warm-up.  Prints one JSON object; ``--out`` also writes it.

    python tools/ingest_streams.py [--steps 40] [--runs 3] [--out profiles/r12a_ingest_streams.json]

``--rows 0,3`` runs a subset (rows 0 and 3 use nothing but ``input_sample_rate``).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diart_amd import models as M  # noqa: E402
from diart_amd.serve import StreamServer  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state  # noqa: E402

# (input rate, format, channels, device_rings)
ROWS = [(16000, "f32", 1, True), (48000, "f32", 1, True), (16000, "s16", 1, True), (48000, "s16", 2, True),
        (44100, "f32", 1, True), (44100, "f32", 1, "all"), (44100, "s16", 2, "all")]


def run_row(dev, rate, fmt, channels, rings, steps, runs, streams=64):
    kw = {}
    if (fmt, channels) != ("f32", 1):
        kw.update(input_format=fmt, input_channels=channels)
    if rings is not True:
        kw.update(device_rings=rings)
    if rate != 16000:
        kw.update(input_sample_rate=rate)
    seg_sd, emb_sd = synth_segmentation_state(), synth_embedding_state()
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=streams), M.HipEmbedding(emb_sd, max_batch=streams),
                       max_streams=streams, device=dev, **kw)
    rng = np.random.default_rng(0)
    block = rate // 2
    total = block * (10 + runs * steps)
    audio = rng.uniform(-0.3, 0.3, (streams, total, channels)).astype(np.float32)
    if fmt == "s16":
        audio = np.round(audio * 32767).astype(np.int16)
    audio = audio.reshape(streams, total * channels)
    bv = block * channels
    for s in range(streams):
        srv.open(s)
        srv.push(s, audio[s, :bv * 10])          # one window each
    srv.drain()
    walls = []
    for r in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            lo = bv * (10 + r * steps + k)
            for s in range(streams):
                srv.push(s, audio[s, lo:lo + bv])
            srv.step()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    wall = float(np.median(walls))
    itemsize = 2 if fmt == "s16" else 4
    upload = streams * (bv * itemsize if srv.rings is not None else srv.chunk_samples * 4)
    return {"input_rate": rate, "format": fmt, "channels": channels, "device_rings": rings,
            "rings": srv.rings is not None, "streams": streams, "steps": steps, "runs": runs,
            "xrt": round(streams * steps * 0.5 / wall, 1), "ms_per_step": round(wall / steps * 1e3, 3),
            "xrt_runs": [round(streams * steps * 0.5 / w, 1) for w in walls], "upload_bytes_per_step": upload}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=str, default=None, help="comma-separated row numbers (default: all)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pick = range(len(ROWS)) if a.rows is None else [int(i) for i in a.rows.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "rows": [run_row(dev, *ROWS[i], a.steps, a.runs) for i in pick]}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
