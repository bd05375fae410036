"""What the form of the clients' audio costs a ``StreamServer`` (DESIGN.md "Raw client audio"): 64 streams, 5 s / 500 ms,
the ``pyannote/embedding`` pair, one process.  One row per input form — sample rate, ``input_format``,
``input_channels``, ``device_rings`` — with x real time (seconds of audio per stream x streams / wall seconds),
milliseconds per step and the bytes a step uploads (ring mode: the new block of every stream as the client sent it;
host-window mode: every stream's whole float32 window).  Each figure is the median of ``--runs`` runs of ``--steps``
steps after a warm-up.  Prints one JSON object; ``--out`` also writes it.

    python tools/ingest_streams.py [--steps 40] [--runs 3] [--out profiles/r12a_ingest_streams.json]

``--rows 0,3`` runs a subset (rows 0 and 3 use nothing but ``input_sample_rate``).  Rows 7 - 11 are the telephone
forms: 8 kHz float32, 16-bit, mu-law, stereo A-law, and 8-bit at 16 kHz.

``--kernel`` adds the ring kernels alone: per-row pushes of 64 rows of 4 000 frames (500 ms at 8 kHz) already on the
device, as mu-law bytes and as float32; the lock-step push of 64 x 8 000 float32 from device memory and from mapped
pinned memory; the gather of 64 windows of 80 000.  ``--calls`` calls between two device events that wait behind a long
matrix product, so the launches are queued before the first one runs and the interval is the GPU's; microseconds per
call (median of 5) and the bytes read and written over that time.

``--parent-tree DIR`` (a checkout of the parent commit with its library built) adds row 0 alone in a child process,
this tree's and that tree's in turn, twice, in the same visit (``--tree`` is the checkout a child imports from); with
``--kernel`` the children time the ring kernels too.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

# (input rate, format, channels, device_rings)
ROWS = [(16000, "f32", 1, True), (48000, "f32", 1, True), (16000, "s16", 1, True), (48000, "s16", 2, True),
        (44100, "f32", 1, True), (44100, "f32", 1, "all"), (44100, "s16", 2, "all"),
        (8000, "f32", 1, True), (8000, "s16", 1, True), (8000, "ulaw", 1, True), (8000, "alaw", 2, True),
        (16000, "u8", 1, True)]


def encode(audio, fmt):
    """float audio in [-1, 1] -> values of ``fmt`` (G.711: the code whose decoded value is nearest)."""
    if fmt == "f32":
        return audio
    if fmt == "s16":
        return np.round(audio * 32767).astype(np.int16)
    if fmt == "u8":
        return np.round(audio * 127 + 128).astype(np.uint8)
    from diart_amd.pcm import alaw_expand, ulaw_expand
    linear = (ulaw_expand if fmt == "ulaw" else alaw_expand)(np.arange(256))
    order = np.argsort(linear, kind="stable")
    levels = linear[order].astype(np.float32)
    v = audio * np.float32(32768.0)
    hi = np.clip(np.searchsorted(levels, v), 1, 255)
    return order[np.where(v - levels[hi - 1] <= levels[hi] - v, hi - 1, hi)].astype(np.uint8)


def run_row(dev, rate, fmt, channels, rings, steps, runs, streams=64):
    from diart_amd import models as M
    from diart_amd.serve import StreamServer
    from diart_amd.synth import synth_embedding_state, synth_segmentation_state
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
    audio = encode(audio, fmt).reshape(streams, total * channels)
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
    itemsize = audio.dtype.itemsize
    upload = streams * (bv * itemsize if srv.rings is not None else srv.chunk_samples * 4)
    return {"input_rate": rate, "format": fmt, "channels": channels, "device_rings": rings,
            "rings": srv.rings is not None, "streams": streams, "steps": steps, "runs": runs,
            "xrt": round(streams * steps * 0.5 / wall, 1), "ms_per_step": round(wall / steps * 1e3, 3),
            "xrt_runs": [round(streams * steps * 0.5 / w, 1) for w in walls], "upload_bytes_per_step": upload}


def push_kernel(dev, calls, rows=64, hop=4000):
    """The ring kernels alone.  Per-row pushes of ``rows`` x ``hop`` frames from device memory, as mu-law bytes and as
    float32; the lock-step push of ``rows`` x 8 000 float32 from device memory and from mapped pinned memory; the gather
    of ``rows`` windows of 80 000.  Each: ``calls`` calls queued behind a long matrix product, between two device
    events, microseconds per call, 5 runs."""
    from diart_amd.pipeline import AudioRing
    rng = np.random.default_rng(1)
    big = torch.randn(8192, 8192, device=dev)
    idx = list(range(rows))

    def timed(call, bytes_read, bytes_written):
        for _ in range(20):
            call()
        us = []
        for _ in range(5):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(6):
                big @ big                       # the launches below are queued while this runs
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / calls)
        t = float(np.median(us))
        return {"us_per_call": round(t, 3), "us_runs": [round(u, 3) for u in us], "bytes_read": bytes_read,
                "bytes_written": bytes_written, "bytes_per_s": round((bytes_read + bytes_written) / (t * 1e-6), 1)}

    out = {}
    blocks = {"ulaw": torch.from_numpy(rng.integers(0, 256, (rows, hop), dtype=np.uint8)).to(dev),
              "f32": torch.from_numpy(rng.uniform(-1, 1, (rows, hop)).astype(np.float32)).to(dev)}
    for fmt, blk in blocks.items():
        ring = AudioRing(rows, 10 * hop, hop, slack_blocks=0, device=dev)
        kw = {} if fmt == "f32" else {"format": fmt}
        # the block read once, every sample written twice
        out[fmt] = timed(lambda: ring.push_rows(blk, idx, **kw), rows * hop * blk.element_size(), rows * hop * 8)
    W, step = 80000, 8000
    host = torch.from_numpy(rng.uniform(-1, 1, (rows, step)).astype(np.float32))
    for name, blk in (("lock_step_device", host.to(dev)), ("lock_step_pinned", host.pin_memory())):
        ring = AudioRing(rows, W, step, device=dev)
        out[name] = timed(lambda: ring.push(blk), rows * step * 4, rows * step * 8)
    batch = torch.empty(rows, W, device=dev)
    out["gather"] = timed(lambda: ring.gather(idx, batch), rows * W * 4, rows * W * 4)      # (the ring is full by now)
    return {"rows": rows, "frames_per_row": hop, "lock_step_hop": step, "gather_window": W, "calls": calls, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=str, default=None, help="comma-separated row numbers (default: all)")
    ap.add_argument("--kernel", action="store_true", help="also time the ring kernels alone")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--tree", type=str, default=str(Path(__file__).resolve().parent.parent),
                    help="the checkout diart_amd is imported from")
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    dev = torch.device("cuda", 0)
    pick = range(len(ROWS)) if a.rows is None else [int(i) for i in a.rows.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "rows": [run_row(dev, *ROWS[i], a.steps, a.runs) for i in pick]}
    if a.kernel:
        res["push_kernel"] = push_kernel(dev, a.calls)
    if a.parent_tree:
        # row 0 (16 kHz float32 mono, the default path) with a process to itself: fresh child processes (this one
        # keeps its GPU state), this tree and the parent's in turn, twice; a child's last line is its JSON object
        def alone(tree):
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--tree", tree, "--rows", "0",
                                "--steps", str(a.steps), "--runs", str(a.runs), "--calls", str(a.calls)]
                               + (["--kernel"] if a.kernel else []), capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"the run of {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            return json.loads(r.stdout.strip().splitlines()[-1])

        here, parent = [], []
        for _ in range(2):
            here.append(alone(a.tree))
            parent.append(alone(a.parent_tree))
        rows_of = {"this_tree": [r["rows"][0] for r in here], "parent_tree": [r["rows"][0] for r in parent]}
        res["default_row_alone"] = {**rows_of, "xrt_runs": {k: [x for r in v for x in r["xrt_runs"]]
                                                            for k, v in rows_of.items()}}
        if a.kernel:
            res["ring_kernels_alone"] = {"this_tree": [r["push_kernel"] for r in here],
                                         "parent_tree": [r["push_kernel"] for r in parent]}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
