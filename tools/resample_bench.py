"""Cost of the GPU resampler (DESIGN.md "Resampling"): for 8 / 22.05 / 32 / 44.1 / 48 kHz -> 16 kHz,
  * the kernel alone on 64 five-second windows: us per call (median of timed calls, CUDA events) and the fraction
    of the f32 vector peak (taps x outputs x 2 FLOP / time / 157.3 TFLOP/s),
  * one 30-minute file (one row),
  * StreamServer at 64 streams with 48 kHz and 44.1 kHz input beside the same server at 16 kHz: x real time
    (seconds of audio per stream x streams / wall seconds) over a run of steps after a warm-up.
Prints one JSON object; ``--out`` also writes it.

    python tools/resample_bench.py [--calls 50] [--steps 40] [--out profiles/resample_bench.json]
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

from diart_amd import _lib  # noqa: E402
from diart_amd import models as M  # noqa: E402
from diart_amd.functional import Resampler  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state  # noqa: E402

PEAK_F32 = 157.3e12
RATES = [8000, 22050, 32000, 44100, 48000]


def time_calls(fn, calls: int) -> float:
    """median seconds of one call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def kernel_rows(dev, calls):
    out = {}
    lib = _lib.load()
    for sr in RATES:
        rs = Resampler(sr, 16000, dev)
        p, t = _lib.C.c_int(), _lib.C.c_int()
        lib.dz_resample_geometry(sr, 16000, _lib.C.byref(p), _lib.C.byref(t), None, None)
        x = torch.rand((64, 5 * sr), device=dev) * 2 - 1
        y = torch.empty((64, 80000), device=dev)
        s = time_calls(lambda: rs.rows(x, y), calls)
        flop = 2.0 * t.value * 64 * 80000
        f = torch.rand((1, 1800 * sr), device=dev) * 2 - 1
        g = torch.empty((1, rs.out_len(1800 * sr)), device=dev)
        sf = time_calls(lambda: rs.rows(f, g), max(5, calls // 5))
        out[str(sr)] = {"phases": p.value, "taps": t.value, "windows64_us": round(s * 1e6, 2),
                        "windows64_peak_fraction": round(flop / s / PEAK_F32, 4),
                        "file30min_us": round(sf * 1e6, 1), "file30min_peak_fraction": round(
                            2.0 * t.value * g.shape[1] / sf / PEAK_F32, 4)}
    return out


def server_xrt(dev, rate, steps, streams=64):
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = synth_segmentation_state(), synth_embedding_state()
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=streams), M.HipEmbedding(emb_sd, max_batch=streams),
                       max_streams=streams, device=dev, input_sample_rate=rate)
    rng = np.random.default_rng(0)
    block = rate // 2
    audio = rng.uniform(-0.3, 0.3, (streams, block * (10 + steps + 1))).astype(np.float32)
    for s in range(streams):
        srv.open(s)
        srv.push(s, audio[s, :block * 10])       # one window + its first step each
    srv.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        lo = block * (10 + k)
        for s in range(streams):
            srv.push(s, audio[s, lo:lo + block])
        srv.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"input_rate": rate, "streams": streams, "steps": steps, "rings": srv.rings is not None,
            "xrt": round(streams * steps * 0.5 / wall, 1), "ms_per_step": round(wall / steps * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_rows(dev, a.calls),
           "server": [server_xrt(dev, r, a.steps) for r in (16000, 48000, 44100, 16000)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
