"""Cost of the volume adjustment (DESIGN.md "Volume adjustment"):
  * ``dz_adjust_volume`` alone, in place, on 64 x 80 000 and 256 x 80 000 mono rows (five-second windows at 16 kHz) and
    on 64 x 110 250 (44.1 kHz: every other row starts 8 bytes off a 16-byte boundary): us per call (a warm call
    first, then the median of the timed calls, device events) — once on ONE buffer (its rows stay in the 256 MiB
    Infinity Cache between calls) and once rotating over enough buffers that no call finds its rows cached — and
    beside each the bytes a call has to move (every sample read once and written once, 8 bytes; the second pass's
    re-read is meant to come from cache) over the time, as a fraction of the 8 TB/s HBM peak,
  * ``StreamServer`` at 64 streams with ``volume_in_db=-20`` and with ``None``: two servers in one process, a warm run
    each, then ``--rounds`` alternating runs of ``--steps`` steps: x real time and ms per step of every run,
  * with ``--parent-tree DIR`` (a checkout of the parent commit with its library built): the ``None`` server alone in
    a child process, this tree's and that tree's in turn, twice, ``--rounds`` runs each, in the same visit.
Prints one JSON object; ``--out`` also writes it.

    python tools/volume_bench.py [--calls 50] [--steps 40] [--rounds 3] [--parent-tree DIR] [--out profiles/<id>_volume.json]
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

HBM_PEAK = 8.0e12                       # bytes / s (spec; about 6.3e12 is reachable)
SHAPES = [(64, 80000), (256, 80000), (64, 110250)]
COLD_BYTES = 768 << 20                  # rotate over at least this much: three times the Infinity Cache


def time_each(fns, calls: int) -> float:
    """median seconds of one call; call i runs fns[i % len(fns)], every function once before the clock starts"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = []
    for i in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fns[i % len(fns)]()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def kernel_rows(dev, calls: int, target: float):
    from diart_amd.functional import adjust_volume_rows
    out = {}
    for rows, samples in SHAPES:
        nbytes = rows * samples * 4
        n = max(2, -(-COLD_BYTES // nbytes))
        bufs = [torch.rand((rows, samples), device=dev) * 0.6 - 0.3 for _ in range(n)]
        assert bufs[0].stride(0) == samples
        moved = 2.0 * nbytes

        def call(x):
            return lambda: adjust_volume_rows(x, target, out=x)

        warm = time_each([call(bufs[0])], calls)
        cold = time_each([call(x) for x in bufs], max(calls, 2 * n))
        out[f"{rows}x{samples}"] = {
            "bytes_moved": int(moved), "row_base_alignment_bytes": 16 if samples % 4 == 0 else (8 if samples % 2 == 0 else 4),
            "one_buffer_us": round(warm * 1e6, 2), "one_buffer_hbm_fraction": round(moved / warm / HBM_PEAK, 4),
            "rotating_buffers": n, "rotating_us": round(cold * 1e6, 2),
            "rotating_hbm_fraction": round(moved / cold / HBM_PEAK, 4)}
        del bufs
        torch.cuda.empty_cache()
    return out


class ServerRun:
    """A StreamServer at ``streams`` streams fed one block per stream and step."""

    def __init__(self, dev, streams: int, volume_in_db, total_steps: int):
        from diart_amd import models as M
        from diart_amd.serve import StreamServer
        from diart_amd.synth import synth_embedding_state, synth_segmentation_state
        kw = {} if volume_in_db is None else {"volume_in_db": volume_in_db}      # (the parent's server has no such argument)
        self.srv = StreamServer(M.HipSegmentation(synth_segmentation_state(), max_batch=streams),
                                M.HipEmbedding(synth_embedding_state(), max_batch=streams), max_streams=streams,
                                device=dev, **kw)
        self.streams, self.block, self.at = streams, 8000, 10
        rng = np.random.default_rng(0)
        self.audio = rng.uniform(-0.3, 0.3, (streams, self.block * (10 + total_steps))).astype(np.float32)
        for s in range(streams):
            self.srv.open(s)
            self.srv.push(s, self.audio[s, :self.block * 10])       # one window each
        self.srv.drain()
        torch.cuda.synchronize()

    def run(self, steps: int) -> dict:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            lo = self.block * self.at
            for s in range(self.streams):
                self.srv.push(s, self.audio[s, lo:lo + self.block])
            self.srv.step()
            self.at += 1
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return {"xrt": round(self.streams * steps * 0.5 / wall, 1), "ms_per_step": round(wall / steps * 1e3, 3)}


def server_rows(dev, steps: int, rounds: int, targets, streams: int = 64):
    runs = {str(t): ServerRun(dev, streams, t, steps * (rounds + 1)) for t in targets}
    for r in runs.values():
        r.run(steps)                                                 # warm
    out = {k: [] for k in runs}
    for _ in range(rounds):
        for k, r in runs.items():                                    # alternating
            out[k].append(r.run(steps))
    return {"streams": streams, "steps": steps, "rings": next(iter(runs.values())).srv.rings is not None, "runs": out,
            "median_ms_per_step": {k: float(np.median([x["ms_per_step"] for x in v])) for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target", type=float, default=-20.0)
    ap.add_argument("--tree", type=str, default=str(Path(__file__).resolve().parent.parent),
                    help="the checkout diart_amd is imported from")
    ap.add_argument("--server-none-only", action="store_true", help="only the server with volume_in_db=None")
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    dev = torch.device("cuda", 0)
    if a.server_none_only:
        print(json.dumps(server_rows(dev, a.steps, a.rounds, [None])))
        return
    res = {"device": torch.cuda.get_device_name(0), "target_db": a.target, "hbm_peak_bytes_per_s": HBM_PEAK,
           "kernel_in_place": kernel_rows(dev, a.calls, a.target),
           "server": server_rows(dev, a.steps, a.rounds, [None, a.target])}
    if a.parent_tree:
        # the two servers above share one process (two engines, two sets of host threads); the comparison with the
        # parent is between servers that each have a process to themselves: fresh child processes (this one keeps
        # its GPU state), this tree and the parent's in turn, twice; a child's last line is its JSON object
        def alone(tree):
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--tree", tree, "--server-none-only",
                                "--steps", str(a.steps), "--rounds", str(a.rounds)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"the run of {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            return json.loads(r.stdout.strip().splitlines()[-1])["runs"]["None"]

        here, parent = [], []
        for _ in range(2):
            here += alone(a.tree)
            parent += alone(a.parent_tree)
        res["server_none_alone"] = {"this_tree": here, "parent_tree": parent, "median_ms_per_step": {
            "this_tree": float(np.median([x["ms_per_step"] for x in here])),
            "parent_tree": float(np.median([x["ms_per_step"] for x in parent]))}}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
