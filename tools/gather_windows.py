#!/usr/bin/env python
"""`dz_gather_windows` alone against the torch copies it replaces in `FileBatch`: one step's stage of `--rows` windows
of 80 000 samples from `--runs` files (consecutive windows 8 000 samples apart), `--iters` queued repetitions timed by
device events.  One JSON line: microseconds per step's stage and TB/s (bytes read + bytes written) for both."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diart_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--runs", type=int, default=16)
ap.add_argument("--iters", type=int, default=200)
args = ap.parse_args()
S, HOP = 80000, 8000
dev = torch.device("cuda", 0)
lib, ctx = _lib.load(), _lib.context(0)
per = args.rows // args.runs
audio = [torch.randn(S + HOP * (per - 1), device=dev) for _ in range(args.runs)]
stage = torch.empty((args.rows, S), device=dev)
table = (_lib.WindowRun * args.runs)()
for i, (t, a) in enumerate(zip(table, audio)):
    t.src, t.row0, t.count = a.data_ptr(), i * per, per
stream = torch.cuda.current_stream(dev).cuda_stream


def kernel():
    _lib.check(lib.dz_gather_windows(ctx, table, args.runs, S, HOP, stage.data_ptr(), stage.stride(0), args.rows, stream),
               "dz_gather_windows")


def copies():
    for i, a in enumerate(audio):
        stage[i * per:(i + 1) * per].copy_(a.unfold(0, S, HOP), non_blocking=True)


def timed(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / args.iters


copies()
want = stage.clone()
stage.zero_()
kernel()
torch.cuda.synchronize()
assert torch.equal(stage, want), "the kernel's stage differs from the copies'"
nbytes = 2 * 4 * args.rows * S
out = {"rows": args.rows, "runs": args.runs, "samples": S, "hop": HOP, "iters": args.iters, "bytes_moved": nbytes}
for name, fn in (("gather_kernel", kernel), ("torch_copies", copies), ("gather_kernel_again", kernel)):
    us = timed(fn)
    out[name] = {"us": round(us, 2), "TB_per_s": round(nbytes / us / 1e6, 3)}
print(json.dumps(out), flush=True)
