"""Time ``HipWeSpeakerEmbedding.forward_multi`` (WeSpeaker ResNet34) at 64 chunks x K = 3 speakers of 5 s in both
arithmetic modes and write one JSON file under profiles/.

    python tools/wespeaker_bench.py [--chunks 64] [--steps 20] [--warmup 5] [--out profiles/wespeaker_bench.json]

Algorithmic FLOPs are counted from the layer shapes (2 per multiply-add; the trunk is the 3x3 / 1x1 convolutions of
layers 1 - 4 plus conv1).  Run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel table
(tools/wespeaker_kstats.py turns that into TFLOP/s per kernel)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK = {"f16x3": 833.0, "f32": 157.0}       # TFLOP/s: split products on the f16 pipe / exact-f32 MFMA


def trunk_flops(num_samples: int) -> dict:
    """FLOPs per row of every convolution stage (2 per MAC)."""
    from diart_amd import _lib
    lib = _lib.load()
    T = [lib.dz_wsp_frames_for(num_samples, s) for s in range(5)]
    out = {"conv1": 2 * 80 * T[0] * 32 * 9}
    cin = 32
    for li, nb in enumerate((3, 4, 6, 3)):
        c, F, Tl = 32 << li, 80 >> li, T[li + 1]
        pos = F * Tl
        fl = 0
        for j in range(nb):
            fl += 2 * pos * c * 9 * (cin if j == 0 else c)        # conv1 of the block (strided on j == 0)
            fl += 2 * pos * c * 9 * c                              # conv2
            if j == 0 and li > 0:
                fl += 2 * pos * c * cin                           # 1x1 shortcut
            cin = c
        out[f"layer{li + 1}"] = fl
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wespeaker_bench.json"))
    a = ap.parse_args()

    import torch
    from diart_amd.models import HipWeSpeakerEmbedding
    from diart_amd.synth import synth_streams, synth_wespeaker_state
    dev = torch.device("cuda", 0)
    S = int(round(a.seconds * 16000))
    x = torch.from_numpy(synth_streams(a.chunks, a.seconds + 0.01, seed0=1))[:, None, :S].contiguous().to(dev)
    w = torch.rand(a.chunks, a.speakers, 293, generator=torch.Generator().manual_seed(0)).to(dev)
    flops = trunk_flops(S)
    trunk = sum(flops.values())
    head = 2 * a.chunks * a.speakers * 5120 * 256
    res = {"workload": f"forward_multi {a.chunks} chunks x K={a.speakers}, {a.seconds:g} s",
           "device": torch.cuda.get_device_name(0), "gflop_per_row": {k: v / 1e9 for k, v in flops.items()},
           "gflop_per_step": (a.chunks * trunk + head) / 1e9, "results": {}}
    for prec in a.precisions.split(","):
        m = HipWeSpeakerEmbedding(synth_wespeaker_state(), max_batch=a.chunks, precision=prec).to(dev)
        for _ in range(a.warmup):
            m.forward_multi(x, w, normalize=True)
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        t0 = time.perf_counter()
        for s, e in ev:
            s.record()
            m.forward_multi(x, w, normalize=True)
            e.record()
        torch.cuda.synchronize(dev)
        wall = (time.perf_counter() - t0) / a.steps * 1e3
        ms = sorted(s.elapsed_time(e) for s, e in ev)
        med = ms[len(ms) // 2]
        tf = a.chunks * trunk / (med * 1e-3) / 1e12
        res["results"][prec] = {"ms_per_step_median": med, "ms_per_step_min": ms[0], "ms_per_step_wall": wall,
                                "trunk_tflops": tf, "fraction_of_peak": tf / PEAK[prec], "peak_tflops": PEAK[prec]}
        print(prec, json.dumps(res["results"][prec]))
        del m
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
