"""Per-kernel summary of a ``rocprofv3 --kernel-trace --stats --output-format csv`` run of tools/wespeaker_bench.py:
time share and algorithmic TFLOP/s of every WeSpeaker kernel against the peak of its arithmetic (833 TFLOP/s for
split-f16 products, 157 TFLOP/s exact f32).

    python tools/wespeaker_kstats.py <kernel_stats.csv> [--chunks 64] [--seconds 5] [--out summary.md]

The conv kernels are told apart by their tile (template arguments): the tile follows Cout, so each instance serves
one stage — Cout 32: layer 1 (6 launches per forward), 64: layer 2 (9), 128 / 256: layers 3 + 4 (13 + 7)."""
from __future__ import annotations

import argparse
import csv
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

# kernel-name fragment -> (stages whose FLOPs it computes, launches per forward, arithmetic)
KERNELS = [
    ("conv2d_split_kernel<4, 1, 1>", ("layer1",), 6, "f16x3"),
    ("conv2d_split_kernel<4, 2, 1>", ("layer2",), 9, "f16x3"),
    ("conv2d_split_kernel<4, 2, 2>", ("layer3", "layer4"), 20, "f16x3"),
    ("conv2d_f32_kernel<32>", ("layer1",), 6, "f32"),
    ("conv2d_f32_kernel<64>", ("layer2",), 9, "f32"),
    ("conv2d_f32_kernel<128>", ("layer3", "layer4"), 20, "f32"),
    ("wsp_conv1_kernel", ("conv1",), 1, "f32"),
]
PEAK = {"f16x3": 833.0, "f32": 157.0}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from wespeaker_bench import trunk_flops
    fl = trunk_flops(int(round(a.seconds * 16000)))
    rows = list(csv.DictReader(open(a.csv)))
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    lines = ["| kernel | calls | total ms | share | avg us | algorithmic TFLOP/s | of peak |", "|---|---|---|---|---|---|---|"]
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name, calls, ns = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        tf = frac = ""
        for frag, stages, per_fwd, arith in KERNELS:
            if frag in name:
                fwd = calls / per_fwd
                flop = fwd * a.chunks * sum(fl[s] for s in stages)
                t = flop / (ns * 1e-9) / 1e12
                tf, frac = f"{t:.1f}", f"{t / PEAK[arith]:.3f} ({arith})"
                break
        short = name if len(name) < 90 else name[:87] + "..."
        lines.append(f"| `{short}` | {calls} | {ns / 1e6:.2f} | {ns / total_ns:.1%} | {ns / calls / 1e3:.1f} | {tf} | {frac} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
