"""Write ``tests/golden/adjust_volume.npz``: inputs, targets and what the REFERENCE's own ``AdjustVolume`` block
(``blocks/utils.py:92-137``, loaded unmodified through ``oracle.pyannote_stub.load_reference``) makes of them, with the
volumes its ``get_volumes`` reports.  Data only.  Runs on the CPU; needs the reference checkout.

    python tools/make_volume_golden.py [--reference /root/reference/src/diart] [--out tests/golden/adjust_volume.npz]

Cases (``CASES``): ``(samples, channels, target dB)``, three chunks each with amplitudes 0.01, 0.3 and 2.0 (seeded
Gaussian noise, so both the saturating and the plain branch occur), at the sample counts around the kernel's quad
and its tail; every target meets every amplitude.  One more case holds the special chunks: all zeros, a NaN at the
first, a middle and the last sample, a +Inf, between two ordinary chunks.  Arrays of case ``i``: ``x{i}``
(batch, samples, channels) float32, ``db{i}``, ``y{i}`` (the block's output) and ``v{i}`` (batch, 1, channels).
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

AMPLITUDES = (0.01, 0.3, 2.0)
TARGETS = (-20.0, 0.0, 6.0)
CASES = [(1, 1, -20.0), (3, 1, 0.0), (255, 1, 6.0), (256, 1, -20.0), (257, 1, 0.0), (1031, 1, 6.0),
         (3, 2, 6.0), (257, 2, -20.0), (1, 3, 0.0), (256, 3, 6.0)]
SPECIAL_SAMPLES = 65


def inputs():
    """[(x (batch, samples, channels) float32, target dB)], the special case last."""
    out = []
    for i, (samples, channels, db) in enumerate(CASES):
        rng = np.random.default_rng(7000 + i)
        x = np.stack([rng.standard_normal((samples, channels)) * a for a in AMPLITUDES]).astype(np.float32)
        out.append((x, db))
    rng = np.random.default_rng(7999)
    x = (rng.standard_normal((7, SPECIAL_SAMPLES, 1)) * 0.3).astype(np.float32)
    x[1] = 0.0
    x[2, 0] = np.nan
    x[3, SPECIAL_SAMPLES // 2] = np.nan
    x[4, -1] = np.nan
    x[5, 17] = np.inf
    out.append((x, -20.0))
    return out


def make(reference: str = "/root/reference/src/diart") -> dict:
    from oracle.pyannote_stub import load_reference
    block_cls = load_reference(reference).blocks_utils.AdjustVolume
    arrays = {}
    for i, (x, db) in enumerate(inputs()):
        t = torch.from_numpy(x.copy())
        arrays[f"x{i}"] = x
        arrays[f"db{i}"] = np.float64(db)
        arrays[f"y{i}"] = block_cls(db)(t).numpy().astype(np.float32)
        arrays[f"v{i}"] = block_cls.get_volumes(t).numpy().astype(np.float32)
    return arrays


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", default="/root/reference/src/diart")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "adjust_volume.npz"))
    args = ap.parse_args()
    arrays = make(args.reference)
    np.savez(args.out, **arrays)
    print(f"{args.out}: {len(arrays) // 4} cases, {Path(args.out).stat().st_size} bytes")


if __name__ == "__main__":
    main()
