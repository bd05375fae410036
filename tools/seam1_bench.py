"""Time the reference-shaped embedding call — every chunk ``num_speakers`` times, ``model((B*K,1,S), (B*K,F))``, what the
reference's ``SpeakerEmbedding`` hands a model — at 64 chunks x 3 speakers of 5 s for
``pyannote/embedding`` and WeSpeaker in both arithmetic modes, with ``repeated_rows="each"`` and ``"share"``; beside it
``forward_multi`` on the same windows and ``dz_rows_repeat`` alone.  Medians of repeated runs, one JSON file.

    python tools/seam1_bench.py [--chunks 64] [--speakers 3] [--steps 20] [--warmup 5] [--out profiles/r13a_seam1.json]
    python tools/seam1_bench.py --each-only --package-root OTHER_CHECKOUT --out each_parent.json
    python tools/seam1_bench.py --merge-each each_parent.json --parent-commit HASH   # "each_parent" beside this commit's "each"

Every figure is wall time of one call followed by a device synchronisation (``"share"`` waits for the device once
itself: a caller sees all of it), so the forms compare like for like.  ``--each-only`` uses nothing this commit added:
it runs against an older checkout (``--package-root``) to show that the default path did not move."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def timed(fn, dev, steps: int, warmup: int) -> dict:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"ms_median": statistics.median(ms), "ms_min": ms[0], "ms_max": ms[-1], "runs": steps}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="xvector,wespeaker")
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--each-only", action="store_true", help="time the default call only (works on older checkouts)")
    ap.add_argument("--package-root", default=str(ROOT), help="the checkout whose diart_amd package is timed")
    ap.add_argument("--merge-each", default=None, help="an --each-only result to record as each_parent")
    ap.add_argument("--parent-commit", default=None, help="the commit --merge-each was measured on (recorded)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13a_seam1.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.package_root).resolve()))

    import torch
    import diart_amd
    from diart_amd import _lib
    from diart_amd.models import HipEmbedding, HipWeSpeakerEmbedding
    from diart_amd.synth import synth_embedding_state, synth_streams, synth_wespeaker_state
    archs = {"xvector": (HipEmbedding, synth_embedding_state), "wespeaker": (HipWeSpeakerEmbedding, synth_wespeaker_state)}
    dev = torch.device("cuda", 0)
    B, K, S = a.chunks, a.speakers, int(round(a.seconds * 16000))
    x = torch.from_numpy(synth_streams(B, a.seconds + 0.01, seed0=1))[:, None, :S].contiguous().to(dev)
    w = (torch.rand(B, K, 293, generator=torch.Generator().manual_seed(0)) ** 2 + 1e-8).to(dev)       # speaker-major
    rows = x.repeat(1, K, 1).reshape(B * K, 1, S)                 # blocks/embedding.py:57 of the reference
    wrows = w.reshape(B * K, 293)
    res = {"workload": f"model(({B}*{K},1,{S}), ({B}*{K},293)): {B} chunks x {K} speakers, {a.seconds:g} s",
           "timing": "wall ms of one call + device synchronisation; median / min / max of `runs` calls after warm-up",
           "device": torch.cuda.get_device_name(0), "package": os.path.relpath(Path(diart_amd.__file__).resolve().parent, ROOT),
           "results": {}}
    for arch in a.models.split(","):
        cls, synth = archs[arch]
        for prec in a.precisions.split(","):
            out = res["results"].setdefault(arch, {}).setdefault(prec, {})
            each = cls(synth(), max_batch=B * K, precision=prec).to(dev)
            out["each"] = timed(lambda: each(rows, wrows), dev, a.steps, a.warmup)
            if not a.each_only:
                out["forward_multi"] = timed(lambda: each.forward_multi(x, w), dev, a.steps, a.warmup)
                out["each_again"] = timed(lambda: each(rows, wrows), dev, a.steps, a.warmup)     # the run-to-run spread
            del each
            if not a.each_only:
                share = cls(synth(), max_batch=B, precision=prec, repeated_rows="share").to(dev)
                out["share"] = timed(lambda: share(rows, wrows), dev, a.steps, a.warmup)
                assert share.last_shared == (B, K), share.last_shared
                del share
            print(arch, prec, json.dumps(out), flush=True)
    if not a.each_only:
        lib, ctx, r = _lib.load(), _lib.context(0), C.c_int()
        flat = rows[:, 0, :]
        st = torch.cuda.current_stream(dev).cuda_stream

        def detect():
            _lib.check(lib.dz_rows_repeat(ctx, flat.data_ptr(), flat.stride(0), B * K, S, st, C.byref(r)), "dz_rows_repeat")

        res["dz_rows_repeat"] = dict(timed(detect, dev, 5 * a.steps, a.warmup), rows=B * K, samples=S, answer=None,
                                     megabytes_read=B * K * S * 4 / 1e6)
        res["dz_rows_repeat"]["answer"] = r.value
        distinct = torch.from_numpy(synth_streams(8, a.seconds + 0.01, seed0=9))[:, :S].repeat(B * K // 8, 1).contiguous().to(dev)
        flat = distinct
        res["dz_rows_repeat_nothing_repeats"] = dict(timed(detect, dev, 5 * a.steps, a.warmup), answer=None)
        res["dz_rows_repeat_nothing_repeats"]["answer"] = r.value
        print("dz_rows_repeat", json.dumps(res["dz_rows_repeat"]), json.dumps(res["dz_rows_repeat_nothing_repeats"]))
    if a.merge_each:
        parent = json.loads(Path(a.merge_each).read_text())
        res["each_parent_commit"] = a.parent_commit
        for arch, precs in parent["results"].items():
            for prec, got in precs.items():
                res["results"].setdefault(arch, {}).setdefault(prec, {})["each_parent"] = got["each"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
