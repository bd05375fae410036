"""Time the speechbrain ResNet (speechbrain/spkrec-resnet-voxceleb): ``HipSbResNetEmbedding.forward_groups`` at 64
chunks x K = 3 speakers of 5 s in both arithmetic modes, and the same model on the N-stream engine (``StreamBatch``
with powerset segmentation, 64 streams, output tail on).  One JSON line; ``--out`` also writes it to a file.

    python tools/sb_resnet_bench.py [--chunks 64] [--steps 10] [--warmup 3] [--engine-steps 20] [--out FILE]

Algorithmic FLOPs are counted from the layer shapes at the handle's 501 frames per row (2 per multiply-add): the DFT
and mel GEMMs, the stem, the 3x3 / 1x1 convolutions of the four layers, the two attention convolutions and the final
Linear.  The masked convolutions skip the tiles that lie wholly behind a group's own T_g, so the kernels do somewhat
less than this where the masks drop samples.  TFLOP/s are against 833 (split products on the f16 pipe) and 157
(exact-f32 MFMA)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK = {"f16x3": 833.0, "f32": 157.0}


def flops_per_row(num_samples: int, shape: dict) -> dict:
    """``shape``: ``weights.sb_resnet_shape`` of the state."""
    T, F, cin = 1 + num_samples // 160, 80, shape["stem"]
    out = {"fbank": 2 * T * (400 * 402 + 201 * 80), "stem": 2 * T * F * 9 * cin}
    for l, (c, nb, s) in enumerate(zip(shape["channels"], shape["block_sizes"], shape["strides"]), start=1):
        macs = 0
        for i in range(nb):
            stride = s if i == 0 else 1
            To, Fo = (T - 1) // stride + 1, (F - 1) // stride + 1
            macs += To * Fo * c * (9 * cin + 9 * c + (cin if (stride != 1 or cin != c) else 0))
            T, F, cin = To, Fo, c
        out[f"layer{l}"] = 2 * macs
    cf = F * cin
    out["attention"] = 2 * T * 2 * 128 * cf
    out["linear"] = 2 * 2 * cf * 256
    return out


def groups_run(a, prec, dev, x, m, state):
    import torch
    from diart_amd.models import HipSbResNetEmbedding
    model = HipSbResNetEmbedding(state, max_batch=a.chunks * a.speakers, precision=prec).to(dev)
    for _ in range(a.warmup):
        model.forward_groups(x, m, normalize=True)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    t0 = time.perf_counter()
    for s, e in ev:
        s.record()
        model.forward_groups(x, m, normalize=True)
        e.record()
    torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return ms, wall


def engine_run(a, prec, dev, audio, seg_state, emb_state):
    import torch
    from diart_amd.models import HipSbResNetEmbedding, HipSegmentation
    from diart_amd.pipeline import StreamBatch
    n, hop, S = a.streams, 8000, 80000
    pipe = StreamBatch(HipSegmentation(seg_state, max_batch=n, powerset=True, precision=prec),
                       HipSbResNetEmbedding(emb_state, precision=prec), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=dev, tail=True)

    def run(t0, count):
        inflight = []
        for t in range(t0, t0 + count):
            inflight.append(pipe.launch(audio[:, t * hop:t * hop + S]))
            if len(inflight) >= pipe.max_inflight:
                pipe.finish(inflight.pop(0), want_scores=False)
        while inflight:
            pipe.finish(inflight.pop(0), want_scores=False)

    run(0, a.warmup)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run(a.warmup, a.engine_steps)
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    return {"xrt": round(n * a.engine_steps / el / 2, 2), "ms_per_step": round(1e3 * el / a.engine_steps, 3),
            "lanes": pipe.depth, "inflight": pipe.max_inflight, "streams": n, "steps": a.engine_steps}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--engine-steps", type=int, default=20, help="0: skip the engine line")
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from diart_amd.hostinfo import limit_host_threads
    from diart_amd.synth import synth_sb_resnet_state, synth_segmentation_state, synth_streams
    if not torch.cuda.is_available():
        raise SystemExit("sb_resnet_bench.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    limit_host_threads()
    dev = torch.device("cuda", 0)
    S = 80000
    x = torch.from_numpy(synth_streams(a.chunks, 5.01, seed0=1))[:, None, :S].contiguous().to(dev)
    # OSP-like masks: most frames kept, so each group's T_g is close to the full 501 frames
    m = (torch.rand(a.chunks, a.speakers, 589, generator=torch.Generator().manual_seed(0)) > 0.3).float().to(dev)
    from diart_amd.weights import sb_resnet_shape
    state = synth_sb_resnet_state()
    fl = flops_per_row(S, sb_resnet_shape(state))
    rows = a.chunks * a.speakers
    per_step = rows * sum(fl.values())
    res = {"tool": "sb_resnet_bench", "workload": f"forward_groups {a.chunks} chunks x K={a.speakers}, 5 s",
           "device": torch.cuda.get_device_name(0), "gflop_per_row": {k: round(v / 1e9, 4) for k, v in fl.items()},
           "tflop_per_step": round(per_step / 1e12, 4), "groups": {}, "engine": {}}
    precs = a.precisions.split(",")
    for prec in precs:
        ms, wall = groups_run(a, prec, dev, x, m, state)
        med = ms[len(ms) // 2]
        tf = per_step / (med * 1e-3) / 1e12
        res["groups"][prec] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(ms[0], 4),
                               "ms_per_step_wall": round(wall, 4), "tflops": round(tf, 2),
                               "fraction_of_peak": round(tf / PEAK[prec], 4), "peak_tflops": PEAK[prec]}
    if a.engine_steps > 0:
        seconds = (S + 8000 * (a.warmup + a.engine_steps + 2)) / 16000.0
        audio = torch.from_numpy(synth_streams(a.streams, seconds, seed0=4242)).to(dev)
        seg_state = synth_segmentation_state(seed=77, powerset=True)
        for prec in precs:
            res["engine"][prec] = engine_run(a, prec, dev, audio, seg_state, state)
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
