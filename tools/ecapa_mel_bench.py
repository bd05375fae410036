"""Time the mel-spectrogram ECAPA-TDNN (speechbrain/spkrec-ecapa-voxceleb-mel-spec): ``HipEcapaMelEmbedding.forward_groups``
at 64 chunks x K = 3 speakers of 5 s in both arithmetic modes, the fbank ``HipEcapaEmbedding`` on the same inputs in the
same process as the comparison, and both on the N-stream engine (``StreamBatch`` with powerset segmentation, 64 streams,
output tail on).  One JSON line; ``--out`` also writes it to a file (profiles/<id>_ecapa_mel.json).

    python tools/ecapa_mel_bench.py [--models mel,fbank] [--chunks 64] [--steps 10] [--warmup 3] [--engine-steps 20] [--out FILE]

Algorithmic FLOPs (2 per multiply-add) are counted from the layer shapes at the handle's frames per row — 313 for the
mel front end (hop 256), 501 for the fbank (hop 160); every row is laid out and computed at that count whatever its own
valid frames.  ``front``: the STFT GEMM (1024 x 1026, or 400 x 402) and the mel GEMM.  ``front_share_of_kernel_time``:
the ``ecapa_fbank`` bracket (mask compaction, geometry, centre padding, STFT, magnitude, mel bank, log / mean) over the
sum of all brackets of a few extra forwards (``dz_prof_*``: the dispatches' own timestamps), beside the front end's
share of the multiply-adds.  TFLOP/s are against 833 (split products on the f16 pipe) and 157 (exact-f32 MFMA).
``--models fbank`` runs on a tree without the mel model (the parent commit's figures for the same visit)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK = {"f16x3": 833.0, "f32": 157.0}


def flops_per_row(model: str, num_samples: int) -> dict:
    T = 1 + num_samples // (256 if model == "mel" else 160)
    front = T * (1024 * 1026 + 513 * 80) if model == "mel" else T * (400 * 402 + 201 * 80)
    mac = {"front": front, "block0": T * 80 * 5 * 1024, "wide1x1": T * (6 * 1024 * 1024 + 3072 * 3072),
           "res2net": 3 * T * 7 * 128 * 128 * 3, "se": 3 * 2 * 1024 * 128,
           "asp": 6144 * 128 + T * (3072 * 128 + 128 * 3072), "fc": 6144 * 192}
    return {k: 2 * v for k, v in mac.items()}


def model_class(model: str):
    from diart_amd import models as M
    return M.HipEcapaMelEmbedding if model == "mel" else M.HipEcapaEmbedding


def brackets(lib, forwards: int) -> dict:
    name, ms, n, ch = C.c_char_p(), C.c_double(), C.c_longlong(), C.c_longlong()
    out = {}
    for tag in range(32):
        if lib.dz_prof_get(tag, C.byref(name), C.byref(ms), C.byref(n), C.byref(ch)) != 0 or n.value == 0:
            continue
        out[name.value.decode()] = round(ms.value / forwards, 4)
    return out


def groups_run(a, model, prec, dev, x, m, state):
    import torch
    from diart_amd import _lib
    net = model_class(model)(state, max_batch=a.chunks * a.speakers, precision=prec).to(dev)
    for _ in range(a.warmup):
        net.forward_groups(x, m, normalize=True)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    t0 = time.perf_counter()
    for s, e in ev:
        s.record()
        net.forward_groups(x, m, normalize=True)
        e.record()
    torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    lib = _lib.load()
    lib.dz_prof_enable(1)
    for _ in range(2):
        net.forward_groups(x, m, normalize=True)
    lib.dz_prof_collect()
    tab = brackets(lib, 2)
    lib.dz_prof_enable(0)
    return ms, wall, tab


def engine_run(a, model, prec, dev, audio, seg_state, emb_state):
    import torch
    from diart_amd.models import HipSegmentation
    from diart_amd.pipeline import StreamBatch
    n, hop, S = a.streams, 8000, 80000
    pipe = StreamBatch(HipSegmentation(seg_state, max_batch=n, powerset=True, precision=prec),
                       model_class(model)(emb_state, precision=prec), n, tau_active=0.5,
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
    ap.add_argument("--models", default="mel,fbank")
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--engine-steps", type=int, default=20, help="0: skip the engine lines")
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from diart_amd.hostinfo import limit_host_threads
    from diart_amd.synth import synth_ecapa_state, synth_segmentation_state, synth_streams
    if not torch.cuda.is_available():
        raise SystemExit("ecapa_mel_bench.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    limit_host_threads()
    dev = torch.device("cuda", 0)
    S = 80000
    x = torch.from_numpy(synth_streams(a.chunks, 5.01, seed0=1))[:, None, :S].contiguous().to(dev)
    # OSP-like masks: most frames kept, so each row's valid frames are close to the full count
    m = (torch.rand(a.chunks, a.speakers, 589, generator=torch.Generator().manual_seed(0)) > 0.3).float().to(dev)
    state = synth_ecapa_state()
    rows = a.chunks * a.speakers
    res = {"tool": "ecapa_mel_bench", "workload": f"forward_groups {a.chunks} chunks x K={a.speakers}, 5 s",
           "device": torch.cuda.get_device_name(0), "models": {}}
    precs, names = a.precisions.split(","), a.models.split(",")
    for model in names:
        fl = flops_per_row(model, S)
        per_step = rows * sum(fl.values())
        r = {"frames_per_row": 1 + S // (256 if model == "mel" else 160),
             "gflop_per_row": {k: round(v / 1e9, 4) for k, v in fl.items()}, "tflop_per_step": round(per_step / 1e12, 4),
             "front_share_of_flops": round(fl["front"] / sum(fl.values()), 4), "groups": {}, "engine": {}}
        for prec in precs:
            ms, wall, tab = groups_run(a, model, prec, dev, x, m, state)
            med = ms[len(ms) // 2]
            tf = per_step / (med * 1e-3) / 1e12
            total = sum(tab.values()) or 1.0
            r["groups"][prec] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(ms[0], 4),
                                 "ms_per_step_max": round(ms[-1], 4), "ms_per_step_wall": round(wall, 4),
                                 "tflops": round(tf, 2), "fraction_of_peak": round(tf / PEAK[prec], 4),
                                 "peak_tflops": PEAK[prec], "kernel_ms_by_bracket": tab,
                                 "front_share_of_kernel_time": round(tab.get("ecapa_fbank", 0.0) / total, 4)}
        res["models"][model] = r
    if a.engine_steps > 0:
        seconds = (S + 8000 * (a.warmup + a.engine_steps + 2)) / 16000.0
        audio = torch.from_numpy(synth_streams(a.streams, seconds, seed0=4242)).to(dev)
        seg_state = synth_segmentation_state(seed=77, powerset=True)
        for model in names:
            for prec in precs:
                res["models"][model]["engine"][prec] = engine_run(a, model, prec, dev, audio, seg_state, state)
    if "mel" in names and "fbank" in names:
        res["mel_over_fbank"] = {prec: round(res["models"]["mel"]["groups"][prec]["ms_per_step_median"] /
                                             res["models"]["fbank"]["groups"][prec]["ms_per_step_median"], 4)
                                 for prec in precs}
        res["frames_ratio"] = round(313 / 501, 4)
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
