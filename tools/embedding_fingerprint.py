"""SHA-256 fingerprints of the seven speaker embeddings and the segmentation: the proof that a change to host code left
every bit alone.

    python tools/embedding_fingerprint.py [--models ecapa,ecapa-mel,sbx,sbr,titanet,wespeaker,xvector,segmentation] [--precisions f16x3,f32] [--out FILE]

For each of ``HipEcapaEmbedding``, ``HipEcapaMelEmbedding``, ``HipSbXvectorEmbedding``, ``HipSbResNetEmbedding``, ``HipTitaNetEmbedding``, ``HipWeSpeakerEmbedding`` and
``HipEmbedding`` on ``diart_amd.synth``'s synthetic state, in both precisions, three calls on fixed inputs:

* ``rows_masked``: the rows forward with masks / weights, N = 5 rows of 16000 samples, Fw = 50.  Row 0 is all ones,
  row 1 keeps fewer samples than the model's minimum (one frame of 320 samples, or none where the minimum is lower;
  for the two models whose matrix is pooling weights it is simply one frame), row 2's waveform holds a NaN;
* ``rows_plain``: the same rows without masks;
* ``groups``: ``forward_groups`` with G = 2, K = 3, or ``forward_multi`` with B = 2, K = 3 for the two models that share
  a trunk.

After each call the digest of the output and of every ``peek`` buffer the model offers is recorded.  Run it at two
commits and compare the JSON: every digest must be equal (5 rows x 101 frames cross a 128-row tile boundary, and the
NaN-row and too-short paths both run).  One JSON line; ``--out`` also writes it to a file.

16000 samples are 56 SincNet frames, below the 128-row chunk pitch from which ``HipEmbedding`` pools inside tdnn5's
epilogue, so ``xvector`` repeats its three calls at 40000 samples (145 frames, 131 behind tdnn5; keys ``<call>@40000``)
and adds ``multi5`` / ``multi5@40000``: ``forward_multi`` with K = 5 speakers, more than the fused pooling takes (plain
tdnn5 + stats_pool on pending frames).

``segmentation`` is ``HipSegmentation`` on ``synth_segmentation_state``, multilabel and powerset, B = 5 rows (row 2
holds a NaN) at both lengths (keys ``multilabel@16000`` ...): ``__call__``, ``forward_vad(return_scores=True)``, and
through the library itself ``dz_seg_forward_osp`` with normalize 0 and 1 (1: the unfused head) and ``dz_seg_front`` +
``dz_seg_back`` on caller-owned wave moments, whose digests must equal ``forward_osp``'s of the same run
(``front_back_equals_osp``)."""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N, S, FW, G, K = 5, 16000, 50, 2, 3
S_LONG, K_MANY = 40000, 5
MAX_PEEK = 12


def models():
    from diart_amd import models as M, synth
    # name -> (class, synthetic state, samples the masks must keep (0: the matrix is pooling weights), forward_multi?)
    return {"ecapa": (M.HipEcapaEmbedding, synth.synth_ecapa_state, 640, False),
            "ecapa-mel": (M.HipEcapaMelEmbedding, synth.synth_ecapa_state, 1024, False),
            "sbx": (M.HipSbXvectorEmbedding, synth.synth_sb_xvector_state, 480, False),
            "sbr": (M.HipSbResNetEmbedding, synth.synth_sb_resnet_state, 3, False),
            "titanet": (M.HipTitaNetEmbedding, synth.synth_titanet_state, 257, False),
            "wespeaker": (M.HipWeSpeakerEmbedding, synth.synth_wespeaker_state, 0, True),
            "xvector": (M.HipEmbedding, synth.synth_embedding_state, 0, True)}


def digest(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def peeks(model, samples: int = S) -> dict:
    from diart_amd._lib import DiartAmdError
    out = {}
    for which in range(MAX_PEEK):
        try:
            buf, frames = model.peek(samples, which)
        except (DiartAmdError, NotImplementedError, AttributeError):
            continue
        out[str(which)] = {"sha256": digest(buf), "count": buf.numel(), "frames": frames}
    return out


def inputs(min_samples: int, dev, samples: int = S):
    """(wave, rows weights, groups weights, K_MANY-speaker weights); the draws at S are the ones they always were"""
    import torch
    g = torch.Generator().manual_seed(20260 if samples == S else 20260 + samples)
    wave = 0.1 * torch.randn(N, 1, samples, generator=g)
    wave[2, 0, 4321] = float("nan")
    m = torch.rand(N, FW, generator=g)
    if min_samples:
        m = (m > 0.4).float()
    m[0] = 1.0
    m[1] = 0.0
    if min_samples == 0 or min_samples > S // FW:
        m[1, 7] = 1.0       # one frame: S / FW = 320 samples
    gm = torch.rand(G, K, FW, generator=g)
    if min_samples:
        gm = (gm > 0.4).float()
    gm[0, 0] = 1.0
    gm[1, 2] = m[1]
    many = torch.rand(G, K_MANY, FW, generator=g)
    return wave.to(dev), m.to(dev), gm.to(dev), many.to(dev)


def result(out, peek=None) -> dict:
    import torch
    res = {"sha256": digest(out), "shape": list(out.shape),
           "nan_rows": int(torch.isnan(out.reshape(-1, out.shape[-1])).any(dim=1).sum())}
    if peek is not None:
        res["peek"] = peek
    return res


def fingerprint(name: str, prec: str, dev) -> dict:
    import torch
    cls, state, min_samples, multi = models()[name]
    model = cls(state(), max_batch=8, precision=prec).to(dev)
    res = {}
    for samples in (S, S_LONG) if name == "xvector" else (S,):
        wave, m, gm, many = inputs(min_samples, dev, samples)
        calls = [("rows_masked", lambda: model(wave, m)), ("rows_plain", lambda: model(wave)),
                 ("groups", lambda: (model.forward_multi if multi else model.forward_groups)(wave[:G], gm))]
        if name == "xvector":
            calls.append(("multi5", lambda: model.forward_multi(wave[:G], many)))
        for call, run in calls:
            out = run()
            torch.cuda.synchronize(dev)
            res[call if samples == S else f"{call}@{samples}"] = result(out, peeks(model, samples))
    return res


def fingerprint_segmentation(prec: str, dev) -> dict:
    import ctypes as C
    import torch
    from diart_amd import _lib, synth
    from diart_amd.models import HipSegmentation, _stream_ptr
    lib = _lib.load()
    res = {}
    for powerset in (False, True):
        model = HipSegmentation(synth.synth_segmentation_state(powerset=powerset), max_batch=8, powerset=powerset,
                                precision=prec).to(dev)
        for samples in (S, S_LONG):
            wave = inputs(0, dev, samples)[0]
            rows = wave[:, 0, :]
            r = {"call": result(model(wave))}
            track, scores = model.forward_vad(wave, return_scores=True)
            r["vad_track"], r["vad_scores"] = result(track), result(scores)
            handle, st = model._need(samples, N), _stream_ptr(dev)
            F, spk = model.num_frames(samples), model.num_speakers

            def osp(normalize: int, halves: bool):
                seg = torch.empty((N, F, spk), dtype=torch.float32, device=dev)
                w = torch.empty((N, spk, F), dtype=torch.float32, device=dev)
                tail = (seg.data_ptr(), C.c_float(3.0), C.c_float(10.0), normalize, w.data_ptr(), st)
                if halves:
                    # caller-owned moments: a front half alone does not hand the handle's own to the back half
                    mom = torch.empty(N * lib.dz_wave_stats_floats(), dtype=torch.float32, device=dev)
                    _lib.check(lib.dz_wave_stats(_lib.context(dev.index), rows.data_ptr(), rows.stride(0), N, samples,
                                                 mom.data_ptr(), st), "dz_wave_stats")
                    _lib.check(lib.dz_seg_use_wave_stats(handle, mom.data_ptr()), "dz_seg_use_wave_stats")
                    _lib.check(lib.dz_seg_front(handle, rows.data_ptr(), rows.stride(0), N, st), "dz_seg_front")
                    _lib.check(lib.dz_seg_back(handle, N, *tail), "dz_seg_back")
                else:
                    _lib.check(lib.dz_seg_forward_osp(handle, rows.data_ptr(), rows.stride(0), N, *tail),
                               "dz_seg_forward_osp")
                torch.cuda.synchronize(dev)
                return {"seg": result(seg), "weights": result(w)}

            for normalize in (0, 1):
                r[f"forward_osp_n{normalize}"] = osp(normalize, False)
                r[f"front_back_n{normalize}"] = osp(normalize, True)
            r["front_back_equals_osp"] = all(r[f"front_back_n{n}"] == r[f"forward_osp_n{n}"] for n in (0, 1))
            res[f"{'powerset' if powerset else 'multilabel'}@{samples}"] = r
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ecapa,ecapa-mel,sbx,sbr,titanet,wespeaker,xvector,segmentation")
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("embedding_fingerprint.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", 0)
    res = {"tool": "embedding_fingerprint", "rows": N, "samples": S, "frames": FW, "groups": [G, K], "digests": {}}
    for name in a.models.split(","):
        res["digests"][name] = {prec: fingerprint_segmentation(prec, dev) if name == "segmentation" else
                                fingerprint(name, prec, dev) for prec in a.precisions.split(",")}
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
