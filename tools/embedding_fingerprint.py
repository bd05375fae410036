"""SHA-256 fingerprints of the five speaker embeddings: the proof that a change to host code left every bit alone.

    python tools/embedding_fingerprint.py [--models ecapa,sbx,titanet,wespeaker,xvector] [--precisions f16x3,f32] [--out FILE]

For each of ``HipEcapaEmbedding``, ``HipSbXvectorEmbedding``, ``HipTitaNetEmbedding``, ``HipWeSpeakerEmbedding`` and
``HipEmbedding`` on ``diart_amd.synth``'s synthetic state, in both precisions, three calls on fixed inputs:

* ``rows_masked``: the rows forward with masks / weights, N = 5 rows of 16000 samples, Fw = 50.  Row 0 is all ones,
  row 1 keeps fewer samples than the model's minimum (one frame of 320 samples, or none where the minimum is lower;
  for the two models whose matrix is pooling weights it is simply one frame), row 2's waveform holds a NaN;
* ``rows_plain``: the same rows without masks;
* ``groups``: ``forward_groups`` with G = 2, K = 3, or ``forward_multi`` with B = 2, K = 3 for the two models that share
  a trunk.

After each call the digest of the output and of every ``peek`` buffer the model offers is recorded.  Run it at two
commits and compare the JSON: every digest must be equal (5 rows x 101 frames cross a 128-row tile boundary, and the
NaN-row and too-short paths both run).  One JSON line; ``--out`` also writes it to a file."""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N, S, FW, G, K = 5, 16000, 50, 2, 3
MAX_PEEK = 12


def models():
    from diart_amd import models as M, synth
    # name -> (class, synthetic state, samples the masks must keep (0: the matrix is pooling weights), forward_multi?)
    return {"ecapa": (M.HipEcapaEmbedding, synth.synth_ecapa_state, 640, False),
            "sbx": (M.HipSbXvectorEmbedding, synth.synth_sb_xvector_state, 480, False),
            "titanet": (M.HipTitaNetEmbedding, synth.synth_titanet_state, 257, False),
            "wespeaker": (M.HipWeSpeakerEmbedding, synth.synth_wespeaker_state, 0, True),
            "xvector": (M.HipEmbedding, synth.synth_embedding_state, 0, True)}


def digest(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def peeks(model) -> dict:
    from diart_amd._lib import DiartAmdError
    out = {}
    for which in range(MAX_PEEK):
        try:
            buf, frames = model.peek(S, which)
        except (DiartAmdError, NotImplementedError, AttributeError):
            continue
        out[str(which)] = {"sha256": digest(buf), "count": buf.numel(), "frames": frames}
    return out


def inputs(min_samples: int, dev):
    import torch
    g = torch.Generator().manual_seed(20260)
    wave = 0.1 * torch.randn(N, 1, S, generator=g)
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
    return wave.to(dev), m.to(dev), gm.to(dev)


def fingerprint(name: str, prec: str, dev) -> dict:
    import torch
    cls, state, min_samples, multi = models()[name]
    model = cls(state(), max_batch=8, precision=prec).to(dev)
    wave, m, gm = inputs(min_samples, dev)
    res = {}
    for call, run in (("rows_masked", lambda: model(wave, m)), ("rows_plain", lambda: model(wave)),
                      ("groups", lambda: (model.forward_multi if multi else model.forward_groups)(wave[:G], gm))):
        out = run()
        torch.cuda.synchronize(dev)
        res[call] = {"sha256": digest(out), "shape": list(out.shape),
                     "nan_rows": int(torch.isnan(out.reshape(-1, out.shape[-1])).any(dim=1).sum()), "peek": peeks(model)}
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ecapa,sbx,titanet,wespeaker,xvector")
    ap.add_argument("--precisions", default="f16x3,f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("embedding_fingerprint.py needs an MI355X GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", 0)
    res = {"tool": "embedding_fingerprint", "rows": N, "samples": S, "frames": FW, "groups": [G, K], "digests": {}}
    for name in a.models.split(","):
        res["digests"][name] = {prec: fingerprint(name, prec, dev) for prec in a.precisions.split(",")}
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
