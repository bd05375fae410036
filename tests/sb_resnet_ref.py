"""Float64 restatement of speechbrain's ResNet speaker embedding (speechbrain/spkrec-resnet-voxceleb) behind pyannote's
``PretrainedSpeakerEmbedding`` for the tests: the wrapper's mask -> kept samples -> relative lengths geometry,
speechbrain ``Fbank(n_mels=80)`` + ``InputNormalization("sentence", std_norm=False)`` (ECAPA's front end), the 2-D
ResNet of ``SEBasicBlock``s (``F.conv2d`` with zero padding 1, ``F.batch_norm`` NOT folded, squeeze-excitation over
every position of the padded batch), the attentive statistics pooling and ``norm_stats`` -> ``fc_embed`` ->
``norm_embed``.  The window, DFT, mel bank and network run in float64; the relative lengths, and the frame count they
select for the sentence mean, keep the reference's float32 arithmetic (``oracle.ecapa_ref.frame_counts``).  DESIGN.md
4.14 states the definition and marks with (R) where it rests on a reading of the published speechbrain / pyannote code."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.ecapa_ref import fbank, frame_counts, sentence_mean_norm

SAMPLE_RATE, HOP, N_MELS = 16000, 160, 80
STRIDES = (1, 2, 2, 2)
BN_EPS = 1e-5
VAR_CLAMP = 1e-5
_BN = ("running_mean", "running_var", "weight", "bias")


def frames(T: int, strides=STRIDES):
    """The time axis after the stem and each of the four layers: kernel 3, padding 1 -> (n - 1) // stride + 1."""
    out = [T]
    for s in strides:
        out.append((out[-1] - 1) // s + 1)
    return out


def min_num_samples(call) -> int:
    """(R) pyannote's ``PretrainedSpeakerEmbedding.min_num_samples``: the bisection over [2, sample_rate / 2] for the
    shortest input ``call(waveform (1, n))`` accepts (a RuntimeError means too short)."""
    lower, upper = 2, round(0.5 * SAMPLE_RATE)
    middle = (lower + upper) // 2
    while lower + 1 < upper:
        try:
            call(torch.randn(1, middle, dtype=torch.float64, generator=torch.Generator().manual_seed(middle)))
            upper = middle
        except RuntimeError:
            lower = middle
        middle = (lower + upper) // 2
    return upper


class SbResNetRef:
    dimension = 256

    def __init__(self, sd: Dict[str, torch.Tensor], strides=STRIDES, min_samples: int = 3):
        self.sd = {k: v.detach().double() for k, v in sd.items() if v.is_floating_point()}
        self.strides = tuple(strides)
        self.min_samples = int(min_samples)
        self.blocks = [sum(1 for i in range(64) if f"layer{L}.{i}.conv1.weight" in sd) for L in (1, 2, 3, 4)]

    def bn(self, x, prefix):
        s = self.sd
        return F.batch_norm(x, *(s[f"{prefix}.{n}"] for n in _BN), training=False, eps=BN_EPS)

    def block(self, x, p, stride):
        """SEBasicBlock: conv3x3(stride)-BN-ReLU-conv3x3-BN -> SE -> + shortcut -> ReLU, on (N, C, T, F)."""
        s = self.sd
        y = F.relu(self.bn(F.conv2d(x, s[p + ".conv1.weight"], None, stride, 1), p + ".bn1"))
        y = self.bn(F.conv2d(y, s[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
        z = y.mean(dim=(2, 3))                                             # AdaptiveAvgPool2d(1): every position
        z = F.relu(z @ s[p + ".se.fc.0.weight"].t() + s[p + ".se.fc.0.bias"])
        z = torch.sigmoid(z @ s[p + ".se.fc.2.weight"].t() + s[p + ".se.fc.2.bias"])
        y = y * z[:, :, None, None]
        r = x
        if p + ".downsample.0.weight" in s:
            r = self.bn(F.conv2d(x, s[p + ".downsample.0.weight"], None, stride, 0), p + ".downsample.1")
        return F.relu(y + r)

    def trunk(self, feats: torch.Tensor):
        """(N, T, 80) -> [stem, layer1 .. layer4], each channels-last (N, T_l, F_l, C_l).  ``lengths`` are not used
        (R): every frame of the padded batch takes part."""
        s = self.sd
        x = feats.unsqueeze(1)                                             # (N, 1, T, 80)
        x = F.relu(self.bn(F.conv2d(x, s["conv1.weight"], s["conv1.bias"], 1, 1), "bn1"))
        out = [x.permute(0, 2, 3, 1)]
        for L, (nb, stride) in enumerate(zip(self.blocks, self.strides), start=1):
            for i in range(nb):
                x = self.block(x, f"layer{L}.{i}", stride if i == 0 else 1)
            out.append(x.permute(0, 2, 3, 1))
        return out

    def head(self, x4: torch.Tensor):
        """Channels-last layer 4 (N, T4, F4, C4) -> (pooled (N, 2 C4 F4) in speechbrain's channel order c F4 + f, emb)."""
        s = self.sd
        x = x4.permute(0, 3, 2, 1).flatten(1, 2)                           # (N, C, F, T) -> (N, C F, T)
        a = F.relu(F.conv1d(x, s["attention.0.weight"].reshape(128, -1, 1), s["attention.0.bias"]))
        a = self.bn(a, "attention.2")
        w = torch.softmax(F.conv1d(a, s["attention.3.weight"].reshape(-1, 128, 1), s["attention.3.bias"]), dim=2)
        mu = (x * w).sum(dim=2)
        sg = torch.sqrt((((x ** 2) * w).sum(dim=2) - mu ** 2).clamp(min=VAR_CLAMP))
        pooled = torch.cat([mu, sg], dim=1)
        e = self.bn(pooled, "norm_stats")
        e = e @ s["fc_embed.weight"].t() + s["fc_embed.bias"]
        return pooled, self.bn(e, "norm_embed")

    @staticmethod
    def device_order(pooled: torch.Tensor, c4: int, f4: int) -> torch.Tensor:
        """pooled (N, 2 C4 F4) from speechbrain's channel order c F4 + f to the activations' f C4 + c (mu | sg)."""
        n = pooled.shape[0]
        return pooled.reshape(n, 2, c4, f4).transpose(2, 3).reshape(n, -1)

    @staticmethod
    def select(waveforms: torch.Tensor, masks: Optional[torch.Tensor]):
        """pyannote's mask -> (padded kept samples (N, Lmax), kept counts (N,))."""
        N, _, S = waveforms.shape
        wav = waveforms[:, 0, :]
        if masks is None:
            return wav, torch.full((N,), S, dtype=torch.long)
        imasks = F.interpolate(masks.unsqueeze(1).float(), size=S, mode="nearest").squeeze(1) > 0.5
        kept = [w[m] for w, m in zip(wav, imasks)]
        return torch.nn.utils.rnn.pad_sequence(kept, batch_first=True), imasks.sum(dim=1)

    def geometry(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> dict:
        signals, lens = self.select(waveforms, masks)
        too_short = lens < self.min_samples
        if signals.shape[1] < self.min_samples:
            return {"signals": None, "lens": lens, "too_short": too_short, "T": 0}
        rel = lens.float() / signals.shape[1]
        rel[too_short] = 1.0
        T = 1 + signals.shape[1] // HOP
        nvalid, _ = frame_counts(rel, T)
        return {"signals": signals, "lens": lens, "rel": rel, "too_short": too_short, "T": T, "nvalid": nvalid}

    def stages(self, geom: dict) -> dict:
        """Every stage of the batch ``geom`` describes, float64: feats (N,T,80), stem, layer1 .. layer4 (channels-last),
        pooled (speechbrain's order), emb (N,256; NaN for too-short rows)."""
        with torch.no_grad():
            feats = sentence_mean_norm(fbank(geom["signals"].double()), geom["rel"])
            xs = self.trunk(feats)
            pooled, emb = self.head(xs[4])
            emb[geom["too_short"]] = float("nan")
        out = {"feats": feats, "stem": xs[0], "pooled": pooled, "emb": emb}
        out.update({f"layer{i}": xs[i] for i in range(1, 5)})
        return out

    def __call__(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pyannote's ``PretrainedSpeakerEmbedding.__call__(waveforms (N,1,S), masks (N,F) | None)`` -> (N,256) float64
        with NaN rows (a NaN / Inf sample makes its row NaN through the arithmetic itself)."""
        geom = self.geometry(waveforms, masks)
        if geom["signals"] is None:
            return torch.full((waveforms.shape[0], self.dimension), float("nan"), dtype=torch.float64)
        return self.stages(geom)["emb"]
