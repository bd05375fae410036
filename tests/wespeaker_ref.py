"""Float64 restatement of pyannote.audio 3.1's ``WeSpeakerResNet34`` (pyannote/wespeaker-voxceleb-resnet34-LM) for the
tests: the kaldi fbank (torchaudio.compliance.kaldi.fbank) restated with ``torch.fft.rfft``, the ResNet34 trunk with
``F.conv2d`` / ``F.batch_norm`` (BatchNorm NOT folded), TSTP pooling with pyannote.audio 3.1's ``StatsPool`` and
``seg_1``.  Independent of the product code (it builds its own mel bank); DESIGN.md "WeSpeaker ResNet34" states the
definition and marks where it rests on a reading of the published code."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

BLOCKS = (3, 4, 6, 3)
EPS_F32 = torch.finfo(torch.float32).eps


def mel_banks(num_bins: int = 80, n_fft: int = 512, sr: int = 16000, low: float = 20.0) -> torch.Tensor:
    """kaldi get_mel_banks (high_freq = Nyquist, no VTLN) padded with a zero Nyquist column: (80, 257) float64."""
    def mel(f):
        return 1127.0 * torch.log(1.0 + torch.as_tensor(f, dtype=torch.float64) / 700.0)
    lo, hi = mel(low), mel(sr / 2)
    d = (hi - lo) / (num_bins + 1)
    out = torch.zeros(num_bins, n_fft // 2 + 1, dtype=torch.float64)
    m = mel(sr / n_fft * torch.arange(n_fft // 2, dtype=torch.float64))
    for b in range(num_bins):
        l, c, r = lo + b * d, lo + (b + 1) * d, lo + (b + 2) * d
        out[b, : n_fft // 2] = torch.clamp(torch.minimum((m - l) / (c - l), (r - m) / (r - c)), min=0.0)
    return out


def fbank_raw(wave: torch.Tensor, window_div: int = 399):
    """(N, S) waveform in [-1, 1] -> (log-mel (N, T, 80) before the mean subtraction, power scale (N, T)): x 2^15,
    kaldi fbank (snip_edges, DC removal, pre-emphasis 0.97 with the first sample replicated, symmetric Hamming,
    512-point power spectrum, log floor at float32 eps).  The power scale is the frame's spectral energy (all 257
    bins) after the DC removal, or, when larger, the energy of a DC residue of one float32 ulp of the frame's mean
    level (what an f32 mean leaves behind).  ``window_div`` 400 makes the window periodic (a mutation the tests'
    gates must see)."""
    x = wave.double() * (1 << 15)
    N, S = x.shape
    T = 1 + (S - 400) // 160
    idx = torch.arange(T)[:, None] * 160 + torch.arange(400)[None, :]
    fr = x[:, idx]                                                     # (N, T, 400)
    level = fr.abs().amax(dim=-1)
    fr = fr - fr.mean(dim=-1, keepdim=True)
    n = torch.arange(400, dtype=torch.float64)
    win = 0.54 - 0.46 * torch.cos(2 * math.pi * n / window_div)

    def spectrum(f):
        prev = torch.cat([f[..., :1], f[..., :-1]], dim=-1)
        spec = torch.fft.rfft(F.pad((f - 0.97 * prev) * win, (0, 112)), dim=-1)      # (N, T, 257)
        return spec.real ** 2 + spec.imag ** 2
    pw = spectrum(fr)
    ulp = torch.where(level > 0, torch.exp2(torch.floor(torch.log2(level.clamp_min(1e-300))) - 23), torch.zeros_like(level))
    e_dc = spectrum(ulp[..., None].expand(-1, -1, 400)).sum(-1)
    e = pw @ mel_banks().t()
    return torch.log(torch.clamp(e, min=EPS_F32)), torch.maximum(pw.sum(-1), e_dc)


def fbank(wave: torch.Tensor, window_div: int = 399) -> torch.Tensor:
    """(N, S) waveform in [-1, 1] -> (N, T, 80) features: ``fbank_raw`` with the mean over frames subtracted per
    row."""
    feats = fbank_raw(wave, window_div)[0]
    return feats - feats.mean(dim=1, keepdim=True)


def frames(num_samples: int):
    """(fbank T, T after layers 1 .. 4): the conv arithmetic (kernel 3 / pad 1 or kernel 1, strides 1, 2, 2, 2)."""
    T = 1 + (num_samples - 400) // 160
    out = [T, T]
    for _ in range(3):
        T = (T + 2 * 1 - 3) // 2 + 1
        out.append(T)
    return out


class WeSpeakerRef:
    def __init__(self, sd: Dict[str, torch.Tensor]):
        self.sd = {k: v.detach().double() for k, v in sd.items()}

    def _bn(self, x, p):
        s = self.sd
        return F.batch_norm(x, s[p + ".running_mean"], s[p + ".running_var"], s[p + ".weight"], s[p + ".bias"],
                            training=False, eps=1e-5)

    def trunk(self, feats: torch.Tensor):
        """(N, T, 80) -> dict of stage outputs in channels-last (N, F, T, C): conv1, layer1 .. layer4."""
        s = self.sd
        x = feats.permute(0, 2, 1).unsqueeze(1)                        # (N, 1, 80, T)
        x = F.relu(self._bn(F.conv2d(x, s["resnet.conv1.weight"], padding=1), "resnet.bn1"))
        out = {"conv1": x}
        for li, nb in enumerate(BLOCKS):
            for j in range(nb):
                p = f"resnet.layer{li + 1}.{j}"
                stride = 2 if (li > 0 and j == 0) else 1
                h = F.relu(self._bn(F.conv2d(x, s[p + ".conv1.weight"], stride=stride, padding=1), p + ".bn1"))
                h = self._bn(F.conv2d(h, s[p + ".conv2.weight"], padding=1), p + ".bn2")
                sc = x
                if p + ".shortcut.0.weight" in s:
                    sc = self._bn(F.conv2d(x, s[p + ".shortcut.0.weight"], stride=stride), p + ".shortcut.1")
                x = F.relu(h + sc)
            out[f"layer{li + 1}"] = x
        return {k: v.permute(0, 2, 3, 1).contiguous() for k, v in out.items()}, x

    @staticmethod
    def pool(x: torch.Tensor, weights: Optional[torch.Tensor]) -> torch.Tensor:
        """TSTP / pyannote.audio 3.1 StatsPool on (N, C, F, T) features: rearranged to (N, C F, T); weights (N, Fw)
        resampled to T with F.interpolate(mode="nearest")."""
        N, C, Fq, T = x.shape
        seq = x.reshape(N, C * Fq, T)
        if weights is None:
            return torch.cat([seq.mean(dim=-1), seq.std(dim=-1, correction=1)], dim=-1)
        w = weights.double().unsqueeze(1)
        if w.shape[-1] != T:
            w = F.interpolate(w, size=T, mode="nearest")
        v1 = w.sum(dim=2) + 1e-8
        mean = (seq * w).sum(dim=2) / v1
        dx2 = (seq - mean.unsqueeze(2)) ** 2
        v2 = (w ** 2).sum(dim=2)
        var = (dx2 * w).sum(dim=2) / (v1 - v2 / v1 + 1e-8)
        return torch.cat([mean, torch.sqrt(var)], dim=1)

    def stages(self, wave: torch.Tensor, weights: Optional[torch.Tensor] = None):
        """(N, S) -> dict: fbank (N, 80, T), conv1, layer1 .. 4 (N, F, T, C), pooled (N, 5120), emb (N, 256)."""
        with torch.no_grad():
            feats = fbank(wave)
            st, x = self.trunk(feats)
            pooled = self.pool(x, weights)
            emb = pooled @ self.sd["resnet.seg_1.weight"].t() + self.sd["resnet.seg_1.bias"]
        st.update(fbank=feats.permute(0, 2, 1).contiguous(), pooled=pooled, emb=emb)
        return st

    def multi(self, wave: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N, S) and weights (N, K, Fw) -> (N, K, 256), the trunk once per row; weights None -> (N, 256)."""
        with torch.no_grad():
            _, x = self.trunk(fbank(wave))
            if weights is not None:
                N, K = weights.shape[:2]
                x, weights = x.repeat_interleave(K, dim=0), weights.reshape(N * K, -1)
            emb = self.pool(x, weights) @ self.sd["resnet.seg_1.weight"].t() + self.sd["resnet.seg_1.bias"]
        return emb if weights is None else emb.view(N, K, -1)

    def __call__(self, wave: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pyannote's ``model(waveforms (N, 1, S), weights (N, Fw))`` -> (N, 256)."""
        if wave.ndim == 3:
            wave = wave[:, 0]
        return self.stages(wave, weights)["emb"]


# --------------------------------------------------------------------------- #
# one convolution of the trunk as the kernels compute it (k_conv2d.hip): channels-last activations, an implicit GEMM
# with k = (kh 3 + kw) Cin + c, epilogue + bias, + residual, ReLU
# --------------------------------------------------------------------------- #
def conv_matrix(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight (Cout, Cin, kh, kw) -> [Cout][(kh 3 + kw) Cin + c], element by element from the index formula."""
    cout, cin, kh = w.shape[0], w.shape[1], w.shape[2]
    k = torch.arange(kh * kh * cin)
    tap, c = k // cin, k % cin
    return w[:, c, tap // kh, tap % kh].contiguous()


def split_planes(m: torch.Tensor) -> torch.Tensor:
    """f32 matrix -> int16 [2][R][K] of f16 bits: hi = f16(m), lo = f16((m - hi) 2^11)."""
    m = m.float()
    hi = m.half()
    lo = ((m - hi.float()) * 2048.0).half()
    return torch.stack([hi, lo]).view(torch.int16)


def im2col(x: torch.Tensor, taps: int, stride: int, tpad=(1, 1)) -> torch.Tensor:
    """Channels-last (B, Fi, Ti, Cin) -> (B, Fo, To, taps Cin): row (b, fo, to) of the implicit GEMM in the kernels' k
    order, zeros where a tap falls into the padding.  ``tpad`` = (left, right) zero columns of the time axis (3x3
    only; (0, 2) is the one-column shift the tests' gates must see)."""
    B, Fi, Ti, Cin = x.shape
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    if taps == 1:
        return x[:, ::stride, ::stride, :][:, :Fo, :To]
    xp = F.pad(x, (0, 0, tpad[0], tpad[1], 1, 1))
    cols = [xp[:, kh: kh + stride * (Fo - 1) + 1: stride, kw: kw + stride * (To - 1) + 1: stride, :]
            for kh in range(3) for kw in range(3)]
    return torch.cat(cols, dim=-1)


def conv_ref(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, r: Optional[torch.Tensor], relu: bool, stride: int):
    """float64 F.conv2d of channels-last x (B, Fi, Ti, Cin) with w (Cout, Cin, k, k) (k 3: padding 1, k 1: none),
    + b, + r (B, Fo, To, Cout), ReLU -> (y (B, Fo, To, Cout), scale): scale = sum |x w| + |b| + |r| per element,
    the denominator of the tests' per-element gate."""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    pad = 1 if w.shape[-1] == 3 else 0
    y = F.conv2d(xd, wd, b.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    scale = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if r is not None:
        y = y + r.double()
        scale = scale + r.double().abs()
    return (F.relu(y) if relu else y), scale
