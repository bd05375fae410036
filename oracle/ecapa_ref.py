"""PyTorch-CPU fp32 restatement of the config-3 embedding path (TEST INFRASTRUCTURE).

``pyannote.audio.pipelines.speaker_verification.PretrainedSpeakerEmbedding`` wrapping
``speechbrain/spkrec-ecapa-voxceleb`` — reached from the reference by the fallback at
``/root/reference/src/diart/models.py:59`` and called at ``models.py:262``; SURVEY.md Appendix
A.3.  Neither pyannote.audio nor speechbrain is in ``/root/reference`` or installable here, so
this is written from the published architecture (ECAPA-TDNN, C=1024, 192-d; Fbank(80), sentence
mean normalisation) — **parity unpinned**; module names are chosen so ``state_dict()`` keys equal
the speechbrain checkpoint's (``blocks.1.res2net_block.blocks.0.conv.conv.weight`` ...), which is
also the key set ``diart_amd.synth.synth_ecapa_state`` produces and ``diart_amd.weights`` consumes.

Quirks restated on purpose (they change the numbers): reflect "same" padding at the edge of the
PADDED batch tensor (so a row's embedding depends on the longest row of its batch), ``top_db``
clipping against the per-row maximum over valid AND padded frames, sentence mean over
``round(len * T)`` frames, masked SE mean / attentive statistics, rows with fewer than
``MIN_NUM_SAMPLES`` kept samples -> NaN, numpy output.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SAMPLE_RATE, N_FFT, HOP, N_MELS = 16000, 400, 160, 80
# PretrainedSpeakerEmbedding.min_num_samples bisects for the shortest input the network accepts:
# reflect padding of 4 frames (k=3, dilation 4) needs T = 1 + n // 160 >= 5 frames
MIN_NUM_SAMPLES = 640


# --------------------------------------------------------------------------- #
# features: speechbrain Fbank(n_mels=80) + InputNormalization("sentence", std_norm=False)
# --------------------------------------------------------------------------- #
def mel_filterbank(n_mels: int = N_MELS, n_fft: int = N_FFT, sample_rate: int = SAMPLE_RATE,
                   dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """speechbrain Filterbank (triangular, f_min=0, f_max=sr/2): (n_fft//2+1, n_mels)."""
    to_mel = lambda hz: 2595.0 * math.log10(1.0 + hz / 700.0)
    mel = torch.linspace(to_mel(0.0), to_mel(sample_rate / 2), n_mels + 2, dtype=dtype)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    band = (hz[1:] - hz[:-1])[:-1]
    f_central = hz[1:-1]
    n_stft = n_fft // 2 + 1
    all_freqs = torch.linspace(0, sample_rate // 2, n_stft, dtype=dtype)
    slope = (all_freqs.repeat(n_mels, 1) - f_central[:, None]) / band[:, None]
    fb = torch.max(torch.zeros(1, dtype=dtype), torch.min(slope + 1.0, -slope + 1.0))
    return fb.t().contiguous()          # (201, 80)


def fbank(wavs: torch.Tensor) -> torch.Tensor:
    """(N, L) -> (N, 1 + L // 160, 80) log-mel in dB with top_db = 80, in the dtype of ``wavs`` (window, DFT and mel
    bank included)."""
    window = torch.hamming_window(N_FFT, dtype=wavs.dtype)
    spec = torch.stft(wavs, N_FFT, HOP, N_FFT, window, center=True, pad_mode="constant",
                      normalized=False, onesided=True, return_complex=True)
    power = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)            # (N, T, 201)
    mel = power @ mel_filterbank(dtype=wavs.dtype)
    x_db = 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
    floor = x_db.amax(dim=(-2, -1)) - 80.0
    return torch.max(x_db, floor.view(-1, 1, 1))


def frame_counts(lens: torch.Tensor, T: int):
    """Per-row frame counts the relative lengths select, in the arithmetic of the reference, which keeps ``lens``
    float32 whatever the network's dtype: ``nvalid = round(lens * T)`` (half to even: the sentence mean) and
    ``nmask = #{t : t < lens * T}`` (the squeeze-excitation mean and the attentive pooling)."""
    assert lens.dtype == torch.float32
    v = lens * T
    nvalid = torch.round(v).long()
    nmask = (torch.arange(T)[None, :] < v[:, None]).sum(dim=1)
    return nvalid, nmask


def rounding_edges(lmax: int, lo: int = MIN_NUM_SAMPLES) -> dict:
    """Kept lengths in ``[lo, lmax]`` at the edges of ``frame_counts`` for a batch whose longest row is ``lmax``:
    "int" (``float32(len / lmax) * T`` is an integer: nmask stops there, round is exact), "half" (on k + 0.5: round
    goes to even), "near" (within one float32 ulp of either, not on it) and "differs" (the float32 value rounds or
    ceils differently from the exact rational ``len T / lmax``: the cases a restatement in float64 gets wrong)."""
    from fractions import Fraction
    T = 1 + lmax // HOP
    lens = np.arange(lo, lmax + 1)
    v = (lens.astype(np.float32) / np.float32(lmax)) * np.float32(T)
    frac2 = v * np.float32(2)
    on_grid = frac2 == np.round(frac2)                         # integer or half-integer (exact in float32)
    is_int = v == np.round(v)
    ulp = np.spacing(v)
    near = ~on_grid & (np.abs(frac2 - np.round(frac2)) <= np.float32(2) * ulp)
    differs = []
    for i in np.flatnonzero(on_grid | near):    # (off the grid by more than an ulp, both round alike: the test scans all)
        x = Fraction(int(lens[i]) * T, lmax)
        fl = x.numerator // x.denominator
        r = x - fl
        exact_round = fl + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2) else 0)
        exact_ceil = fl + (1 if r else 0)
        if int(np.rint(v[i])) != exact_round or int(np.ceil(v[i])) != exact_ceil:
            differs.append(int(lens[i]))
    return {"T": T, "int": lens[is_int].tolist(), "half": lens[on_grid & ~is_int].tolist(),
            "near": lens[near].tolist(), "differs": differs}


def sentence_mean_norm(feats: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    out = feats.clone()
    for i in range(feats.shape[0]):
        n = int(torch.round(lens[i] * feats.shape[1]).int())
        out[i] = feats[i] - feats[i, :n].mean(dim=0)
    return out


# --------------------------------------------------------------------------- #
# ECAPA-TDNN (speechbrain.lobes.models.ECAPA_TDNN)
# --------------------------------------------------------------------------- #
class _Conv(nn.Module):
    """speechbrain Conv1d(padding="same", padding_mode="reflect") on (N, C, T)."""

    def __init__(self, cin, cout, k, dilation=1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k, dilation=dilation)
        self.pad = dilation * (k - 1) // 2

    def forward(self, x):
        if self.pad:
            x = F.pad(x, (self.pad, self.pad), mode="reflect")
        return self.conv(x)


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.norm = nn.BatchNorm1d(c)

    def forward(self, x):
        return self.norm(x)


class TDNNBlock(nn.Module):
    def __init__(self, cin, cout, k, dilation=1):
        super().__init__()
        self.conv, self.norm = _Conv(cin, cout, k, dilation), _BN(cout)

    def forward(self, x):
        return self.norm(F.relu(self.conv(x)))


class Res2NetBlock(nn.Module):
    def __init__(self, c, scale=8, k=3, dilation=1):
        super().__init__()
        self.scale = scale
        self.blocks = nn.ModuleList([TDNNBlock(c // scale, c // scale, k, dilation) for _ in range(scale - 1)])

    def forward(self, x):
        y, prev = [], None
        for i, xi in enumerate(torch.chunk(x, self.scale, dim=1)):
            if i == 0:
                yi = xi
            elif i == 1:
                yi = self.blocks[i - 1](xi)
            else:
                yi = self.blocks[i - 1](xi + prev)
            y.append(yi)
            prev = yi
        return torch.cat(y, dim=1)


def length_to_mask(length: torch.Tensor, max_len: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``length`` stays float32 (the comparison is the reference's); the 0 / 1 mask takes the network's dtype."""
    return (torch.arange(max_len)[None, :] < length[:, None]).to(dtype)


class SEBlock(nn.Module):
    def __init__(self, c, se):
        super().__init__()
        self.conv1, self.conv2 = _Conv(c, se, 1), _Conv(se, c, 1)

    def forward(self, x, lengths):
        L = x.shape[-1]
        mask = length_to_mask(lengths * L, L, x.dtype).unsqueeze(1)
        s = (x * mask).sum(dim=2, keepdim=True) / mask.sum(dim=2, keepdim=True)
        s = torch.sigmoid(self.conv2(F.relu(self.conv1(s))))
        return s * x


class SERes2NetBlock(nn.Module):
    def __init__(self, c, dilation, scale=8, se=128):
        super().__init__()
        self.tdnn1 = TDNNBlock(c, c, 1)
        self.res2net_block = Res2NetBlock(c, scale, 3, dilation)
        self.tdnn2 = TDNNBlock(c, c, 1)
        self.se_block = SEBlock(c, se)

    def forward(self, x, lengths):
        r = x
        x = self.tdnn2(self.res2net_block(self.tdnn1(x)))
        return self.se_block(x, lengths) + r


class AttentiveStatisticsPooling(nn.Module):
    def __init__(self, c, att=128):
        super().__init__()
        self.tdnn = TDNNBlock(c * 3, att, 1)
        self.conv = _Conv(att, c, 1)

    @staticmethod
    def _stats(x, m, eps=1e-12):
        mean = (m * x).sum(2)
        std = torch.sqrt((m * (x - mean.unsqueeze(2)).pow(2)).sum(2).clamp(eps))
        return mean, std

    def forward(self, x, lengths, logits_out: Optional[list] = None):
        L = x.shape[-1]
        mask = length_to_mask(lengths * L, L, x.dtype).unsqueeze(1)
        total = mask.sum(dim=2, keepdim=True)
        mean, std = self._stats(x, mask / total)
        attn = torch.cat([x, mean.unsqueeze(2).repeat(1, 1, L), std.unsqueeze(2).repeat(1, 1, L)], dim=1)
        attn = self.conv(torch.tanh(self.tdnn(attn)))
        if logits_out is not None:
            logits_out.append(attn)          # before the -inf fill of the padding
        attn = attn.masked_fill(mask == 0, float("-inf"))
        attn = F.softmax(attn, dim=2)
        mean, std = self._stats(x, attn)
        return torch.cat((mean, std), dim=1).unsqueeze(2)


class EcapaTdnnRef(nn.Module):
    """(N, T, 80) features, relative lengths (N,) -> (N, 192)."""

    def __init__(self, channels=1024, lin_neurons=192):
        super().__init__()
        c = channels
        self.blocks = nn.ModuleList([TDNNBlock(N_MELS, c, 5, 1), SERes2NetBlock(c, 2), SERes2NetBlock(c, 3),
                                     SERes2NetBlock(c, 4)])
        self.mfa = TDNNBlock(3 * c, 3 * c, 1)
        self.asp = AttentiveStatisticsPooling(3 * c)
        self.asp_bn = _BN(6 * c)
        self.fc = _Conv(6 * c, lin_neurons, 1)

    def forward(self, feats, lengths, return_intermediate: bool = False):
        x = feats.transpose(1, 2)
        xl = []
        for i, layer in enumerate(self.blocks):
            x = layer(x) if i == 0 else layer(x, lengths)
            xl.append(x)
        cat = torch.cat(xl[1:], dim=1)
        m = self.mfa(cat)
        logits = [] if return_intermediate else None
        pooled = self.asp(m, lengths, logits)
        out = self.fc(self.asp_bn(pooled)).squeeze(2)
        if return_intermediate:
            return out, {"block0": xl[0], "cat": cat, "mfa": m, "logits": logits[0], "pooled": pooled.squeeze(2)}
        return out


class PretrainedSpeakerEmbeddingRef:
    """``__call__(waveforms (N,1,S), masks (N,F) | None) -> ndarray (N,192)`` with NaN rows.

    ``dtype=torch.float64`` runs the Fbank (window, DFT, mel bank) and the network in float64 while the relative
    lengths, and so every frame count they select, keep the reference's float32 arithmetic (``frame_counts``):
    the high-precision restatement the HIP path's stages are measured against."""

    dimension = 192

    def __init__(self, state: Optional[dict] = None, dtype: torch.dtype = torch.float32):
        self.dtype = dtype
        self.model = EcapaTdnnRef().eval()
        if state is not None:
            self.model.load_state_dict(state)
        self.model.to(dtype)

    def to(self, device):
        return self

    def select(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor]):
        """mask -> (padded kept samples (N, Lmax), kept counts (N,))."""
        N, _, S = waveforms.shape
        wav = waveforms[:, 0, :]
        if masks is None:
            return wav, torch.full((N,), S, dtype=torch.long)
        imasks = F.interpolate(masks.unsqueeze(1).float(), size=S, mode="nearest").squeeze(1) > 0.5
        kept = [w[m] for w, m in zip(wav, imasks)]
        return nn.utils.rnn.pad_sequence(kept, batch_first=True), imasks.sum(dim=1)

    def geometry(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> dict:
        """The batch geometry of one call: padded kept samples, kept counts, float32 relative lengths, T and the
        per-row frame counts (``frame_counts``).  ``signals`` is None when every row is too short."""
        signals, wav_lens = self.select(waveforms, masks)
        N, max_len = signals.shape
        too_short = wav_lens < MIN_NUM_SAMPLES
        if max_len < MIN_NUM_SAMPLES:
            return {"signals": None, "lens": wav_lens, "too_short": too_short, "T": 0}
        rel = wav_lens.float() / max_len
        rel[too_short] = 1.0
        T = 1 + max_len // HOP
        nvalid, nmask = frame_counts(rel, T)
        return {"signals": signals, "lens": wav_lens, "rel": rel, "too_short": too_short, "T": T,
                "nvalid": nvalid, "nmask": nmask}

    def stages(self, geom: dict, rows=slice(None)) -> dict:
        """Every stage for ``rows`` of the batch ``geom`` describes, in ``self.dtype``: feats (n,T,80), block0
        (n,T,1024), mfa (n,T,3072), logits (n,T,3072, before the -inf fill), pooled (n,6144), emb (n,192, NaN
        for too-short rows).  A row's stages depend on the others only through the padded length, so a batch can
        be computed a slice of rows at a time."""
        with torch.no_grad():
            rel = geom["rel"][rows]
            feats = sentence_mean_norm(fbank(geom["signals"][rows].to(self.dtype)), rel)
            emb, inter = self.model(feats, rel, return_intermediate=True)
            emb[geom["too_short"][rows]] = float("nan")
        return {"feats": feats, "block0": inter["block0"].transpose(1, 2), "mfa": inter["mfa"].transpose(1, 2),
                "logits": inter["logits"].transpose(1, 2), "pooled": inter["pooled"], "emb": emb}

    def __call__(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> np.ndarray:
        with torch.no_grad():
            geom = self.geometry(waveforms, masks)
            if geom["signals"] is None:
                return np.full((waveforms.shape[0], self.dimension), np.nan, dtype=np.float32)
            feats = sentence_mean_norm(fbank(geom["signals"].to(self.dtype)), geom["rel"])
            emb = self.model(feats, geom["rel"]).numpy().copy()
            emb[geom["too_short"].numpy()] = np.nan
            return emb
