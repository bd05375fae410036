"""Float64 restatement of speechbrain's x-vector (speechbrain/spkrec-xvect-voxceleb) behind pyannote's
``PretrainedSpeakerEmbedding`` for the tests: the wrapper's mask -> kept samples -> relative lengths geometry,
speechbrain ``Fbank(n_mels=24)`` + ``InputNormalization("sentence", std_norm=False)``, the five TDNN layers
(``F.conv1d`` after reflect "same" padding -> LeakyReLU(0.01) -> ``F.batch_norm``, BatchNorm NOT folded),
``StatisticsPooling`` with lengths and ``Linear(3000, 512)``.  The window, DFT, mel bank and network run in float64;
the relative lengths, and every frame count they select, keep the reference's float32 arithmetic
(``oracle.ecapa_ref.frame_counts``).  DESIGN.md "speechbrain x-vector" states the definition and marks with (R)
where it rests on a reading of the published speechbrain / pyannote code."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.ecapa_ref import frame_counts, mel_filterbank, sentence_mean_norm

SAMPLE_RATE, N_FFT, HOP, N_MELS = 16000, 400, 160, 24
# (R) Conv1d(padding="same", padding_mode="reflect"): pad = dilation (k - 1) / 2 per side = 2, 2, 3, 0, 0.  Reflect
# padding needs pad < frames, so the network accepts T >= 4 frames, T = 1 + n // 160: n >= 480.  pyannote bisects
# for the shortest input the network accepts (min_num_samples), which is this value.
PADS = (2, 2, 3, 0, 0)
MIN_NUM_SAMPLES = 480
KERNELS, DILATIONS = (5, 3, 3, 1, 1), (1, 2, 3, 1, 1)
CONV_KEYS = (0, 3, 6, 9, 12)
# (R) StatisticsPooling: eps = 1e-5 added to the std; the mean gets _get_gauss_noise, a band [eps, 9 eps]
STD_EPS = 1e-5
NOISE_MID = 5e-5


def min_num_samples() -> int:
    """The bisection pyannote runs, on the restated arithmetic: the smallest n for which every reflect pad fits."""
    return next(n for n in range(1, 2 * SAMPLE_RATE) if 1 + n // HOP > max(PADS))


def fbank(wavs: torch.Tensor) -> torch.Tensor:
    """(N, L) -> (N, 1 + L // 160, 24) log-mel in dB with top_db = 80 (per-row maximum over all frames of the
    padded batch), in the dtype of ``wavs``."""
    window = torch.hamming_window(N_FFT, dtype=wavs.dtype)
    spec = torch.stft(wavs, N_FFT, HOP, N_FFT, window, center=True, pad_mode="constant",
                      normalized=False, onesided=True, return_complex=True)
    power = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)
    mel = power @ mel_filterbank(n_mels=N_MELS, dtype=wavs.dtype)
    x_db = 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
    floor = x_db.amax(dim=(-2, -1)) - 80.0
    return torch.max(x_db, floor.view(-1, 1, 1))


def noise_band(shape, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(R) speechbrain StatisticsPooling._get_gauss_noise: randn, shifted to min 0, scaled to max 1, mapped
    affinely onto [1e-5, 9e-5] (the largest draw gets 1e-5, the smallest 9e-5)."""
    g = torch.randn(shape, generator=generator, dtype=torch.float64)
    g = g - g.min()
    g = g / g.max()
    return 1e-5 * ((1 - 9) * g + 9)


def stats_pool(x: torch.Tensor, rel: torch.Tensor, noise) -> torch.Tensor:
    """(R) StatisticsPooling(x (N, T, C), lengths): per row n = int(round(rel T)) frames (float32 arithmetic), mean
    and UNBIASED std over them (n = 1: std NaN, as torch.std), mean + noise, std + 1e-5.  ``noise``: a float added
    to every mean (the HIP path: 5e-5) or a torch.Generator drawing the reference's random band."""
    nvalid, _ = frame_counts(rel, x.shape[1])
    mean = torch.stack([x[i, :int(n)].mean(dim=0) for i, n in enumerate(nvalid)])
    std = torch.stack([x[i, :int(n)].std(dim=0) for i, n in enumerate(nvalid)])
    mean = mean + (noise_band(mean.shape, noise).to(mean.dtype) if isinstance(noise, torch.Generator) else noise)
    return torch.cat([mean, std + STD_EPS], dim=1)


class SbXvectorRef:
    dimension = 512

    def __init__(self, sd: Dict[str, torch.Tensor]):
        self.sd = {k: v.detach().double() for k, v in sd.items()}

    def tdnn(self, feats: torch.Tensor):
        """(N, T, 24) -> [five (N, T, C) channels-last layer outputs]."""
        s, x, out = self.sd, feats.transpose(1, 2), []
        for i, (k, d, pad) in enumerate(zip(KERNELS, DILATIONS, PADS)):
            c, n = f"blocks.{CONV_KEYS[i]}.conv", f"blocks.{CONV_KEYS[i] + 2}.norm"
            if pad:
                x = F.pad(x, (pad, pad), mode="reflect")
            x = F.leaky_relu(F.conv1d(x, s[c + ".weight"], s[c + ".bias"], dilation=d), 0.01)
            x = F.batch_norm(x, s[n + ".running_mean"], s[n + ".running_var"], s[n + ".weight"], s[n + ".bias"],
                             training=False, eps=1e-5)
            out.append(x.transpose(1, 2))
        return out

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
        too_short = lens < MIN_NUM_SAMPLES
        if signals.shape[1] < MIN_NUM_SAMPLES:
            return {"signals": None, "lens": lens, "too_short": too_short, "T": 0}
        rel = lens.float() / signals.shape[1]
        rel[too_short] = 1.0
        T = 1 + signals.shape[1] // HOP
        nvalid, _ = frame_counts(rel, T)
        return {"signals": signals, "lens": lens, "rel": rel, "too_short": too_short, "T": T, "nvalid": nvalid}

    def stages(self, geom: dict, noise=NOISE_MID) -> dict:
        """Every stage of the batch ``geom`` describes, float64: feats (N,T,24), tdnn1 .. tdnn5 (N,T,C), pooled
        (N,3000), emb (N,512; NaN for too-short rows)."""
        with torch.no_grad():
            feats = sentence_mean_norm(fbank(geom["signals"].double()), geom["rel"])
            xs = self.tdnn(feats)
            pooled = stats_pool(xs[4], geom["rel"], noise)
            emb = pooled @ self.sd["blocks.16.w.weight"].t() + self.sd["blocks.16.w.bias"]
            emb[geom["too_short"]] = float("nan")
        out = {"feats": feats, "pooled": pooled, "emb": emb}
        out.update({f"tdnn{i + 1}": x for i, x in enumerate(xs)})
        return out

    def __call__(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None, noise=NOISE_MID) -> torch.Tensor:
        """pyannote's ``PretrainedSpeakerEmbedding.__call__(waveforms (N,1,S), masks (N,F) | None)`` -> (N,512)
        float64 with NaN rows."""
        geom = self.geometry(waveforms, masks)
        if geom["signals"] is None:
            return torch.full((waveforms.shape[0], self.dimension), float("nan"), dtype=torch.float64)
        return self.stages(geom, noise)["emb"]

