"""Float64 restatement of the mel-spectrogram ECAPA-TDNN call (TEST INFRASTRUCTURE).

``speechbrain/spkrec-ecapa-voxceleb-mel-spec`` behind pyannote's ``PretrainedSpeakerEmbedding``: the masked call of
``oracle/ecapa_ref.py::PretrainedSpeakerEmbeddingRef`` (kept samples, zero padding to the longest kept row, float32
relative lengths, NaN rows) in front of speechbrain's ``MelSpectrogramEncoder.encode_waveform``: torchaudio's
``MelSpectrogram(16000, n_fft=1024, win_length=1024, hop_length=256, f_min=0, f_max=8000, n_mels=80, power=1,
norm="slaney", mel_scale="slaney", center=True, pad_mode="reflect")`` on the PADDED batch, ``log(clamp(x, 1e-5))``,
``InputNormalization("sentence", std_norm=False)`` and ``ECAPA_TDNN``.  Neither speechbrain nor torchaudio is
installed here and the checkpoint has not been seen: every point that is a reading is marked (R) in DESIGN.md 4.15.

The STFT is written out (reflect padding, framing, window, ``torch.fft.rfft``) instead of calling ``torch.stft``, which
the host test compares it with; the mel bank is written from torchaudio's ``melscale_fbanks`` formulas, not taken from
``diart_amd.weights``.  ``EcapaTdnnRef``, ``sentence_mean_norm`` and ``frame_counts`` are oracle/ecapa_ref.py's.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ecapa_ref import EcapaTdnnRef, PretrainedSpeakerEmbeddingRef, frame_counts, sentence_mean_norm

SAMPLE_RATE, N_FFT, HOP, N_MELS, LOG_FLOOR = 16000, 1024, 256, 80, 1e-5
# reflect padding of 4 frames (k = 3, dilation 4) needs T = 1 + n // 256 >= 5 frames; the STFT's own reflect padding
# needs n > 512
MIN_NUM_SAMPLES = 1024


def reflect_index(i: np.ndarray, n: int) -> np.ndarray:
    """Index ``i`` of a signal of ``n`` samples under reflect padding: ``i < 0`` reads ``-i``, ``i >= n`` reads
    ``2 (n - 1) - i``."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def frames(wavs: torch.Tensor) -> torch.Tensor:
    """(N, L) -> (N, 1 + L // 256, 1024): the frames of the centred STFT, reflected at L (the padded batch's length)."""
    N, L = wavs.shape
    T = 1 + L // HOP
    idx = (np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]) - N_FFT // 2
    return wavs[:, torch.from_numpy(reflect_index(idx, L))]


def stft(wavs: torch.Tensor) -> torch.Tensor:
    """(N, L) -> complex (N, T, 513): rfft of the periodic-Hann-windowed frames, in the dtype of ``wavs``."""
    window = torch.hann_window(N_FFT, periodic=True, dtype=wavs.dtype)
    return torch.fft.rfft(frames(wavs) * window, dim=-1)


def hz_to_mel(f: float) -> float:
    """The slaney scale: 200 / 3 Hz per mel below 1 kHz, 27 mels per factor 6.4 above."""
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)


def mel_to_hz(m: torch.Tensor) -> torch.Tensor:
    return torch.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * torch.exp((m - 15.0) * (math.log(6.4) / 27.0)))


def mel_points(f_min: float = 0.0, f_max: float = 8000.0, dtype=torch.float64) -> torch.Tensor:
    """The n_mels + 2 band edges in Hz: equally spaced on the slaney scale."""
    return mel_to_hz(torch.linspace(hz_to_mel(f_min), hz_to_mel(f_max), N_MELS + 2, dtype=dtype))


def mel_filterbank(f_min: float = 0.0, f_max: float = 8000.0, dtype=torch.float64) -> torch.Tensor:
    """torchaudio.functional.melscale_fbanks(513, f_min, f_max, 80, 16000, norm="slaney", mel_scale="slaney"): (513, 80)."""
    all_freqs = torch.linspace(0, SAMPLE_RATE // 2, N_FFT // 2 + 1, dtype=dtype)
    f_pts = mel_points(f_min, f_max, dtype)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0.0)
    return fb * (2.0 / (f_pts[2:] - f_pts[:-2]))[None, :]


def magnitude(wavs: torch.Tensor) -> torch.Tensor:
    s = stft(wavs)
    return torch.sqrt(s.real ** 2 + s.imag ** 2)


def log_mel(wavs: torch.Tensor) -> torch.Tensor:
    """(N, L) -> (N, T, 80): log(clamp(|STFT| @ bank, 1e-5)), in the dtype of ``wavs``."""
    return torch.log(torch.clamp(magnitude(wavs) @ mel_filterbank(dtype=wavs.dtype), min=LOG_FLOOR))


def geometry_of_lengths(lens, min_num_samples: int = MIN_NUM_SAMPLES) -> dict:
    """The batch geometry of a call whose rows keep ``lens`` samples, in the float32 arithmetic of the reference:
    Lmax, T = 1 + Lmax // 256, too-short flags, nvalid and nmask (``frame_counts``).  T = 0 when every row is too short."""
    lens = torch.as_tensor(lens, dtype=torch.long)
    lmax = int(lens.max())
    too_short = lens < min_num_samples
    if lmax < min_num_samples:
        z = torch.zeros_like(lens)
        return {"lmax": lmax, "T": 0, "too_short": torch.ones_like(too_short), "nvalid": z, "nmask": z}
    rel = lens.float() / lmax
    rel[too_short] = 1.0
    T = 1 + lmax // HOP
    nvalid, nmask = frame_counts(rel, T)
    return {"lmax": lmax, "T": T, "too_short": too_short, "rel": rel, "nvalid": nvalid, "nmask": nmask}


def rounding_edges(lmax: int, lo: int = MIN_NUM_SAMPLES) -> dict:
    """The hop-256 counterpart of oracle/ecapa_ref.py's ``rounding_edges``: kept lengths in ``[lo, lmax]`` where
    ``float32(len / lmax) * T``, T = 1 + lmax // 256, is an integer ("int"), on k + 0.5 ("half"), within one float32
    ulp of either but not on it ("near"), or rounds / ceils differently from the exact rational ("differs")."""
    from fractions import Fraction
    T = 1 + lmax // HOP
    lens = np.arange(lo, lmax + 1)
    v = (lens.astype(np.float32) / np.float32(lmax)) * np.float32(T)
    frac2 = v * np.float32(2)
    on_grid = frac2 == np.round(frac2)
    is_int = v == np.round(v)
    near = ~on_grid & (np.abs(frac2 - np.round(frac2)) <= np.float32(2) * np.spacing(v))
    differs = []
    for i in np.flatnonzero(on_grid | near):
        x = Fraction(int(lens[i]) * T, lmax)
        fl = x.numerator // x.denominator
        r = x - fl
        exact_round = fl + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2) else 0)
        exact_ceil = fl + (1 if r else 0)
        if int(np.rint(v[i])) != exact_round or int(np.ceil(v[i])) != exact_ceil:
            differs.append(int(lens[i]))
    return {"T": T, "int": lens[is_int].tolist(), "half": lens[on_grid & ~is_int].tolist(),
            "near": lens[near].tolist(), "differs": differs}


class MelSpecEmbeddingRef(PretrainedSpeakerEmbeddingRef):
    """``__call__(waveforms (N,1,S), masks (N,F) | None) -> ndarray (N,192)`` with NaN rows: the wrapper's call (``select``
    is the parent's) with this model's geometry (hop 256, ``min_num_samples`` 1024) and features."""

    def __init__(self, state: Optional[dict] = None, dtype: torch.dtype = torch.float64,
                 min_num_samples: int = MIN_NUM_SAMPLES):
        super().__init__(state, dtype)
        self.min_num_samples = min_num_samples

    def geometry(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> dict:
        signals, wav_lens = self.select(waveforms, masks)
        geom = geometry_of_lengths(wav_lens, self.min_num_samples)
        geom.update(signals=signals if geom["T"] else None, lens=wav_lens)
        return geom

    def stages(self, geom: dict, rows=slice(None)) -> dict:
        """Every stage for ``rows`` of the batch ``geom`` describes, in ``self.dtype``: mag (n,T,513), feats (n,T,80),
        block0 (n,T,1024), mfa (n,T,3072), pooled (n,6144), emb (n,192; NaN for too-short rows)."""
        with torch.no_grad():
            rel = geom["rel"][rows]
            sig = geom["signals"][rows].to(self.dtype)
            feats = sentence_mean_norm(log_mel(sig), rel)
            emb, inter = self.model(feats, rel, return_intermediate=True)
            emb[geom["too_short"][rows]] = float("nan")
        return {"mag": magnitude(sig), "feats": feats, "block0": inter["block0"].transpose(1, 2),
                "mfa": inter["mfa"].transpose(1, 2), "pooled": inter["pooled"], "emb": emb}

    def embed(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The call's embeddings (N,192) in ``self.dtype``, NaN rows kept (what tests/titanet_chain.py's ``embed`` takes)."""
        geom = self.geometry(waveforms, masks)
        if geom["signals"] is None:
            return torch.full((waveforms.shape[0], self.dimension), float("nan"), dtype=self.dtype)
        return self.stages(geom)["emb"]

    def __call__(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> np.ndarray:
        return self.embed(waveforms, masks).float().numpy()
