"""Float64 restatement of NeMo's TitaNet-L (nvidia/speakerverification_en_titanet_large) behind pyannote's
``PretrainedSpeakerEmbedding`` NeMo wrapper, for the tests.  NeMo, pyannote and the checkpoint are not available
to the tests, so the definition is restated from the published NeMo / pyannote.audio code; DESIGN.md 4.12 states it
and lists the points marked (R) below, which rest on that reading.  Every (R) point that a release changed is a
named parameter here and in ``weights.PackedTitaNet``.

Wrapper: mask -> kept samples -> zero-padded batch, ``wav_lens`` = absolute kept counts, rows shorter than
``min_num_samples`` computed at the longest length and returned NaN, a batch whose longest row is too short all NaN;
the (N, 192) result is not normalised.
Front end (``AudioToMelSpectrogramPreprocessor``, eval): pre-emphasis 0.97, STFT n_fft 512 / symmetric Hann 400 /
hop 160 / centred, power, 80 slaney mel bins 0 - 8000 Hz, log(x + 2^-24), per-feature mean / unbiased std over
the row's valid frames, frames past them zero, time padded to a multiple of 16.
Encoder (``ConvASREncoder``, conv_mask): five separable Jasper blocks with squeeze-excitation, BatchNorm eps 1e-3
NOT folded.  Decoder: attentive statistics pooling, BatchNorm1d(6144), Conv1d(6144, 192, 1)."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

SAMPLE_RATE, N_FFT, WIN, HOP, N_MELS = 16000, 512, 400, 160, 80
PREEMPH, LOG_GUARD, STD_GUARD, BN_EPS = 0.97, 2.0 ** -24, 1e-5, 1e-3
# (repeats, kernel, C_in, C_out, residual) of encoder.encoder.{0..4}
BLOCKS = ((1, 3, 80, 1024, False), (3, 7, 1024, 1024, True), (3, 11, 1024, 1024, True), (3, 15, 1024, 1024, True),
          (1, 1, 1024, 3072, False))
EMB, ATT = 192, 128
PAD_MODES = ("reflect", "constant")
FRAME_COUNTS = ("floor_plus_one", "padded")
# (R) pyannote bisects for the shortest input the model accepts.  On this restatement that is the first length
# whose centre padding is defined in the reflect form (pad n_fft / 2 = 256 < length) — which also leaves two valid
# frames, so the unbiased std of the normalisation exists.  One value for both padding modes.
MIN_NUM_SAMPLES = N_FFT // 2 + 1


def mel_filterbank(dtype=torch.float64) -> torch.Tensor:
    """librosa.filters.mel(sr=16000, n_fft=512, n_mels=80, fmin=0, fmax=8000, htk=False, norm="slaney") as
    (257, 80): what NeMo's FilterbankFeatures multiplies the power spectrum with."""
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    to_mel = lambda hz: hz / f_sp if hz < min_log_hz else min_log_mel + math.log(hz / min_log_hz) / logstep
    mels = torch.linspace(to_mel(0.0), to_mel(SAMPLE_RATE / 2.0), N_MELS + 2, dtype=torch.float64)
    hz = torch.where(mels < min_log_mel, mels * f_sp, min_log_hz * torch.exp(logstep * (mels - min_log_mel)))
    freqs = torch.linspace(0.0, SAMPLE_RATE / 2.0, N_FFT // 2 + 1, dtype=torch.float64)
    lower = (freqs[None, :] - hz[:-2, None]) / (hz[1:-1] - hz[:-2])[:, None]
    upper = (hz[2:, None] - freqs[None, :]) / (hz[2:] - hz[1:-1])[:, None]
    w = torch.clamp(torch.minimum(lower, upper), min=0.0) * (2.0 / (hz[2:] - hz[:-2]))[:, None]
    return w.t().contiguous().to(dtype)


def valid_frames(lens: torch.Tensor, frame_count: str = "floor_plus_one") -> torch.Tensor:
    """(R) frames NeMo counts as valid for ``lens`` samples: ``len // hop + 1`` ("floor_plus_one") or
    ``(len + 2 (n_fft // 2) - n_fft) // hop + 1`` ("padded", newer releases)."""
    if frame_count == "floor_plus_one":
        return lens // HOP + 1
    if frame_count == "padded":
        return (lens + 2 * (N_FFT // 2) - N_FFT) // HOP + 1
    raise ValueError(f"frame_count={frame_count!r}: expected one of {FRAME_COUNTS}")


class TitaNetRef:
    dimension = EMB

    def __init__(self, sd: Dict[str, torch.Tensor], pad_mode: str = "reflect", frame_count: str = "floor_plus_one",
                 min_num_samples: int = MIN_NUM_SAMPLES, attention_order: str = "relu_bn_tanh", dtype=torch.float64):
        """(R) ``pad_mode``: the centred STFT's padding, "reflect" (older NeMo) | "constant" (newer);
        (R) ``frame_count``: ``valid_frames``; (R) ``attention_order``: "relu_bn_tanh" (TDNNModule = conv -> ReLU ->
        BatchNorm, then Tanh) | "bn_relu_tanh"; ``dtype``: float64, or float32 to measure what f32 arithmetic gives."""
        if pad_mode not in PAD_MODES:
            raise ValueError(f"pad_mode={pad_mode!r}: expected one of {PAD_MODES}")
        assert attention_order in ("relu_bn_tanh", "bn_relu_tanh")
        self.dtype = dtype
        self.sd = {k: v.detach().to(dtype) for k, v in sd.items() if v.is_floating_point()}
        self.pad_mode, self.frame_count, self.min_num_samples = pad_mode, frame_count, int(min_num_samples)
        self.attention_order = attention_order

    # ------------------------------------------------------------------ wrapper
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
        too_short = lens < self.min_num_samples
        if signals.shape[1] < self.min_num_samples:
            return {"signals": None, "lens": lens, "too_short": too_short}
        lens = lens.clone()
        lens[too_short] = signals.shape[1]
        return {"signals": signals, "lens": lens, "too_short": too_short,
                "frames": valid_frames(lens, self.frame_count)}

    # ------------------------------------------------------------------ front end
    def features(self, signals: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """(N, L) zero-padded signals, (N,) lengths -> (N, Tpad, 80) normalised log-mel, zero past each row's frames."""
        x = signals.to(self.dtype)
        L = x.shape[1]
        x = torch.cat([x[:, :1], x[:, 1:] - PREEMPH * x[:, :-1]], dim=1)
        x = x * (torch.arange(L)[None, :] < lens[:, None])           # (R) the pre-emphasised signal is masked at len
        window = torch.hann_window(WIN, periodic=False, dtype=self.dtype)
        spec = torch.stft(x, N_FFT, HOP, WIN, window, center=True, pad_mode=self.pad_mode, normalized=False,
                          onesided=True, return_complex=True)
        power = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)                   # (N, T, 257)
        logmel = torch.log(power @ mel_filterbank(self.dtype) + LOG_GUARD)
        frames = valid_frames(lens, self.frame_count)
        out = torch.zeros_like(logmel)
        for i, n in enumerate(frames.tolist()):
            v = logmel[i, :n]
            out[i, :n] = (v - v.mean(dim=0)) / (v.std(dim=0) + STD_GUARD)            # (n = 1: NaN, as torch.std)
        T = out.shape[1]
        return F.pad(out, (0, 0, 0, (-T) % 16))

    # ------------------------------------------------------------------ encoder
    def _bn(self, x, prefix, eps=BN_EPS):
        s = self.sd
        return F.batch_norm(x, s[prefix + ".running_mean"], s[prefix + ".running_var"], s[prefix + ".weight"],
                            s[prefix + ".bias"], training=False, eps=eps)

    def block(self, i: int, x: torch.Tensor, frames: torch.Tensor) -> torch.Tensor:
        """Jasper block i over x (N, C, T) with ``frames`` valid frames per row."""
        s, (R, k, cin, cout, residual) = self.sd, BLOCKS[i]
        p = f"encoder.encoder.{i}."
        mask = (torch.arange(x.shape[2])[None, :] < frames[:, None])[:, None, :].to(x.dtype)
        y = x
        for j in range(R):
            y = F.conv1d(y * mask, s[p + f"mconv.{5 * j}.conv.weight"], padding=k // 2, groups=y.shape[1])
            y = F.conv1d(y * mask, s[p + f"mconv.{5 * j + 1}.conv.weight"])
            y = self._bn(y, p + f"mconv.{5 * j + 2}")
            if j < R - 1:
                y = F.relu(y)
        se = p + f"mconv.{5 * (R - 1) + 3}.fc."
        y = y * mask
        ctx = y.sum(dim=2) / frames[:, None].to(y.dtype)
        gate = torch.sigmoid(F.relu(ctx @ s[se + "0.weight"].t()) @ s[se + "2.weight"].t())
        y = y * gate[:, :, None]
        if residual:
            y = y + self._bn(F.conv1d(x * mask, s[p + "res.0.0.conv.weight"]), p + "res.0.1")
        return F.relu(y)

    # ------------------------------------------------------------------ decoder
    def pool(self, x: torch.Tensor, frames: torch.Tensor) -> torch.Tensor:
        """Attentive statistics pooling of x (N, 3072, T) -> (N, 6144)."""
        s, a = self.sd, "decoder._pooling.attention_layer."
        mask = (torch.arange(x.shape[2])[None, :] < frames[:, None])[:, None, :]

        def stats(w):
            mean = (w * x).sum(dim=2)
            return mean, torch.sqrt(((w * (x - mean[:, :, None]) ** 2).sum(dim=2)).clamp(min=1e-12))

        mean, std = stats(mask.to(x.dtype) / frames[:, None, None].to(x.dtype))
        T = x.shape[2]
        att = torch.cat([x, mean[:, :, None].expand(-1, -1, T), std[:, :, None].expand(-1, -1, T)], dim=1)
        att = F.conv1d(att, s[a + "0.conv_layer.weight"], s[a + "0.conv_layer.bias"])
        att = (self._bn(F.relu(att), a + "0.bn", 1e-5) if self.attention_order == "relu_bn_tanh"
               else F.relu(self._bn(att, a + "0.bn", 1e-5)))
        att = F.conv1d(torch.tanh(att), s[a + "2.weight"], s[a + "2.bias"])
        alpha = torch.softmax(att.masked_fill(~mask, float("-inf")), dim=2)
        return torch.cat(stats(alpha), dim=1)

    def stages(self, geom: dict) -> dict:
        """feats (N,Tpad,80), block0 .. block4 (N,Tpad,C) channels-last, pooled (N,6144), emb (N,192; NaN rows)."""
        s = self.sd
        with torch.no_grad():
            frames = geom["frames"]
            feats = self.features(geom["signals"], geom["lens"])
            out, x = {"feats": feats}, feats.transpose(1, 2)
            for i in range(len(BLOCKS)):
                x = self.block(i, x, frames)
                out[f"block{i}"] = x.transpose(1, 2)
            pooled = self.pool(x, frames)
            e = "decoder.emb_layers.0."
            z = F.batch_norm(pooled, s[e + "0.running_mean"], s[e + "0.running_var"], s[e + "0.weight"], s[e + "0.bias"],
                             training=False, eps=1e-5)
            emb = z @ s[e + "1.weight"][:, :, 0].t() + s[e + "1.bias"]
            emb[geom["too_short"]] = float("nan")
        out.update(pooled=pooled, emb=emb)
        return out

    def __call__(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``NeMoPretrainedSpeakerEmbedding.__call__(waveforms (N,1,S), masks (N,F) | None)`` -> (N,192) with NaN rows."""
        geom = self.geometry(waveforms, masks)
        if geom["signals"] is None:
            return torch.full((waveforms.shape[0], EMB), float("nan"), dtype=self.dtype)
        return self.stages(geom)["emb"]


def parameter_count(sd: Dict[str, torch.Tensor]) -> int:
    """Trainable parameters of a state dict in NeMo's keys (running statistics and counters are buffers)."""
    return sum(v.numel() for k, v in sd.items()
               if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
