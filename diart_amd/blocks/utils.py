"""``Binarize``: frame scores -> speech turns (reference:
``/root/reference/src/diart/blocks/utils.py:11-59``).  Same turns, found per speaker from the
rising / falling edges of ``score > threshold`` instead of a Python loop over frames; turn
boundaries are frame middles, a turn still open at the last frame closes at the middle of the
(virtual) frame after it, labels are ``speaker{index}`` and the track is the speaker index."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..features import Annotation, Segment, SlidingWindowFeature, TemporalFeatureFormatter, TemporalFeatures
from ..functional import _gpu, _target_db, adjust_volume, adjust_volume_rows, resample, resampler  # noqa: F401


def windows_batch(waveforms: Sequence[SlidingWindowFeature], device=None) -> torch.Tensor:
    """``(batch, samples, channels)`` float tensor of the chunks' audio ON ``device`` — what the reference builds
    with ``torch.stack`` (/root/reference/src/diart/blocks/diarization.py:175) and each block then uploads on its
    own (segmentation.py:47, embedding.py:52: the same 320 KB per chunk twice).  Here the batch is uploaded ONCE
    and both blocks get the device tensor.  When the chunks are overlapping views of one host buffer at a
    constant hop — what a rolling window over a file or a stream is: 32 windows of 5 s at a 500 ms step are 20.5 s
    of audio, not 160 s — only the span they cover crosses PCIe and the batch is a strided view of it on the device
    (the kernels read rows at any stride).  Values are identical either way."""
    datas = [w.data for w in waveforms]
    dev = torch.device("cpu") if device is None else torch.device(device)
    span = _common_span(datas) if dev.type == "cuda" else None
    if span is not None:
        flat, hop, n = span
        import warnings
        with warnings.catch_warnings():          # (a read-only source buffer: nothing here writes through the view)
            warnings.simplefilter("ignore", UserWarning)
            d = torch.from_numpy(flat).to(dev)
        return d.as_strided((len(datas), n, 1), (hop, 1, 1))
    return torch.stack([torch.from_numpy(x) for x in datas]).to(dev)


def _common_span(datas):
    """(1-D host view covering every window, hop in samples, samples per window) when the windows are mono float32
    views of ONE buffer at a constant, 16-byte aligned, non-negative hop; else None."""
    if len(datas) < 2:
        return None
    first = datas[0]
    if not isinstance(first, np.ndarray) or first.dtype != np.float32 or first.ndim != 2 or first.shape[1] != 1:
        return None
    n = first.shape[0]

    def owner(a):
        while isinstance(getattr(a, "base", None), np.ndarray):
            a = a.base
        return a

    root = owner(first)
    if root is first or not isinstance(root, np.ndarray):
        return None
    addrs = []
    for x in datas:
        if not isinstance(x, np.ndarray) or x.dtype != np.float32 or x.shape != (n, 1) or x.strides[0] != 4 or owner(x) is not root:
            return None
        addrs.append(x.__array_interface__["data"][0])
    hop_b = addrs[1] - addrs[0]
    if hop_b < 0 or hop_b % 16 or any(b - a != hop_b for a, b in zip(addrs, addrs[1:])):
        return None
    if hop_b >= 4 * n:          # windows that do not overlap (far apart in one large or mmap'd buffer): the span would
        return None             # move MORE than the stacked batch does
    lo, hi = root.__array_interface__["data"][0], root.__array_interface__["data"][0] + root.nbytes
    if not root.flags["C_CONTIGUOUS"] or addrs[0] < lo or addrs[-1] + 4 * n > hi:
        return None
    total = (addrs[-1] - addrs[0]) // 4 + n
    flat = np.lib.stride_tricks.as_strided(first[:, 0], shape=(total,), strides=(4,))
    return flat, hop_b // 4, n


class Binarize:
    """Frame scores -> speech turns.  ``offset=None``: ``score > threshold`` (the reference).  ``offset``: hysteresis,
    pyannote's onset / offset — a frame of a column is on when its score is > ``threshold`` while the column is off and
    > ``offset`` while it is on.  The state is kept per column, starts off, crosses from one call into the next (a
    call is one step of one stream, so the column count may not change between calls) and is cleared by ``reset()``; a NaN frame is off and leaves the state off.  The
    turns are formed from the frames as before: a turn open at the last frame is closed there."""

    def __init__(self, threshold: float, uri: Optional[str] = None, offset: Optional[float] = None):
        from .base import check_tau_offset
        self.uri, self.threshold = uri, threshold
        self.offset = check_tau_offset(offset, "Binarize(offset=)")
        self._state: Optional[np.ndarray] = None

    def reset(self):
        self._state = None

    def _active(self, data: np.ndarray) -> np.ndarray:
        if self.offset is None:
            return data > self.threshold                         # strict, utils.py:45
        num_frames, num_speakers = data.shape
        if self._state is None:
            self._state = np.zeros(num_speakers, dtype=bool)
        elif self._state.shape != (num_speakers,):
            raise ValueError(f"Binarize(offset=): {num_speakers} columns, but the state carried from the call before has "
                             f"{self._state.shape[0]}; reset() starts another stream")
        data = np.asarray(data, dtype=np.float64)
        on = np.empty((num_frames, num_speakers), dtype=bool)
        state = self._state
        for r in range(num_frames):
            state = data[r] > np.where(state, self.offset, self.threshold)
            on[r] = state
        self._state = state
        return on

    def __call__(self, segmentation: SlidingWindowFeature) -> Annotation:
        num_frames, num_speakers = segmentation.data.shape
        ts = segmentation.sliding_window
        active = np.zeros((num_frames + 2, num_speakers), dtype=np.int8)
        active[1:-1] = self._active(segmentation.data)
        edges = np.diff(active, axis=0)                          # (num_frames + 1, speakers)
        annotation = Annotation(uri=self.uri, modality="speech")
        for spk in np.nonzero(edges.any(axis=0))[0]:
            onsets = np.nonzero(edges[:, spk] == 1)[0]           # first active frame
            offsets = np.nonzero(edges[:, spk] == -1)[0]         # first inactive frame after it
            for a, b in zip(onsets, offsets):
                annotation[Segment(ts[int(a)].middle, ts[int(b)].middle), int(spk)] = f"speaker{spk}"
        return annotation


class Resample:
    """Resample audio chunks (reference ``blocks/utils.py:62-89``, ``torchaudio.transforms.Resample``) on the GPU:
    ``(batch, samples, channels)`` or ``(samples, channels)`` features in, the same kind out, each chunk resampled
    on its own along the sample axis.  A ``SlidingWindowFeature`` keeps its start time and gets the resolution
    duration / samples.  ``resample`` is the functional form for whole signals."""

    def __init__(self, sample_rate: int, resample_rate: int, device: Optional[torch.device] = None):
        self.sample_rate, self.resample_rate = int(sample_rate), int(resample_rate)
        self.resample = resampler(self.sample_rate, self.resample_rate, device)
        self.device = self.resample.device
        self.formatter = TemporalFeatureFormatter()

    def __call__(self, waveform: TemporalFeatures) -> TemporalFeatures:
        wav = self.formatter.cast(waveform).to(self.device)  # (batch, samples, channels)
        if self.sample_rate == self.resample_rate:
            return self.formatter.restore_type(wav)
        out = self.resample(wav.transpose(-1, -2)).transpose(-1, -2)
        return self.formatter.restore_type(out)



class AdjustVolume:
    """Change the volume of audio chunks (reference ``blocks/utils.py:92-137``) on the GPU: ``(batch, samples,
    channels)`` or ``(samples, channels)`` features in, the same kind out, every (chunk, channel) signal scaled to
    ``volume_in_db`` dB on its own and, where that would exceed full scale, divided by its scaled peak — so the output
    volume may be lower than asked for.  As in the reference a chunk of zero energy, or with a NaN / Inf sample, comes
    out all NaN.  A ``SlidingWindowFeature`` keeps its sliding window.  ``adjust_volume`` is the functional form."""

    def __init__(self, volume_in_db: float, device: Optional[torch.device] = None):
        self.target_db = _target_db(volume_in_db)
        self.device = None if device is None else torch.device(device)
        self.formatter = TemporalFeatureFormatter()

    @staticmethod
    def get_volumes(waveforms: torch.Tensor) -> torch.Tensor:
        """Volumes in dB of audio chunks ``(batch, samples, channels)``, per channel: ``(batch, 1, channels)``."""
        return 10 * torch.log10(waveforms.square().mean(dim=1, keepdim=True))

    def __call__(self, waveform: TemporalFeatures) -> TemporalFeatures:
        wav = self.formatter.cast(waveform)          # (batch, samples, channels)
        src = wav.device
        dev = _gpu(src if src.type == "cuda" else self.device)
        B, S, C = wav.shape
        x = wav.to(dev).contiguous().reshape(B, S * C)
        out = adjust_volume_rows(x, self.target_db, channels=C).reshape(B, S, C)
        return self.formatter.restore_type(out if src == dev else out.to(src))
