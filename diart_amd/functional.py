"""Tensor functions of the hot path, computed by HIP kernels.

Same names and results as ``/root/reference/src/diart/functional.py`` (:6-13
``overlapped_speech_penalty``, :16-27 ``normalize_embeddings``), plus ``resample`` and ``adjust_volume``, the
functional forms of the ``Resample`` and ``AdjustVolume`` blocks, and ``decode_pcm``, the push kernel's sample
conversion over one buffer, and ``overlap_track``, the per-frame reduction of ``OverlappedSpeechDetection`` (the one
function here that answers a host tensor on the host: its definition is a torch statement), and ``min_duration``,
which is no tensor function at all: the rule of the track pipelines' minimum durations on an annotation, host
bookkeeping at the end of a file.  Inputs may live on the host
(the reference runs these on CPU tensors) or on the GPU; the result comes back on the device
of the input.  There is no torch fallback: without ``libdiart_amd.so`` and a GPU they raise.

``linkage_centroid`` and ``cut_linkage`` are the clustering of the whole-file mode (``offline.py``):
a CUDA tensor runs the HIP kernels of ``csrc/k_agglo.hip``, a host array the same text compiled for the host, which is
the library's own code and no fallback to another implementation.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _lib


def _gpu(device: Optional[torch.device] = None) -> torch.device:
    if device is not None and device.type == "cuda":
        return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
    if not torch.cuda.is_available():
        raise _lib.DiartAmdError("diart_amd.functional needs an MI355X GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def overlapped_speech_penalty(segmentation: torch.Tensor, gamma: float = 3, beta: float = 10,
                              normalize: bool = False, speaker_major: bool = False) -> torch.Tensor:
    """segmentation (batch, frames, speakers) -> weights (paper Eq. 2), same shape —
    or (batch, speakers, frames) with ``speaker_major`` (the layout the pooling kernel reads).
    ``normalize`` adds the per-(batch, speaker) min-max of ``blocks/embedding.py:102-106``."""
    if segmentation.ndim != 3:
        raise ValueError("segmentation must be (batch, frames, speakers)")
    src = segmentation.device
    dev = _gpu(src)
    seg = segmentation.to(dev, torch.float32).contiguous()
    B, F, K = seg.shape
    out = torch.empty((B, K, F) if speaker_major else (B, F, K), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().dz_osp(_lib.context(dev.index), seg.data_ptr(), B, F, K, float(gamma),
                                  float(beta), int(bool(normalize)), int(bool(speaker_major)),
                                  out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "dz_osp")
    return out if src == dev else out.to(src)


def normalize_embeddings(embeddings: torch.Tensor, norm: Union[float, torch.Tensor] = 1) -> torch.Tensor:
    """(batch, speakers, feat) or (speakers, feat) -> 3-D tensor with L2 norm ``norm``."""
    if embeddings.ndim == 2:
        embeddings = embeddings.unsqueeze(0)
    if isinstance(norm, torch.Tensor):
        b1, s1, _ = norm.shape
        b2, s2, _ = embeddings.shape
        assert b1 == b2 and s1 == s2
    src = embeddings.device
    dev = _gpu(src)
    out = embeddings.to(dev, torch.float32).contiguous().clone()
    B, K, D = out.shape
    _lib.check(_lib.load().dz_l2_normalize(_lib.context(dev.index), out.data_ptr(), B * K, D, 1.0,
                                           torch.cuda.current_stream(dev).cuda_stream), "dz_l2_normalize")
    if isinstance(norm, torch.Tensor):
        out = norm.to(dev) * out
    elif norm != 1:
        out = norm * out
    return out if src == dev else out.to(src)


class Resampler:
    """``orig_freq`` -> ``new_freq`` on one GPU (``dz_resample_*``): torchaudio's ``sinc_interp_hann`` resampler with
    its defaults, the filter built once in float64 and rounded to float32 (DESIGN.md "Resampling").  Each output is
    one f32 fused-multiply-add chain over its taps, so a signal's outputs do not depend on the batch it comes in."""

    def __init__(self, orig_freq: int, new_freq: int, device: Optional[torch.device] = None):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.device = _gpu(device)
        self._lib = _lib.load()
        self._h = _lib.vp()
        _lib.check(self._lib.dz_resample_create(_lib.context(self.device.index), self.orig_freq, self.new_freq,
                                                _lib.C.byref(self._h)), "dz_resample_create")

    def out_len(self, in_len: int) -> int:
        n = self._lib.dz_resample_out_len(self.orig_freq, self.new_freq, int(in_len))
        if n < 0:
            raise ValueError(f"{in_len} samples at {self.orig_freq} Hz have no output length at {self.new_freq} Hz")
        return int(n)

    def rows(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x`` (rows, L) float32 on this device, rows at any stride (a ring or window-batch view is read in
        place) -> ``out`` (rows, out_len(L)), allocated when not given.  Enqueued on the current stream."""
        assert x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1
        R, L = x.shape
        M = self.out_len(L)
        if out is None:
            out = torch.empty((R, M), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (R, M) and out.stride(1) == 1
        _lib.check(self._lib.dz_resample_forward(self._h, x.data_ptr(), x.stride(0), L, R, out.data_ptr(),
                                                 out.stride(0), torch.cuda.current_stream(self.device).cuda_stream),
                   "dz_resample_forward")
        return out

    def __call__(self, waveform: torch.Tensor) -> torch.Tensor:
        """(..., L) on the host or the GPU -> (..., out_len(L)) on the device of the input."""
        src = waveform.device
        lead, L = waveform.shape[:-1], waveform.shape[-1]
        x = waveform.to(self.device, torch.float32).reshape(-1, L)
        if x.stride(1) != 1:
            x = x.contiguous()
        y = self.rows(x).reshape(*lead, -1)
        return y if src == self.device else y.to(src)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.dz_resample_destroy(h)
            self._h = None


_resamplers = {}


def resampler(orig_freq: int, new_freq: int, device: Optional[torch.device] = None) -> Resampler:
    """The process's ``Resampler`` for (GPU, orig_freq, new_freq), created on first use."""
    dev = _gpu(device)
    key = (dev.index, int(orig_freq), int(new_freq))
    if key not in _resamplers:
        _resamplers[key] = Resampler(orig_freq, new_freq, dev)
    return _resamplers[key]


def resample(waveform, orig_freq: int, new_freq: int, device: Optional[torch.device] = None):
    """``torchaudio.functional.resample(waveform, orig_freq, new_freq)`` over the last axis, on the GPU.  A tensor
    comes back on its own device, a numpy array as a float32 array; equal rates return ``waveform`` itself."""
    if int(orig_freq) == int(new_freq):
        return waveform
    if isinstance(waveform, torch.Tensor):
        return resampler(orig_freq, new_freq, device if waveform.device.type != "cuda" else waveform.device)(waveform)
    import numpy as np
    x = torch.from_numpy(np.ascontiguousarray(waveform, dtype=np.float32))
    return resampler(orig_freq, new_freq, device)(x).numpy()


def _target_db(volume_in_db) -> float:
    """``volume_in_db`` as a finite float, or ``ValueError`` (before anything touches a device)."""
    import math
    import numbers
    if isinstance(volume_in_db, bool) or not isinstance(volume_in_db, numbers.Real) or not math.isfinite(volume_in_db):
        raise ValueError(f"volume_in_db={volume_in_db!r} (expected a finite number of dB)")
    return float(volume_in_db)


def adjust_volume_rows(x: torch.Tensor, volume_in_db: float, out: Optional[torch.Tensor] = None,
                       channels: int = 1) -> torch.Tensor:
    """``x`` (rows, samples * channels) float32 on a GPU, a row's channels interleaved, rows at any stride (a ring or
    window-batch view is read in place) -> ``out`` of the same shape (allocated when not given; ``out is x``: in
    place), every (row, channel) signal brought to ``volume_in_db`` on its own (``dz_adjust_volume``, DESIGN.md
    "Volume adjustment").  Enqueued on the current stream."""
    target = _target_db(volume_in_db)
    assert x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1
    R, L = x.shape
    if not (1 <= channels <= 8) or L % channels or R < 1 or L < 1:
        raise ValueError(f"adjust_volume_rows: {R} rows of {L} values in {channels} channels")
    if out is None:
        out = torch.empty((R, L), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.device == x.device and out.dtype == torch.float32 and tuple(out.shape) == (R, L) \
        and out.stride(1) == 1
    # one row: its stride is never used (and torch reports any number for it)
    xs, os_ = (L, L) if R == 1 else (x.stride(0), out.stride(0))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dz_adjust_volume(_lib.context(x.device.index), x.data_ptr(), xs, out.data_ptr(), os_, R,
                                                L // channels, int(channels), target,
                                                torch.cuda.current_stream(x.device).cuda_stream), "dz_adjust_volume")
    return out


def adjust_volume(waveform, volume_in_db: float, device: Optional[torch.device] = None):
    """The ``AdjustVolume`` block's arithmetic over the last axis of ``(..., samples)``, on the GPU: each signal is
    scaled to ``volume_in_db`` dB (``10 log10`` of its mean square) and, where the scaled peak exceeds 1, divided by
    it.  A tensor comes back on its own device, a numpy array as a float32 array.  As in the reference a signal of
    zero energy, or with a NaN / Inf sample, comes out all NaN."""
    target = _target_db(volume_in_db)
    if not isinstance(waveform, torch.Tensor):
        import numpy as np
        x = torch.from_numpy(np.ascontiguousarray(waveform, dtype=np.float32))
        return adjust_volume(x, target, device).numpy()
    if waveform.ndim == 0 or waveform.numel() == 0:
        raise ValueError(f"adjust_volume: empty waveform of shape {tuple(waveform.shape)}")
    src = waveform.device
    dev = _gpu(src if src.type == "cuda" or device is None else torch.device(device))
    lead, L = waveform.shape[:-1], waveform.shape[-1]
    x = waveform.to(dev, torch.float32).reshape(-1, L)
    if x.stride(1) != 1:
        x = x.contiguous()
    y = adjust_volume_rows(x, target).reshape(*lead, L)
    return y if src == dev else y.to(src)


def decode_pcm(raw, input_format: str, channels: int = 1, device: Optional[torch.device] = None) -> torch.Tensor:
    """Interleaved frames of ``channels`` values of ``input_format`` (``diart_amd.pcm``: "f32" | "s16" | "u8" | "s32" |
    "ulaw" | "alaw") -> mono float32 on the GPU, by the push kernel's per-frame function (``dz_pcm_decode``): the bits
    a ``StreamServer`` with that format hands its models.  ``raw``: a numpy array or tensor of the format's dtype, 1-D
    or ``(n, channels)``, or a bytes-like object of little-endian values; whole frames."""
    import numpy as np
    from .pcm import PCM_FORMATS
    if input_format not in PCM_FORMATS:
        raise ValueError(f"decode_pcm: input_format={input_format!r} (expected one of {tuple(PCM_FORMATS)})")
    if not (isinstance(channels, int) and 1 <= channels <= 8):
        raise ValueError(f"decode_pcm: channels={channels!r} (expected 1 .. 8)")
    code, dtype = PCM_FORMATS[input_format]
    tdtype = torch.from_numpy(np.zeros(0, dtype)).dtype
    if isinstance(raw, torch.Tensor):
        x = raw
    elif isinstance(raw, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(raw))
    else:
        view = memoryview(raw).cast("B")
        if len(view) % dtype.itemsize:
            raise ValueError(f"decode_pcm: {len(view)} bytes are not whole {input_format} values")
        x = torch.from_numpy(np.frombuffer(view, dtype=dtype).copy())
    if x.dtype != tdtype:
        raise ValueError(f"decode_pcm: {x.dtype} values for input_format={input_format!r} (expected {dtype.name})")
    if not (x.ndim == 1 or (x.ndim == 2 and x.shape[1] == channels)):
        raise ValueError(f"decode_pcm: values of shape {tuple(x.shape)} (expected 1-D or (n, {channels}))")
    if x.numel() == 0 or x.numel() % channels:
        raise ValueError(f"decode_pcm: {x.numel()} values are not a whole number (>= 1) of {channels}-channel frames")
    dev = _gpu(x.device if x.device.type == "cuda" or device is None else torch.device(device))
    x = x.to(dev).contiguous().reshape(-1)
    frames = x.numel() // channels
    out = torch.empty(frames, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dz_pcm_decode(_lib.context(dev.index), x.data_ptr(), frames, code, int(channels),
                                             out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "dz_pcm_decode")
        # `x` may be a temporary copy: its memory is reused in stream order by the caching allocator
    return out


def overlap_track(scores):
    """The OverlappedSpeechDetection track of ``scores (..., K)``, ``K`` speakers last: per row the second largest
    value counted with multiplicity, NaN ordered above every number, shaped ``(..., 1)``, of the scores' dtype and on
    their device.  The definition is

        torch.sort(scores, dim=-1, descending=True).values[..., 1:2]

    and that statement is what a CPU tensor or a numpy array gets (the array comes back as an array).  A CUDA tensor
    runs ``overlap_track_kernel`` (``dz_overlap_track``) on the current stream: rows packed or at one common stride
    are read in place, anything else is copied first.  The kernel is float32 with 2 <= K <= 8, and nothing is
    converted behind the caller's back: a CUDA tensor of another dtype or with more speakers is a ``ValueError``.
    ``K < 2`` (one speaker has no overlap) and empty scores are a ``ValueError`` on every path."""
    if not isinstance(scores, torch.Tensor):
        import numpy as np
        return overlap_track(torch.from_numpy(np.asarray(scores))).numpy()
    if scores.ndim < 1 or scores.shape[-1] < 2:
        raise ValueError(f"overlap_track: scores of shape {tuple(scores.shape)} (at least 2 speakers on the last axis: "
                         "one speaker has no overlap)")
    if scores.numel() == 0:
        raise ValueError(f"overlap_track: empty scores of shape {tuple(scores.shape)}")
    if not scores.is_cuda:
        return torch.sort(scores, dim=-1, descending=True).values[..., 1:2]
    K = scores.shape[-1]
    if K > 8:
        raise ValueError(f"overlap_track: {K} speakers (the kernel takes 2 .. 8)")
    if scores.dtype != torch.float32:
        raise ValueError(f"overlap_track: {scores.dtype} scores on the GPU (the kernel takes float32)")
    x = scores
    if x.ndim != 2 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < K):
        x = x.reshape(-1, K)
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < K):
            x = x.contiguous()
    rows = x.shape[0]
    out = torch.empty(rows, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dz_overlap_track(x.data_ptr(), x.stride(0) if rows > 1 else K, rows, K, out.data_ptr(),
                                                torch.cuda.current_stream(x.device).cuda_stream), "dz_overlap_track")
    return out.reshape(*scores.shape[:-1], 1)


def gallery_match(embeddings, voiceprints):
    """The nearest voiceprint of every row of ``embeddings (..., D)`` among ``voiceprints (E, D)`` by the clustering's
    cosine distance -> ``(index int32, distance f32, second f32)`` shaped ``(...)``.  The definition is, on float64,

        d = 1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None])
        index = d.argmin(dim=1)          # the lowest index among equal distances

    with ``distance`` that minimum and ``second`` the smallest distance among the other voiceprints (+inf when E == 1);
    a row with a NaN / Inf element or of zero norm gets -1 / NaN / NaN.  A CPU tensor or a numpy array gets exactly that
    statement, rounded to float32 (the array comes back as arrays).  A CUDA tensor runs ``gallery_match`` of
    ``csrc/k_gallery.hip`` (``dz_gallery_match``; float32, D a multiple of 64 from 64 to 512, E <= 65 536) against a
    gallery built from ``voiceprints`` for this call; to match step after step keep a ``gallery.SpeakerGallery``."""
    import numpy as np
    if not isinstance(embeddings, torch.Tensor):
        out = gallery_match(torch.from_numpy(np.asarray(embeddings)), voiceprints)
        return tuple(t.numpy() for t in out)
    g = voiceprints if isinstance(voiceprints, torch.Tensor) else torch.from_numpy(np.asarray(voiceprints))
    if g.ndim != 2 or g.shape[0] < 1 or embeddings.ndim < 1 or embeddings.shape[-1] != g.shape[1] or embeddings.numel() == 0:
        raise ValueError(f"gallery_match: embeddings of shape {tuple(embeddings.shape)} against voiceprints of shape "
                         f"{tuple(g.shape)}")
    if embeddings.is_cuda:
        from .gallery import SpeakerGallery
        names = [f"voiceprint {e}" for e in range(g.shape[0])]
        return SpeakerGallery(names, g, embeddings.device).match(embeddings)
    lead = embeddings.shape[:-1]
    x = embeddings.reshape(-1, g.shape[1]).to(torch.float64)
    g = g.detach().cpu().to(torch.float64)
    norm = x.norm(dim=1, keepdim=True)
    bad = ~torch.isfinite(x).all(dim=1) | (norm[:, 0] == 0) | ~torch.isfinite(norm[:, 0])
    x = torch.where(bad[:, None], torch.ones_like(x), x)
    d = 1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None])
    index = d.argmin(dim=1)
    dist = d.gather(1, index[:, None])[:, 0]
    second = d.scatter(1, index[:, None], float("inf")).min(dim=1).values
    nan = torch.full_like(dist, float("nan"))
    index = torch.where(bad, torch.full_like(index, -1), index).to(torch.int32)
    return (index.reshape(lead), torch.where(bad, nan, dist).to(torch.float32).reshape(lead),
            torch.where(bad, nan, second).to(torch.float32).reshape(lead))


SIGMA_FLOOR = 1e-3      # a guard against dividing by zero (top_n == 1, a degenerate cohort), not a tuned value


def _cohort_stats64(x, c, top_n):
    """x (R, D), c (M, D) float64 -> (mean, std) of the top_n NEAREST cohort members of every row."""
    d = 1 - (x @ c.T) / (x.norm(dim=1, keepdim=True) * c.norm(dim=1)[None])
    near = d.topk(top_n, dim=1, largest=False).values
    return near.mean(dim=1), near.std(dim=1, unbiased=False).clamp_min(SIGMA_FLOOR)


def _cohort_args(embeddings, cohort, top_n, who, voiceprints=None):
    import numpy as np
    c = cohort if isinstance(cohort, torch.Tensor) else torch.from_numpy(np.asarray(cohort))
    g = voiceprints
    if g is not None and not isinstance(g, torch.Tensor):
        g = torch.from_numpy(np.asarray(g))
    D = embeddings.shape[-1] if embeddings.ndim >= 1 else -1
    if (c.ndim != 2 or c.shape[0] < 1 or c.shape[1] != D or embeddings.numel() == 0
            or (g is not None and (g.ndim != 2 or g.shape[0] < 1 or g.shape[1] != D))):
        raise ValueError(f"{who}: embeddings of shape {tuple(embeddings.shape)} against "
                         + (f"voiceprints of shape {tuple(g.shape)} and " if g is not None else "")
                         + f"a cohort of shape {tuple(c.shape)}")
    if int(top_n) != top_n or not 1 <= int(top_n) <= c.shape[0]:
        raise ValueError(f"{who}: top_n={top_n!r} (1 .. the cohort's {c.shape[0]} rows)")
    return c, g, int(top_n)


def _unusable(x):
    """x (R, D) float64 -> (bad (R,), x with the unusable rows replaced by ones): the gallery's rule."""
    norm = x.norm(dim=1)
    bad = ~torch.isfinite(x).all(dim=1) | (norm == 0) | ~torch.isfinite(norm)
    return bad, torch.where(bad[:, None], torch.ones_like(x), x)


def cohort_stats(embeddings, cohort, top_n):
    """Mean and population standard deviation of the cosine distances of every row of ``embeddings (..., D)`` to its
    ``top_n`` NEAREST rows of ``cohort (M, D)`` -> ``(mean f32, std f32)`` shaped ``(...)``.  On float64:

        d = 1 - (x @ c.T) / (x.norm(dim=1, keepdim=True) * c.norm(dim=1)[None])
        near = d.topk(top_n, dim=1, largest=False).values
        mean, std = near.mean(dim=1), near.std(dim=1, unbiased=False).clamp_min(1e-3)

    (the floor guards a division, it is no tuned value); a row with a NaN / Inf element or of zero norm gets NaN.  A CPU
    tensor or a numpy array gets exactly that statement, rounded to float32.  A CUDA tensor runs the kernels of
    ``csrc/k_cohort.hip`` (``dz_gallery_cohort_stats``; M <= 8 192) on a gallery built for this call."""
    import numpy as np
    if not isinstance(embeddings, torch.Tensor):
        return tuple(t.numpy() for t in cohort_stats(torch.from_numpy(np.asarray(embeddings)), cohort, top_n))
    c, _, top_n = _cohort_args(embeddings, cohort, top_n, "cohort_stats")
    if embeddings.is_cuda:
        from .gallery import SpeakerGallery
        c = c.detach().cpu()
        return SpeakerGallery(["voiceprint 0"], c[:1], embeddings.device, cohort=c, top_n=top_n).cohort_stats(embeddings)
    lead = embeddings.shape[:-1]
    bad, x = _unusable(embeddings.reshape(-1, c.shape[1]).to(torch.float64))
    mean, std = _cohort_stats64(x, c.detach().cpu().to(torch.float64), top_n)
    nan = torch.full_like(mean, float("nan"))
    return (torch.where(bad, nan, mean).to(torch.float32).reshape(lead),
            torch.where(bad, nan, std).to(torch.float32).reshape(lead))


def gallery_match_normalised(embeddings, voiceprints, cohort, top_n=300):
    """``gallery_match`` by the distance normalised against a cohort of impostors (adaptive s-norm) ->
    ``(index int32, distance f32, second f32)`` shaped ``(...)``.  On float64, with ``cohort_stats`` as above,

        mu_x, sd_x = cohort_stats(x, c, top_n)              # per embedding row
        mu_g, sd_g = cohort_stats(g, c, top_n)              # per voiceprint
        d  = 1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None])
        dn = 0.5 * ((d - mu_g[None]) / sd_g[None] + (d - mu_x[:, None]) / sd_x[:, None])
        index = dn.argmin(dim=1)                            # the lowest index among equal values

    ``dn`` is minus the AS-norm score of the similarity ``1 - d``: signed, lower is closer; a true match is typically
    several units below zero, an impostor near or above zero.  ``distance`` is ``dn`` at ``index``, ``second`` the
    smallest ``dn`` among the other voiceprints (+inf when E == 1); an unusable row gets -1 / NaN / NaN.  ``top_n``
    = 300 is the value of the published recipes, not measured here.  A CPU tensor or a numpy array gets exactly that
    statement, rounded to float32; a CUDA tensor runs ``dz_gallery_match_norm`` (``csrc/k_cohort.hip``) on a gallery
    built for this call; to match step after step keep a ``gallery.SpeakerGallery`` with a cohort."""
    import numpy as np
    if not isinstance(embeddings, torch.Tensor):
        out = gallery_match_normalised(torch.from_numpy(np.asarray(embeddings)), voiceprints, cohort, top_n)
        return tuple(t.numpy() for t in out)
    c, g, top_n = _cohort_args(embeddings, cohort, top_n, "gallery_match_normalised", voiceprints)
    if embeddings.is_cuda:
        from .gallery import SpeakerGallery
        names = [f"voiceprint {e}" for e in range(g.shape[0])]
        return SpeakerGallery(names, g, embeddings.device, cohort=c.detach().cpu(), top_n=top_n).match_normalised(embeddings)
    lead = embeddings.shape[:-1]
    bad, x = _unusable(embeddings.reshape(-1, g.shape[1]).to(torch.float64))
    g, c = g.detach().cpu().to(torch.float64), c.detach().cpu().to(torch.float64)
    mu_x, sd_x = _cohort_stats64(x, c, top_n)
    mu_g, sd_g = _cohort_stats64(g, c, top_n)
    d = 1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None])
    dn = 0.5 * ((d - mu_g[None]) / sd_g[None] + (d - mu_x[:, None]) / sd_x[:, None])
    index = dn.argmin(dim=1)
    dist = dn.gather(1, index[:, None])[:, 0]
    second = dn.scatter(1, index[:, None], float("inf")).min(dim=1).values
    nan = torch.full_like(dist, float("nan"))
    index = torch.where(bad, torch.full_like(index, -1), index).to(torch.int32)
    return (index.reshape(lead), torch.where(bad, nan, dist).to(torch.float32).reshape(lead),
            torch.where(bad, nan, second).to(torch.float32).reshape(lead))


def min_duration(annotation, min_duration_on: float = 0.0, min_duration_off: float = 0.0, patch_collar: float = 0.05):
    """The minimum durations of ``VoiceActivityDetection`` and ``OverlappedSpeechDetection`` on a file's accumulated
    turns, per label: the gaps are filled first — ``annotation.support(max(patch_collar, min_duration_off))``, which is
    ``support(patch_collar)`` followed by ``support(min_duration_off)`` — then every merged turn with
    ``end - start < min_duration_on`` (strictly) is dropped.  A turn that will be dropped still bridges gaps.  This is
    ``PredictionAccumulator``'s stitching followed by the tail of pyannote's ``Binarize``.  ``annotation``: the project's
    ``Annotation`` or pyannote's; a new one of the same class comes back.  Both durations 0:
    ``annotation.support(patch_collar)``.  It needs the whole file: a live step has no look-ahead, and no engine calls it."""
    from .blocks.base import check_min_duration
    on = check_min_duration(min_duration_on, "min_duration_on", "min_duration")
    off = check_min_duration(min_duration_off, "min_duration_off", "min_duration")
    merged = annotation.support(max(float(patch_collar), off))
    if on == 0.0:
        return merged
    out = type(merged)(uri=merged.uri, modality=merged.modality)
    for segment, track, label in merged.itertracks(yield_label=True):
        if not (segment.end - segment.start < on):
            out[segment, track] = label
    return out


# ---------------------------------------------------------------------------------------------- whole-file clustering
LINKAGE_MAX_DIM = 1024               # AG_DMAX (csrc/agglo_core.h)
LINKAGE_MAX_FILES = 1024             # files of one dz_agglo_linkage call
LINKAGE_MEMORY_BUDGET = 4 << 30      # bytes of distance matrices (8 N^2 per file) one call may hold: N <= 23 170
# backend=None on a machine with a GPU: a file of fewer rows runs on the host.  Measured (profiles/r36a_offline.json, D =
# 256): one core takes 1.5 ms at N = 256 and 6.0 ms at 512, the GPU call 2.6 ms and 5.3 ms (about 10 us per merge, a
# dependent chain inside one workgroup): the host wins up to 256 rows, the GPU from 512 on.
LINKAGE_GPU_MIN_ROWS = 512


def _linkage_groups(counts, memory_budget: int):
    """Files whose float64 distance matrices fit the budget together share a call, in order; a file that does not fit
    it alone is refused by name."""
    groups, cur, used = [], [], 0
    for i, n in enumerate(counts):
        need = 8 * int(n) * int(n)
        if need > memory_budget:
            raise ValueError(f"file {i}: the distance matrix of {n} rows takes {need} bytes, above memory_budget = "
                             f"{memory_budget}; whole-file clustering needs 8 N^2 bytes per file")
        if cur and (used + need > memory_budget or len(cur) == LINKAGE_MAX_FILES):
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += need
    if cur:
        groups.append(cur)
    return groups


def linkage_unit_rows(rows, backend: Optional[str] = None, device: Optional[torch.device] = None,
                      memory_budget: int = LINKAGE_MEMORY_BUDGET, num_threads: int = 8):
    """Centroid linkage of every file of ``rows`` — ``(N_f, D)`` float64 arrays (or CUDA tensors) of finite unit rows,
    which the caller has checked — as a list of ``(max(N_f - 1, 0), 4)`` float64 arrays in scipy's ``linkage`` layout.
    ``backend="gpu"``: ``dz_agglo_linkage`` (``csrc/k_agglo.hip``); ``"core"``: the same text on host threads
    (``dz_agglo_linkage_host``); ``None``: on a machine with a GPU the files of at least ``LINKAGE_GPU_MIN_ROWS`` rows on
    the GPU and the smaller ones on the host (the two give the same ``Z`` bit for bit), else the host."""
    import numpy as np
    if backend not in ("gpu", "core", None):
        raise ValueError(f"backend must be 'gpu', 'core' or None, got {backend!r}")
    if not rows:
        return []
    dims = {int(x.shape[1]) for x in rows}
    if len(dims) != 1:
        raise ValueError(f"the files of one call share their dimension, got {sorted(dims)}")
    D = dims.pop()
    if not 1 <= D <= LINKAGE_MAX_DIM:
        raise ValueError(f"dimension {D} outside [1, {LINKAGE_MAX_DIM}]")
    counts = [int(x.shape[0]) for x in rows]
    groups = _linkage_groups(counts, int(memory_budget))          # refusals come before the GPU is touched
    if backend is None and torch.cuda.is_available():
        out = [None] * len(rows)
        for where, part in (("gpu", [i for i, n in enumerate(counts) if n >= LINKAGE_GPU_MIN_ROWS]),
                            ("core", [i for i, n in enumerate(counts) if n < LINKAGE_GPU_MIN_ROWS])):
            for i, Z in zip(part, linkage_unit_rows([rows[i] for i in part], where, device, memory_budget, num_threads)):
                out[i] = Z
        return out
    backend = backend or "core"
    lib = _lib.load()
    out = [None] * len(rows)
    dev = _gpu(device) if backend == "gpu" else None
    for group in groups:
        off = np.concatenate([[0], np.cumsum([counts[i] for i in group])]).astype(np.int32)
        nz = int(sum(max(counts[i] - 1, 0) for i in group))
        if backend == "gpu":
            x = torch.cat([(rows[i] if isinstance(rows[i], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows[i])))
                           .to(dev, torch.float64) for i in group]).contiguous()
            Z = torch.zeros((max(nz, 1), 4), dtype=torch.float64, device=dev)
            status = torch.zeros(len(group), dtype=torch.int32, device=dev)
            need = lib.dz_agglo_work_bytes(len(group), off.ctypes.data)
            if need < 0:
                _lib.check(2, "dz_agglo_work_bytes")
            work = torch.empty(int(need), dtype=torch.uint8, device=dev)
            _lib.check(lib.dz_agglo_linkage(_lib.context(dev.index), len(group), off.ctypes.data, x.data_ptr(), D,
                                            Z.data_ptr(), status.data_ptr(), work.data_ptr(), int(need),
                                            torch.cuda.current_stream(dev).cuda_stream), "dz_agglo_linkage")
            Zh, st = Z.cpu().numpy(), status.cpu().numpy()        # the one synchronising copy of the call
            del work
        else:
            x = np.ascontiguousarray(np.concatenate([np.asarray(rows[i].cpu() if isinstance(rows[i], torch.Tensor) else rows[i],
                                                                dtype=np.float64).reshape(counts[i], D) for i in group]))
            Zh, st = np.zeros((max(nz, 1), 4), dtype=np.float64), np.zeros(len(group), dtype=np.int32)
            _lib.check(lib.dz_agglo_linkage_host(len(group), off.ctypes.data, x.ctypes.data, D, Zh.ctypes.data,
                                                 st.ctypes.data, int(num_threads)), "dz_agglo_linkage_host")
        if (st != -1).any():
            bad = int(np.flatnonzero(st != -1)[0])
            raise _lib.DiartAmdError(f"linkage of file {group[bad]} stopped at merge {int(st[bad])}: an index failed its "
                                     "range check (rows that are not finite?)")
        z0 = 0
        for i in group:
            m = max(counts[i] - 1, 0)
            out[i] = Zh[z0:z0 + m].copy()
            z0 += m
    return out


def linkage_centroid(x, memory_budget: int = LINKAGE_MEMORY_BUDGET, num_threads: int = 8):
    """``scipy.cluster.hierarchy.linkage(x / |x|, "centroid")`` in float64: the dendrogram ``Z`` ``(N - 1, 4)`` of the
    rows of ``x`` ``(N, D)``, each scaled to unit length — ``(smaller id, larger id, height, size)`` per merge, the
    merge at step t getting id ``N + t``.  A CUDA tensor runs the HIP kernels (``csrc/k_agglo.hip``); a CPU tensor or a
    numpy array runs the same text on the host.  A list of such arrays is clustered in one call and returns a list.
    ``N`` = 0 or 1 gives an empty ``Z``.  Refused: a non-finite or zero row, ``D`` above 1 024, a matrix (``8 N^2``
    bytes) above ``memory_budget``."""
    import numpy as np
    many = isinstance(x, (list, tuple))
    xs = list(x) if many else [x]
    gpu = [isinstance(a, torch.Tensor) and a.is_cuda for a in xs]
    if any(gpu) and not all(gpu):
        raise ValueError("the files of one call live on one side: all CUDA tensors, or all host arrays")
    unit = []
    for i, a in enumerate(xs):
        if a.ndim != 2:
            raise ValueError(f"file {i}: rows (N, D) expected, got shape {tuple(a.shape)}")
        if a.shape[1] > LINKAGE_MAX_DIM or a.shape[1] < 1:
            raise ValueError(f"file {i}: dimension {a.shape[1]} outside [1, {LINKAGE_MAX_DIM}]")
        if isinstance(a, torch.Tensor) and a.is_cuda:
            a = a.to(torch.float64)
            norm = a.norm(dim=1, keepdim=True)
            ok = bool((torch.isfinite(a).all() & torch.isfinite(norm).all() & (norm > 0).all()).item())
        else:
            a = np.asarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                norm = np.sqrt((a * a).sum(axis=1, keepdims=True))
            ok = bool(np.isfinite(a).all() and np.isfinite(norm).all() and (norm > 0).all())
        if not ok:
            raise ValueError(f"file {i}: a row is not finite or has zero norm; linkage_centroid takes rows it can scale to "
                             "unit length")
        unit.append(a / norm if a.shape[0] else a)
    Z = linkage_unit_rows(unit, "gpu" if any(gpu) else "core", xs[0].device if any(gpu) else None, memory_budget,
                          num_threads)
    return Z if many else Z[0]


def cut_linkage(Z, threshold: float, min_cluster_size: int = 1, max_speakers: Optional[int] = None, n: Optional[int] = None):
    """``fcluster(Z, threshold, "distance")`` followed by the whole-file mode's choice of clusters: a flat cluster is a
    maximal subtree whose merge heights are all ``<= threshold``; kept are those with at least ``min_cluster_size``
    leaves, at most ``max_speakers`` of them by size (ties: the one whose first leaf comes first), the largest one when
    none qualifies, numbered ``0 .. G - 1`` by their first leaf.  Returns ``(labels, G)``: per leaf its kept cluster
    or -1.  ``n``: the leaves, ``len(Z) + 1`` unless given (an empty ``Z`` stands for one leaf, or for none)."""
    import math
    import numpy as np
    if not math.isfinite(float(threshold)):
        raise ValueError(f"threshold must be finite, got {threshold}")
    if int(min_cluster_size) < 1:
        raise ValueError(f"min_cluster_size must be at least 1, got {min_cluster_size}")
    if max_speakers is not None and int(max_speakers) < 1:
        raise ValueError(f"max_speakers must be at least 1, got {max_speakers}")
    Z = np.ascontiguousarray(Z, dtype=np.float64).reshape(-1, 4)
    n = Z.shape[0] + 1 if n is None else int(n)
    if n != Z.shape[0] + 1 and not (n == 0 and Z.shape[0] == 0):
        raise ValueError(f"{Z.shape[0]} merges are no dendrogram over {n} leaves")
    labels, G = np.full(max(n, 1), -1, dtype=np.int32), _lib.C.c_int(0)
    _lib.check(_lib.load().dz_agglo_cut(Z.ctypes.data, n, float(threshold), int(min_cluster_size),
                                        2 ** 31 - 1 if max_speakers is None else int(max_speakers), labels.ctypes.data,
                                        _lib.C.byref(G)), "dz_agglo_cut")
    return labels[:n], int(G.value)
