"""Operator API of the hot path: ``SegmentationModel`` / ``EmbeddingModel``.

Mirrors the duck-typed boundary of the reference (``/root/reference/src/diart/models.py``:
``LazyModel`` :112-139, ``SegmentationModel`` :142-198, ``EmbeddingModel`` :201-265 and the
"Custom models" contract of ``/root/reference/README.md:186-209``): a model wraps a *loader*
(``Callable[[], Callable]``); the loaded object answers ``__call__``, ``.to(device)`` and is
only ``.eval()``-ed when it is an ``nn.Module``.  Here the loaded objects are
``HipSegmentation`` / ``HipEmbedding``: thin handles on ``libdiart_amd.so`` — every FLOP of
the forward pass runs in hand-written HIP kernels, torch only owns the memory.

Because the callables follow the reference contract they can also be handed to the
reference's own classes unchanged::

    from diart.models import SegmentationModel            # the reference
    from diart_amd.models import SegmentationLoader
    seg = SegmentationModel(SegmentationLoader("seg_state.pt"))

Loaders are picklable and hold no HIP state until ``__call__`` (``Parallelize`` pickles the
config that holds them, ``/root/reference/src/diart/inference.py:527-555``).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Callable, Dict, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .weights import (ECAPA_MEL_FEATURES, ECAPA_MEL_MIN_NUM_SAMPLES, PackedEcapa, PackedEcapaMel, PackedEmbedding, PackedSbResNet, PackedSbXvector, PackedSegmentation, PackedTitaNet, PackedWeSpeaker,
                      SB_RESNET_MARKERS, SB_RESNET_MIN_NUM_SAMPLES, SB_RESNET_STRIDES, TITANET_MARKERS,
                      TITANET_MIN_NUM_SAMPLES)

StateSource = Union[str, Path, Dict[str, torch.Tensor]]


def default_precision(given: Optional[str] = None) -> str:
    """Arithmetic of the GEMM-shaped layers: the ``precision=`` argument of a model, "f16x3" when it does not say
    (f32 operands split into two f16 numbers = 22 mantissa bits, three f16 MFMAs per product, f32
    accumulation: measured against the f32 CPU restatement of the networks it is indistinguishable
    from "f32", the exact-f32 MFMA path, and 1.8x faster end to end; weights.PRECISIONS,
    DESIGN.md 4.2); ``DZ_ENGINE=precision=...`` overrides both (config.py)."""
    from .config import setting
    from .weights import PRECISIONS
    p = setting("precision", given, "f16x3")
    if p not in PRECISIONS:
        raise ValueError(f"precision={p!r}: expected one of {PRECISIONS}")
    return p


REPEATED_ROWS = ("each", "share")


def repeated_rows_mode(given: Optional[str] = None, shares: bool = True, who: str = "") -> str:
    """What a model does with the K copies of every waveform in the reference's ``(batch spk)`` call
    (blocks/embedding.py:56-59): "each" (the default) runs the network on every row, "share" asks the device how often
    the rows repeat (``dz_rows_repeat``) and runs everything before the pooling once per distinct window.
    ``DZ_ENGINE=repeated_rows=...`` overrides the argument of the models that can share (config.py).  ``shares=False``:
    a model whose rows are different inputs refuses "share" and ignores the override."""
    if shares:
        from .config import setting
        given = setting("repeated_rows", given, "each")
    mode = "each" if given is None else given
    if mode not in REPEATED_ROWS:
        raise ValueError(f"repeated_rows={mode!r}: expected one of {REPEATED_ROWS}")
    if mode == "share" and not shares:
        raise ValueError(f"repeated_rows='share': {who} has no trunk to share — its masks select the SAMPLES each row "
                         "keeps, so the K rows of a chunk are K different inputs from the first layer on "
                         "(use forward_groups, or repeated_rows='each')")
    return mode


def _read_state(src: StateSource) -> Dict[str, torch.Tensor]:
    """A state dict, or a file holding one: ``.safetensors``, a plain ``torch.save`` of a state dict (speechbrain's
    ``embedding_model.ckpt``) or a PyTorch-Lightning checkpoint (``pyannote/segmentation``, ``pyannote/embedding``:
    what the reference loads through pyannote.audio, /root/reference/src/diart/models.py:50, :59).  Files are read
    by ``checkpoint.read_state``: tensors only, no foreign class is imported and no pickle code runs."""
    if isinstance(src, dict):
        return src
    from .checkpoint import read_state
    return read_state(src)


def _device_index(device: torch.device) -> int:
    if device.type != "cuda":
        raise _lib.DiartAmdError(
            f"diart_amd runs on MI355X only (requested device '{device}'); there is no CPU path")
    return device.index if device.index is not None else torch.cuda.current_device()


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _as_rows(waveform: torch.Tensor) -> torch.Tensor:
    """(B,1,S) or (B,S) float32 device tensor with 16-byte aligned rows; never copies a view
    that is already usable (so a rolling window is addressed in place)."""
    if waveform.ndim == 3:
        if waveform.shape[1] != 1:
            raise ValueError(f"expected mono audio (batch, 1, samples), got {tuple(waveform.shape)}")
        waveform = waveform[:, 0, :]
    if waveform.ndim != 2:
        raise ValueError(f"expected (batch, channels, samples), got {tuple(waveform.shape)}")
    if waveform.dtype != torch.float32:
        waveform = waveform.float()
    ok = (waveform.stride(1) == 1 and waveform.data_ptr() % 16 == 0
          and (waveform.shape[0] == 1 or waveform.stride(0) % 4 == 0))
    return waveform if ok else waveform.contiguous()


class _HipModule:
    """Common handle management: packed weights per device, one C handle per (S, max_batch)."""

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int):
        self._state = state
        self._max_batch = int(max_batch)
        self.device: Optional[torch.device] = None
        self._packed = None
        self._handles: Dict[int, tuple] = {}

    def to(self, device: Union[torch.device, str]):
        device = torch.device(device)
        idx = _device_index(device)
        device = torch.device("cuda", idx)
        if self.device != device:
            self._release()
            self.device = device
            self._packed = self._pack(device)
        return self

    def _need(self, num_samples: int, batch: int):
        if self.device is None:
            self.to(torch.device("cuda"))
        h = self._handles.get(num_samples)
        if h is None or h[1] < batch:
            if h is not None:
                self._destroy(h[0])
            cap = max(self._max_batch, batch)
            h = (self._create(num_samples, cap), cap)
            self._handles[num_samples] = h
        return h[0]

    repeated_rows = "each"
    last_shared: Optional[tuple] = None
    MAX_MULTI = 8               # speakers per window of dz_emb_forward_multi / dz_wsp_forward_multi (kMaxSpk, MAXK)

    def _shared_call(self, rows: torch.Tensor, weights: torch.Tensor) -> Optional[torch.Tensor]:
        """``repeated_rows="share"``: ``__call__``'s rows (N,S) and weights (N,F) through ``forward_multi`` when every
        window is there R >= 2 times in a row — B = N / R windows addressed in place (row stride x R), weights viewed as
        (B,R,F) -> (N,D); None when nothing repeats.  ``dz_rows_repeat`` waits for the current stream once (four bytes
        come back).  The detected repetition may exceed the caller's speaker count when neighbouring windows are
        bit-identical (silence): identical waveforms have identical trunks.  ``forward_multi`` pools at most
        ``MAX_MULTI`` rows per window, and every divisor of a repetition is a repetition too, so R is the largest
        divisor of what the device found that fits (9 -> 3, 96 -> 8; a prime above the limit -> 1: nothing is shared).
        ``last_shared`` = the (B, R) that ran, or None."""
        N, S = rows.shape
        r = C.c_int(0)
        _lib.check(_lib.load().dz_rows_repeat(_lib.context(self.device.index), rows.data_ptr(), rows.stride(0), N, S,
                                              _stream_ptr(self.device), C.byref(r)), "dz_rows_repeat")
        R = max(d for d in range(1, self.MAX_MULTI + 1) if r.value % d == 0)
        if R < 2:
            return None
        B = N // R
        out = self.forward_multi(rows[::R, None, :], weights.view(B, R, weights.shape[1]))
        self.last_shared = (B, R)
        return out.view(N, self.dimension)

    def _release(self):
        for h, _ in self._handles.values():
            self._destroy(h)
        self._handles = {}
        self._packed = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # pickling ships the (CPU) state dict only
    def __getstate__(self):
        return {"_state": {k: v.cpu() for k, v in self._state.items()},
                "_max_batch": self._max_batch, "extra": self._extra_state()}

    def __setstate__(self, st):
        self.__init__(st["_state"], st["_max_batch"], **st["extra"])


class HipSegmentation(_HipModule):
    """pyannote/segmentation forward: ``waveform (B,1,S) -> (B,F,K)`` activations in [0,1]
    (hard {0,1} multilabel when ``powerset``) — the callable behind
    ``SegmentationModel.__call__`` (reference models.py:188-198)."""

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 64, powerset: bool = False,
                 precision: Optional[str] = None, recurrence: Optional[str] = None):
        """``recurrence``: the LSTM recurrence kernel of this model's own calls — "valu" (default: one chain per CU on
        the f32 vector units, the shortest layer) or a matrix-core variant "0" | "3" | "4" (16 chains per workgroup,
        default precision only).  A throughput engine (``StreamBatch``) chooses its own (``struct_throughput``)."""
        super().__init__(state, max_batch)
        from .config import setting
        self.powerset = bool(powerset)
        self.precision = default_precision(precision)
        self.recurrence = str(setting("recurrence", recurrence, "valu"))
        self.num_speakers: Optional[int] = None

    def _extra_state(self):
        return {"powerset": self.powerset, "precision": self.precision, "recurrence": self.recurrence}

    def _pack(self, device):
        p = PackedSegmentation(self._state, device, powerset=self.powerset, precision=self.precision,
                               recurrence=self.recurrence)
        self.num_speakers = p.num_speakers
        return p

    def _create(self, num_samples, cap, throughput: bool = False, recurrence: Optional[str] = None):
        """``throughput``: the handle of an engine that keeps several steps in flight (``StreamBatch``): the matrix-core
        recurrence (``PackedSegmentation.struct_throughput``) instead of the low-latency one; ``recurrence``: that
        kernel, whatever the model's own (``PackedSegmentation.struct_for``)."""
        h = _lib.vp()
        lib = _lib.load()
        w = (self._packed.struct_for(recurrence) if recurrence is not None else
             self._packed.struct_throughput if throughput else self._packed.struct)
        _lib.check(lib.dz_seg_create(_lib.context(self.device.index), C.byref(w),
                                     cap, num_samples, C.byref(h)), "dz_seg_create")
        return h

    def throughput_recurrence(self) -> str:
        """What a throughput handle of this model runs its recurrence on: "valu" | "0" | "3" | "4" (bench.py names the kernel)."""
        p = self._packed
        return str(int(p.struct_throughput.lstm_variant)) if p.struct_throughput.whh_split[0] else "valu"

    def _destroy(self, h):
        _lib.load().dz_seg_destroy(h)

    def num_frames(self, num_samples: int) -> int:
        return int(_lib.load().dz_seg_frames_for(int(num_samples)))

    def __call__(self, waveform: torch.Tensor) -> torch.Tensor:
        if self.device is None:
            self.to(waveform.device)
        if waveform.device != self.device:
            waveform = waveform.to(self.device)
        rows = _as_rows(waveform)
        B, S = rows.shape
        if B < 1:
            raise ValueError("empty batch")
        handle = self._need(S, B)
        out = torch.empty((B, self.num_frames(S), self.num_speakers), dtype=torch.float32,
                          device=self.device)
        _lib.check(_lib.load().dz_seg_forward(handle, rows.data_ptr(), rows.stride(0) if B > 1 else S,
                                              B, out.data_ptr(), _stream_ptr(self.device)),
                   "dz_seg_forward")
        return out

    def forward_vad(self, waveform: torch.Tensor, return_scores: bool = False):
        """VoiceActivityDetection's hot path (reference blocks/vad.py:146-148): ``waveform (B,1,S) -> (B,F,1)``, the
        max over speakers of ``__call__``'s scores (NaN where a row is NaN), computed by the kernel that writes the
        scores (``dz_seg_forward_vad``).  ``return_scores``: ``(track, scores (B,F,K))``.  Enqueued on the current
        stream; does not synchronise."""
        if self.device is None:
            self.to(waveform.device)
        if waveform.device != self.device:
            waveform = waveform.to(self.device)
        rows = _as_rows(waveform)
        B, S = rows.shape
        if B < 1:
            raise ValueError("empty batch")
        handle = self._need(S, B)
        F = self.num_frames(S)
        scores = torch.empty((B, F, self.num_speakers), dtype=torch.float32, device=self.device)
        track = torch.empty((B, F, 1), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().dz_seg_forward_vad(handle, rows.data_ptr(), rows.stride(0) if B > 1 else S, B,
                                                  scores.data_ptr(), track.data_ptr(), _stream_ptr(self.device)),
                   "dz_seg_forward_vad")
        return (track, scores) if return_scores else track

    def forward_overlap(self, waveform: torch.Tensor, return_scores: bool = False):
        """OverlappedSpeechDetection's hot path: ``waveform (B,1,S) -> (B,F,1)``, per frame the second largest of
        ``__call__``'s scores counted with multiplicity, NaN ordered above every number (``torch.sort(scores, -1,
        descending=True).values[..., 1:2]``), computed by the kernel that writes the scores (``dz_seg_forward_track``
        with ``DZ_TRACK_OVERLAP``).  ``return_scores``: ``(track, scores (B,F,K))``.  A model with one speaker has no
        overlap: ``ValueError``.  Enqueued on the current stream; does not synchronise."""
        if self.device is None:
            self.to(waveform.device)
        if self.num_speakers < 2:                # (known once the weights are packed)
            raise ValueError(f"forward_overlap: a model with {self.num_speakers} speaker has no overlap track "
                             "(at least 2 speakers)")
        if waveform.device != self.device:
            waveform = waveform.to(self.device)
        rows = _as_rows(waveform)
        B, S = rows.shape
        if B < 1:
            raise ValueError("empty batch")
        handle = self._need(S, B)
        F = self.num_frames(S)
        scores = torch.empty((B, F, self.num_speakers), dtype=torch.float32, device=self.device)
        track = torch.empty((B, F, 1), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().dz_seg_forward_track(handle, rows.data_ptr(), rows.stride(0) if B > 1 else S, B,
                                                    scores.data_ptr(), track.data_ptr(), _lib.TRACK_OVERLAP,
                                                    _stream_ptr(self.device)), "dz_seg_forward_track")
        return (track, scores) if return_scores else track


class _HipSpeakerEmbedding(_HipModule):
    """The plumbing of every speaker-embedding handle: one C prefix (``_c``: ``dz_emb``, ``dz_ecapa``, ``dz_sbx``,
    ``dz_ttn``, ``dz_wsp``) names their create / destroy / forward / peek functions; ``(waveform (N,1,S), masks or
    weights (N,F) | None) -> (N,dimension)``."""

    dimension: int
    _c: str                     # the C prefix
    _packer: type               # weights.Packed*
    _frames_arg = "masks"       # what the (N, F) matrix is called (error messages)
    _int32_peeks = frozenset()  # peek buffers that hold int32

    _shares = False             # does ``repeated_rows="share"`` apply (is there a speaker-independent trunk)?

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None):
        super().__init__(state, max_batch)
        self.precision = default_precision(precision)
        self.repeated_rows = repeated_rows_mode(repeated_rows, self._shares, type(self).__name__)

    def _extra_state(self):
        return {"precision": self.precision, "repeated_rows": self.repeated_rows}

    def _pack(self, device):
        return self._packer(self._state, device, precision=self.precision)

    def _fn(self, name: str):
        return getattr(_lib.load(), f"{self._c}_{name}")

    def _create(self, num_samples, cap):
        h = _lib.vp()
        _lib.check(self._fn("create")(_lib.context(self.device.index), C.byref(self._packed.struct), cap, num_samples,
                                      C.byref(h)), f"{self._c}_create")
        return h

    def _destroy(self, h):
        self._fn("destroy")(h)

    def __call__(self, waveform: torch.Tensor, masks_or_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.device is None:
            self.to(waveform.device)
        rows = _as_rows(waveform.to(self.device))
        N, S = rows.shape
        mptr, fw = None, 0
        if masks_or_weights is not None:
            m = masks_or_weights.to(self.device, torch.float32).contiguous()
            if m.ndim != 2 or m.shape[0] != N:
                raise ValueError(f"{self._frames_arg} must be (batch, frames), got {tuple(m.shape)}")
            mptr, fw = m.data_ptr(), m.shape[1]
        self.last_shared = None
        if self.repeated_rows == "share" and masks_or_weights is not None and N >= 2:
            shared = self._shared_call(rows, m)
            if shared is not None:
                return shared
        handle = self._need(S, N)
        out = torch.empty((N, self.dimension), dtype=torch.float32, device=self.device)
        _lib.check(self._fn("forward")(handle, rows.data_ptr(), rows.stride(0) if N > 1 else S, mptr, N, fw,
                                       out.data_ptr(), _stream_ptr(self.device)), f"{self._c}_forward")
        return out

    def _peek_raw(self, handle, which: int):
        if not hasattr(_lib.load(), f"{self._c}_peek"):
            raise NotImplementedError(f"{type(self).__name__}: {self._c} handles expose no intermediate buffers (no "
                                      f"{self._c}_peek)")
        ptr, cnt, frames = _lib.vp(), C.c_longlong(), C.c_int()
        _lib.check(self._fn("peek")(handle, which, C.byref(ptr), C.byref(cnt), C.byref(frames)), f"{self._c}_peek")
        return ptr, cnt.value, frames.value

    def peek(self, num_samples: int, which: int):
        """Intermediate of the last forward (parity tests; synchronises): ``(flat tensor, frames)``, see ``<_c>_peek``."""
        return self.peek_handle(self._handles[num_samples][0], which)

    def peek_handle(self, handle, which: int):
        """``peek`` of a handle this model created for someone else (``StreamBatch``'s per-lane handles)."""
        ptr, cnt, frames = self._peek_raw(handle, which)
        out = torch.empty(cnt, dtype=torch.int32 if which in self._int32_peeks else torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.memcpy(out.data_ptr(), ptr, cnt * 4)
        return out, frames


class _HipTrunkEmbedding(_HipSpeakerEmbedding):
    """The pyannote x-vector and WeSpeaker: the (N, F) matrix is pooling weights, so everything before the pooling is
    speaker-independent; ``blocks.SpeakerEmbedding`` takes ``forward_multi`` where a model has it."""

    _frames_arg, _shares = "weights", True

    def forward_multi(self, waveform: torch.Tensor, weights: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """``waveform (B,1,S)``, ``weights (B,K,F)`` speaker-major -> ``(B,K,dimension)`` the reference's ``(B*K)``-row call (blocks/embedding.py:56-65) with
        everything before the pooling computed once per window instead of K times.  No synchronisation."""
        if self.device is None:
            self.to(waveform.device)
        rows = _as_rows(waveform.to(self.device))
        B, S = rows.shape
        weights = weights.to(self.device, torch.float32).contiguous()
        if weights.ndim != 3 or weights.shape[0] != B:
            raise ValueError(f"weights must be (batch, speakers, frames), got {tuple(weights.shape)}")
        K, fw = weights.shape[1], weights.shape[2]
        handle = self._need(S, B)
        out = torch.empty((B, K, self.dimension), dtype=torch.float32, device=self.device)
        _lib.check(self._fn("forward_multi")(handle, rows.data_ptr(), rows.stride(0) if B > 1 else S, weights.data_ptr(),
                                             B, K, fw, 1 if normalize else 0, out.data_ptr(), _stream_ptr(self.device)),
                   f"{self._c}_forward_multi")
        return out


class HipEmbedding(_HipTrunkEmbedding):
    """pyannote/embedding forward: ``(waveform (N,1,S), weights (N,F) | None) -> (N,512)`` — the
    callable behind ``EmbeddingModel.__call__`` (reference models.py:248-265)."""

    dimension = 512
    _c = "dz_emb"

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 64, precision: Optional[str] = None,
                 weight_interp: Optional[str] = None, repeated_rows: Optional[str] = None):
        """``weight_interp``: StatsPool's resampling of the pooling weights to the feature frames — "linear"
        (pyannote.audio 2.x .. 3.0: ``F.interpolate(mode="linear")``; the default, setup.cfg pins ``>=2.1.1``) or
        "nearest" (pyannote.audio >= 3.1).  ``EmbeddingLoader`` sets it from the version a checkpoint records.
        ``repeated_rows``: "each" | "share" (``repeated_rows_mode``)."""
        super().__init__(state, max_batch, precision, repeated_rows)
        self.weight_interp = weight_interp or "linear"

    def _extra_state(self):
        return {"precision": self.precision, "weight_interp": self.weight_interp, "repeated_rows": self.repeated_rows}

    def _pack(self, device):
        return PackedEmbedding(self._state, device, precision=self.precision, weight_interp=self.weight_interp)

    PEEK_RECORD = ("form", "planes", "batch", "pending", "x5_valid", "pooled_rows", "P2", "T1", "T2", "T3", "T4", "T5",
                   "nt2", "pooled_ld")

    def peek_record(self, num_samples: int, handle=None) -> Dict[str, int]:
        """The record of ``dz_emb_peek`` (buffer 8, host memory) by name: what the buffers of the last call hold and
        in which form; no copy, no synchronisation.  ``handle``: one this model created for someone else."""
        ptr, cnt, _ = self._peek_raw(handle or self._handles[num_samples][0], 8)
        rec = (C.c_int * cnt).from_address(ptr.value)
        return dict(zip(self.PEEK_RECORD, rec))


class _HipGroupsEmbedding(_HipSpeakerEmbedding):
    """ECAPA-TDNN and the speechbrain x-vector: the same batch geometry, hence the same groups forward."""

    def forward_groups(self, waveform: torch.Tensor, masks: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """``waveform (G,1,S)``, ``masks (G,K,Fw)`` speaker-major -> ``(G,K,dimension)``: the counterpart of
        ``HipEmbedding.forward_multi``.  Each chunk's K rows are one call of their own, with the batch geometry
        (padded frames, relative lengths) of those K rows alone, as the live reference embeds a chunk
        (``StreamingInference`` at batch 1); all G groups run in one launch sequence whose geometry is derived on
        the device — no synchronisation.  ``normalize``: L2-normalise every row (``EmbeddingNormalization(1)``)."""
        if self.device is None:
            self.to(waveform.device)
        rows = _as_rows(waveform.to(self.device))
        G, S = rows.shape
        masks = masks.to(self.device, torch.float32).contiguous()
        if masks.ndim != 3 or masks.shape[0] != G:
            raise ValueError(f"masks must be (groups, speakers, frames), got {tuple(masks.shape)}")
        K = masks.shape[1]
        handle = self._need(S, G * K)
        out = torch.empty((G, K, self.dimension), dtype=torch.float32, device=self.device)
        self.groups_launch(handle, rows.data_ptr(), rows.stride(0) if G > 1 else S, masks.data_ptr(), G, K,
                           masks.shape[2], normalize, out.data_ptr(), _stream_ptr(self.device))
        return out

    def groups_launch(self, handle, wave_ptr: int, wave_stride: int, masks_ptr: int, G: int, K: int, mask_frames: int,
                      normalize: bool, out_ptr: int, stream_ptr: int) -> None:
        """``<_c>_forward_groups`` on a handle of this model (``GroupsBatch``'s lanes): raw device addresses,
        masks (G,K,Fw) contiguous, out (G*K,dimension); no synchronisation."""
        _lib.check(self._fn("forward_groups")(handle, wave_ptr, wave_stride, masks_ptr, G, K, mask_frames,
                                              1 if normalize else 0, out_ptr, stream_ptr), f"{self._c}_forward_groups")

    # the two-chain engine's hooks: the whole network consumes the masks, so nothing runs before the segmentation
    def engine_rows(self, n: int, K: int) -> int:
        return n * K

    def early_launch(self, handle, wave_ptr: int, wave_stride: int, N: int, stream_ptr: int) -> None:
        pass

    def late_launch(self, handle, wave_ptr: int, wave_stride: int, weights_ptr: int, N: int, K: int, F: int,
                    out_ptr: int, stream_ptr: int) -> None:
        self.groups_launch(handle, wave_ptr, wave_stride, weights_ptr, N, K, F, True, out_ptr, stream_ptr)


class HipEcapaEmbedding(_HipGroupsEmbedding):
    """speechbrain ECAPA-TDNN behind pyannote's ``PretrainedSpeakerEmbedding`` contract
    (BASELINE.json config 3): ``(waveform (N,1,S), masks (N,F) | None) -> (N,192)``; a row whose
    mask keeps fewer than 640 samples is NaN.  The reference reaches this model through the
    fallback at models.py:59 and calls it at :262; it returns numpy there, a device tensor here
    (``EmbeddingModel`` accepts both, models.py:263-264)."""

    dimension = 192
    _c, _packer, _int32_peeks = "dz_ecapa", PackedEcapa, frozenset((5, 6, 7, 8))

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 192, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None):
        super().__init__(state, max_batch, precision, repeated_rows)

    def last_frames(self, num_samples: int) -> int:
        """Frames of the batch geometry of the last forward (= those of its longest kept row, what every row is
        padded to: ``dz_ecapa_peek``); no copy, no synchronisation.  ``bench.py --config 3`` prices its kernels with it."""
        return self._peek_raw(self._handles[num_samples][0], 5)[2]


ECAPA_MEL_OPTIONS = ("min_num_samples",) + tuple(ECAPA_MEL_FEATURES)


class HipEcapaMelEmbedding(_HipGroupsEmbedding):
    """speechbrain's mel-spectrogram ECAPA-TDNN (speechbrain/spkrec-ecapa-voxceleb-mel-spec) behind pyannote's
    ``PretrainedSpeakerEmbedding`` contract, the wrapper the reference falls back to for it (models.py:59):
    ``(waveform (N,1,S), masks (N,F) | None) -> (N,192)``, not normalised; a row whose mask keeps fewer than
    ``min_num_samples`` (1024) samples, or whose kept samples hold a NaN, is NaN, and a call whose longest row is that
    short is all NaN.  ``HipEcapaEmbedding``'s network and checkpoint keys behind another front end: a centred,
    reflect-padded STFT of 1024 samples at hop 256 over the padded batch, magnitude, 80 slaney mel bins,
    ``log(max(x, 1e-5))``, sentence mean — 313 frames for 5 s instead of 501.  The same call shape as
    ``HipEcapaEmbedding``, so the same engine forms take it; masks select samples, so ``repeated_rows="share"`` is
    refused.  ``features``: the settings of ``weights.ECAPA_MEL_FEATURES``; a value the kernels are not built for is
    refused by name."""

    dimension = 192
    _c, _packer, _int32_peeks = "dz_ecm", PackedEcapaMel, frozenset((5, 6, 7, 8, 9))

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 192, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None, min_num_samples: int = ECAPA_MEL_MIN_NUM_SAMPLES, **features):
        super().__init__(state, max_batch, precision, repeated_rows)
        from .weights import ecapa_mel_features
        self.features = ecapa_mel_features(**features)
        self.min_num_samples = int(min_num_samples)
        if self.min_num_samples <= 512:
            raise ValueError(f"ecapa-mel: min_num_samples={min_num_samples} — the centred STFT reflects 512 samples, "
                             "which needs more than 512")

    def _extra_state(self):
        return dict(super()._extra_state(), min_num_samples=self.min_num_samples, **self.features)

    def _pack(self, device):
        return PackedEcapaMel(self._state, device, precision=self.precision, min_num_samples=self.min_num_samples,
                              **self.features)

    def num_frames(self, num_samples: int) -> int:
        """Frames every buffer lays a row of ``num_samples`` samples out with (``dz_ecm_frames_for``: 1 + S // 256)."""
        return int(_lib.load().dz_ecm_frames_for(int(num_samples)))

    def last_frames(self, num_samples: int) -> int:
        """Frames per row of the buffers of the last forward (``dz_ecm_peek``); no copy, no synchronisation."""
        return self._peek_raw(self._handles[num_samples][0], 5)[2]


class HipSbXvectorEmbedding(_HipGroupsEmbedding):
    """speechbrain's x-vector (speechbrain/spkrec-xvect-voxceleb) behind pyannote's ``PretrainedSpeakerEmbedding``
    contract, the wrapper the reference falls back to for it (models.py:59): ``(waveform (N,1,S), masks (N,F) |
    None) -> (N,512)``; a row whose mask keeps fewer than 480 samples, or whose kept samples hold a NaN, is NaN.
    The same call shape and batch geometry as ``HipEcapaEmbedding``, so the same engine forms take it."""

    dimension = 512
    min_num_samples = 480
    _c, _packer, _int32_peeks = "dz_sbx", PackedSbXvector, frozenset((7, 8, 9))

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 192, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None):
        super().__init__(state, max_batch, precision, repeated_rows)


TITANET_OPTIONS = ("pad_mode", "frame_count", "min_num_samples", "attention_order")


class HipTitaNetEmbedding(_HipGroupsEmbedding):
    """NeMo's TitaNet-L (nvidia/speakerverification_en_titanet_large) behind pyannote's ``PretrainedSpeakerEmbedding``
    contract, the NeMo wrapper the reference falls back to for it (models.py:59): ``(waveform (N,1,S), masks (N,F) |
    None) -> (N,192)``, not normalised; a row whose mask keeps fewer than ``min_num_samples`` samples, or whose kept
    samples hold a NaN, is NaN, and a call whose longest row is that short is all NaN.  The same call shape as
    ``HipEcapaEmbedding``, so the same engine forms take it; masks select samples, so ``repeated_rows="share"`` is
    refused.  ``pad_mode`` / ``frame_count`` / ``min_num_samples`` / ``attention_order``: the switches of
    ``weights.PackedTitaNet``."""

    dimension = 192
    _c, _packer, _int32_peeks = "dz_ttn", PackedTitaNet, frozenset((7, 8, 9))

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 192, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None, pad_mode: str = "reflect", frame_count: str = "floor_plus_one",
                 min_num_samples: int = TITANET_MIN_NUM_SAMPLES, attention_order: str = "relu_bn_tanh"):
        super().__init__(state, max_batch, precision, repeated_rows)
        self.pad_mode, self.frame_count, self.attention_order = pad_mode, frame_count, attention_order
        self.min_num_samples = int(min_num_samples)

    def _extra_state(self):
        return dict(super()._extra_state(), pad_mode=self.pad_mode, frame_count=self.frame_count,
                    min_num_samples=self.min_num_samples, attention_order=self.attention_order)

    def _pack(self, device):
        return PackedTitaNet(self._state, device, precision=self.precision, pad_mode=self.pad_mode,
                             frame_count=self.frame_count, min_num_samples=self.min_num_samples,
                             attention_order=self.attention_order)

    def num_frames(self, num_samples: int) -> int:
        """Frames every buffer lays a row of ``num_samples`` samples out with (``dz_ttn_frames_for``)."""
        return int(_lib.load().dz_ttn_frames_for(int(num_samples)))


SB_RESNET_OPTIONS = ("strides", "min_num_samples", "rows_per_pass")


class HipSbResNetEmbedding(_HipGroupsEmbedding):
    """speechbrain's ResNet (speechbrain/spkrec-resnet-voxceleb) behind pyannote's ``PretrainedSpeakerEmbedding``
    contract, the wrapper the reference falls back to for it (models.py:59): ``(waveform (N,1,S), masks (N,F) |
    None) -> (N,256)``, not normalised; a row whose mask keeps fewer than ``min_num_samples`` samples, or whose kept
    samples hold a NaN, is NaN.  ECAPA's front end and batch geometry, a 2-D squeeze-excitation ResNet over every frame
    of the padded batch, attentive statistics pooling.  The same call shape as ``HipEcapaEmbedding``,
    so the same engine forms take it; masks select samples, so ``repeated_rows="share"`` is refused.  ``strides``: the
    four layers' (not visible in the checkpoint's shapes); ``rows_per_pass``: rows the trunk runs over at a time (0:
    the library's default, 16; a handle's arena grows with it, no result depends on it)."""

    dimension = 256
    _c, _packer, _int32_peeks = "dz_sbr", PackedSbResNet, frozenset((7, 8, 9))

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 192, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None, strides=SB_RESNET_STRIDES,
                 min_num_samples: int = SB_RESNET_MIN_NUM_SAMPLES, rows_per_pass: int = 0):
        super().__init__(state, max_batch, precision, repeated_rows)
        self.strides = tuple(int(s) for s in strides)
        self.min_num_samples, self.rows_per_pass = int(min_num_samples), int(rows_per_pass)

    def _extra_state(self):
        return dict(super()._extra_state(), strides=self.strides, min_num_samples=self.min_num_samples,
                    rows_per_pass=self.rows_per_pass)

    def _pack(self, device):
        return PackedSbResNet(self._state, device, precision=self.precision, strides=self.strides,
                              min_num_samples=self.min_num_samples, rows_per_pass=self.rows_per_pass)


class HipWeSpeakerEmbedding(_HipTrunkEmbedding):
    """pyannote.audio 3.1's ``WeSpeakerResNet34`` (pyannote/wespeaker-voxceleb-resnet34-LM): ``(waveform (N,1,S),
    weights (N,Fw) | None) -> (N,256)`` — the callable the reference loads through ``PyannoteLoader`` (models.py:42-59)
    and calls at blocks/embedding.py:56-65.  kaldi fbank, ResNet34 trunk on implicit-GEMM 2-D convolutions
    (k_conv2d.hip), TSTP pooling with the 3.1 weighted statistics (nearest-resampled weights), ``seg_1``.  A row
    with a NaN / Inf sample comes back NaN."""

    dimension = 256
    _c, _packer = "dz_wsp", PackedWeSpeaker

    def __init__(self, state: Dict[str, torch.Tensor], max_batch: int = 64, precision: Optional[str] = None,
                 repeated_rows: Optional[str] = None):
        """``repeated_rows``: "each" | "share" (``repeated_rows_mode``)."""
        super().__init__(state, max_batch, precision, repeated_rows)

    def num_frames(self, num_samples: int, stage: int = 0) -> int:
        """Frames of the fbank (stage 0) or after layer 1 .. 4 (``dz_wsp_frames_for``)."""
        return int(_lib.load().dz_wsp_frames_for(int(num_samples), int(stage)))

    def trunk_launch(self, handle, wave_ptr: int, wave_stride: int, batch: int, stream_ptr: int) -> None:
        """``dz_wsp_trunk`` on a handle of this model (``WeSpeakerBatch``'s lanes): fbank + ResNet34 of ``batch``
        windows at raw device addresses, into the handle; no synchronisation."""
        _lib.check(_lib.load().dz_wsp_trunk(handle, wave_ptr, wave_stride, batch, stream_ptr), "dz_wsp_trunk")

    def pool_launch(self, handle, weights_ptr: int, batch: int, K: int, weight_frames: int, normalize: bool,
                    out_ptr: int, stream_ptr: int) -> None:
        """``dz_wsp_pool`` of the handle's last ``trunk_launch``: weights (batch,K,Fw) contiguous, out
        (batch*K,256); the caller has ordered ``stream_ptr`` behind the trunk's stream.  No synchronisation."""
        _lib.check(_lib.load().dz_wsp_pool(handle, weights_ptr, batch, K, weight_frames, 1 if normalize else 0,
                                           out_ptr, stream_ptr), "dz_wsp_pool")

    # the two-chain engine's hooks: the trunk runs beside the segmentation, only the pooling waits for it
    def engine_rows(self, n: int, K: int) -> int:
        return n

    early_launch = trunk_launch

    def late_launch(self, handle, wave_ptr: int, wave_stride: int, weights_ptr: int, N: int, K: int, F: int,
                    out_ptr: int, stream_ptr: int) -> None:
        self.pool_launch(handle, weights_ptr, N, K, F, True, out_ptr, stream_ptr)


# --------------------------------------------------------------------------- #
# loaders (picklable, no HIP state)
# --------------------------------------------------------------------------- #
class SegmentationLoader:
    def __init__(self, state: StateSource, max_batch: int = 64, powerset: bool = False,
                 precision: Optional[str] = None):
        self.state, self.max_batch, self.powerset, self.precision = state, max_batch, powerset, precision

    def __call__(self) -> HipSegmentation:
        return HipSegmentation(_read_state(self.state), self.max_batch, self.powerset, self.precision)


class EmbeddingLoader:
    """``arch``: "xvector" (pyannote/embedding), "ecapa" (speechbrain/spkrec-ecapa-voxceleb), "wespeaker"
    (pyannote/wespeaker-voxceleb-resnet34-LM), "sb-xvector" (speechbrain/spkrec-xvect-voxceleb), "sb-resnet"
    (speechbrain/spkrec-resnet-voxceleb), "ecapa-mel" (speechbrain/spkrec-ecapa-voxceleb-mel-spec) or "titanet"
    (nvidia/speakerverification_en_titanet_large, a ``.nemo`` archive); None = decide from the checkpoint keys (``encoder.encoder.0.mconv.0.conv.weight`` +
    ``decoder.emb_layers.0.1.weight``: titanet, ``resnet.``: wespeaker, ``asp.``: ecapa, speechbrain ``Xvector`` keys
    ``blocks.0.conv.weight`` + ``blocks.16.w.weight``: sb-xvector, speechbrain ``ResNet`` keys
    ``layer1.0.se.fc.0.weight`` + ``fc_embed.weight``: sb-resnet, otherwise xvector).  The mel-spectrogram ECAPA has
    the fbank ECAPA's keys: a state FILE beside which a ``hyperparams.yaml`` names ``mel_spectogram`` is "ecapa-mel"
    (``checkpoint.ecapa_mel_hyperparams``), a plain state dict with ``asp.`` keys stays "ecapa"."""

    def __init__(self, state: StateSource, max_batch: int = 64, arch: Optional[str] = None,
                 precision: Optional[str] = None, weight_interp: Optional[str] = None,
                 repeated_rows: Optional[str] = None, **arch_options):
        """``arch_options`` (titanet only): ``pad_mode``, ``frame_count``, ``min_num_samples``, ``attention_order`` of
        ``HipTitaNetEmbedding`` — the switches DESIGN.md 4.12 marks (R); they override what the archive's yaml records.
        ``arch_options`` (sb-resnet only): ``strides``, ``min_num_samples``, ``rows_per_pass`` of ``HipSbResNetEmbedding``.
        ``arch_options`` (ecapa-mel only): ``min_num_samples`` and the feature settings of ``HipEcapaMelEmbedding`` — the
        points DESIGN.md 4.15 marks (R); they override what a ``hyperparams.yaml`` beside the state file records.
        ``weight_interp`` (x-vector only): "linear" | "nearest" | None = from the ``pyannote.audio`` version the
        checkpoint file records (>= 3.1: "nearest"; older, absent, or a plain state dict: "linear").
        ``repeated_rows``: "each" | "share" (``repeated_rows_mode``: the reference-shaped ``(batch spk)`` call runs the
        trunk once per window; xvector and wespeaker only — ecapa, ecapa-mel, sb-xvector, sb-resnet and titanet refuse "share")."""
        if repeated_rows is not None and repeated_rows not in REPEATED_ROWS:
            raise ValueError(f"repeated_rows={repeated_rows!r}: expected one of {REPEATED_ROWS}")
        self.state, self.max_batch, self.arch, self.precision = state, max_batch, arch, precision
        self.weight_interp = weight_interp
        self.repeated_rows = repeated_rows
        unknown = set(arch_options) - set(TITANET_OPTIONS) - set(SB_RESNET_OPTIONS) - set(ECAPA_MEL_OPTIONS)
        if unknown:
            raise TypeError(f"EmbeddingLoader: unknown option(s) {sorted(unknown)} (titanet takes {TITANET_OPTIONS}, "
                            f"sb-resnet {SB_RESNET_OPTIONS}, ecapa-mel {ECAPA_MEL_OPTIONS})")
        self.arch_options = arch_options

    def __call__(self):
        sd = _read_state(self.state)
        arch = self.arch or ("ecapa" if any(k.startswith("asp.") for k in sd) else "xvector")
        if self.arch is None and any(k.startswith("resnet.") for k in sd):
            arch = "wespeaker"
        if arch == "xvector" and self.arch is None and "blocks.0.conv.weight" in sd and "blocks.16.w.weight" in sd:
            arch = "sb-xvector"     # (the pyannote x-vector packer has no ``blocks.`` keys: this state failed there)
        if self.arch is None and all(k in sd for k in TITANET_MARKERS):
            arch = "titanet"
        if arch == "xvector" and self.arch is None and all(k in sd for k in SB_RESNET_MARKERS):
            arch = "sb-resnet"      # (the pyannote x-vector packer has no ``layer1.`` keys: this state failed there)
        yaml_features = None
        if arch == "ecapa" and self.arch is None and not isinstance(self.state, dict):
            from .checkpoint import ecapa_mel_hyperparams
            yaml_features = ecapa_mel_hyperparams(self.state)
            if yaml_features is not None:
                arch = "ecapa-mel"
        if arch == "ecapa-mel":
            other = sorted(set(self.arch_options) - set(ECAPA_MEL_OPTIONS))
            if other:
                raise TypeError(f"EmbeddingLoader: {other} are options of another architecture, this state is {arch!r}")
            if yaml_features is None and not isinstance(self.state, dict):
                from .checkpoint import ecapa_mel_hyperparams
                yaml_features = ecapa_mel_hyperparams(self.state)
            kw = dict(yaml_features or {})
            kw.update(self.arch_options)
            return HipEcapaMelEmbedding(sd, self.max_batch, self.precision, self.repeated_rows, **kw)
        if arch == "sb-resnet":
            other = sorted(set(self.arch_options) - set(SB_RESNET_OPTIONS))
            if other:
                raise TypeError(f"EmbeddingLoader: {other} are options of the titanet architecture, this state is {arch!r}")
            return HipSbResNetEmbedding(sd, self.max_batch, self.precision, self.repeated_rows, **self.arch_options)
        if arch == "titanet":
            other = sorted(set(self.arch_options) - set(TITANET_OPTIONS))
            if other:
                raise TypeError(f"EmbeddingLoader: {other} are options of the sb-resnet architecture, this state is "
                                f"{arch!r}")
            # the front-end switches a .nemo archive's model_config.yaml records (checkpoint.nemo_frontend)
            kw = {}
            if not isinstance(self.state, dict):
                from .checkpoint import nemo_frontend
                kw = nemo_frontend(self.state)
            kw.update(self.arch_options)
            return HipTitaNetEmbedding(sd, self.max_batch, self.precision, self.repeated_rows, **kw)
        if self.arch_options:
            raise TypeError(f"EmbeddingLoader: {sorted(self.arch_options)} are options of the titanet, sb-resnet or ecapa-mel "
                            f"architecture, this state is {arch!r}")
        if arch == "sb-xvector":
            return HipSbXvectorEmbedding(sd, self.max_batch, self.precision, self.repeated_rows)
        if arch == "wespeaker":
            return HipWeSpeakerEmbedding(sd, self.max_batch, self.precision, self.repeated_rows)
        if arch == "ecapa":
            return HipEcapaEmbedding(sd, self.max_batch, self.precision, self.repeated_rows)
        interp = self.weight_interp
        if interp is None and not isinstance(self.state, dict):
            from .checkpoint import pyannote_version
            v = pyannote_version(self.state)
            interp = "nearest" if v is not None and v >= (3, 1) else "linear"
        return HipEmbedding(sd, self.max_batch, self.precision, interp, self.repeated_rows)


# --------------------------------------------------------------------------- #
# the reference's wrappers (same names, same semantics)
# --------------------------------------------------------------------------- #
class LazyModel:
    """Defers loading until first use; ``.to`` loads then moves; ``__call__`` forwards."""

    def __init__(self, loader: Callable[[], Callable]):
        self.get_model = loader
        self.model: Optional[Callable] = None

    def is_in_memory(self) -> bool:
        return self.model is not None

    def load(self):
        if self.model is None:
            self.model = self.get_model()

    def to(self, device: torch.device) -> "LazyModel":
        self.load()
        self.model = self.model.to(device)
        return self

    def eval(self) -> "LazyModel":
        self.load()
        if isinstance(self.model, nn.Module):
            self.model.eval()
        return self

    def __call__(self, *args, **kwargs):
        self.load()
        return self.model(*args, **kwargs)


def _no_onnx(*_a, **_k):
    raise NotImplementedError(
        "diart_amd replaces the torch/ONNX back-ends of the hot path with HIP kernels; "
        "ONNX models are not part of this path (reference models.py:62-109)")


class SegmentationModel(LazyModel):
    """``waveform (batch, channels, samples) -> (batch, frames, speakers)``."""

    from_onnx = staticmethod(_no_onnx)

    @staticmethod
    def from_state(state: StateSource, max_batch: int = 64, powerset: bool = False,
                   precision: Optional[str] = None) -> "SegmentationModel":
        return SegmentationModel(SegmentationLoader(state, max_batch, powerset, precision))

    @staticmethod
    def from_pyannote(model, use_hf_token=True) -> "SegmentationModel":
        """``model``: path to a pyannote checkpoint / state-dict file (the hub is unreachable
        from an air-gapped MI355X box, so hub names are rejected with a clear message)."""
        if isinstance(model, (str, Path)) and Path(model).exists():
            return SegmentationModel.from_state(model, powerset="3.0" in str(model))
        raise FileNotFoundError(
            f"'{model}': pass a local pyannote checkpoint / state-dict file "
            "(gated HuggingFace downloads are not available here)")

    @staticmethod
    def from_pretrained(model, use_hf_token=True) -> "SegmentationModel":
        if isinstance(model, (str, Path)) and Path(model).name.endswith(".onnx"):
            return SegmentationModel.from_onnx(model)
        if isinstance(model, dict):
            return SegmentationModel.from_state(model)
        return SegmentationModel.from_pyannote(model, use_hf_token)

    def __call__(self, waveform: torch.Tensor) -> torch.Tensor:
        return super().__call__(waveform)


class EmbeddingModel(LazyModel):
    """``(waveform (batch, channels, samples), weights (batch, frames) | None) ->
    (batch, embedding_dim)``; numpy results are converted like the reference does."""

    from_onnx = staticmethod(_no_onnx)

    @staticmethod
    def from_state(state: StateSource, max_batch: int = 64, arch: Optional[str] = None,
                   precision: Optional[str] = None, weight_interp: Optional[str] = None,
                   repeated_rows: Optional[str] = None, **arch_options) -> "EmbeddingModel":
        return EmbeddingModel(EmbeddingLoader(state, max_batch, arch, precision, weight_interp, repeated_rows,
                                              **arch_options))

    @staticmethod
    def from_pyannote(model, use_hf_token=True, repeated_rows: Optional[str] = None, **arch_options) -> "EmbeddingModel":
        if isinstance(model, (str, Path)) and Path(model).exists():
            return EmbeddingModel.from_state(model, repeated_rows=repeated_rows, **arch_options)
        raise FileNotFoundError(
            f"'{model}': pass a local pyannote checkpoint / state-dict file "
            "(gated HuggingFace downloads are not available here)")

    @staticmethod
    def from_pretrained(model, use_hf_token=True, repeated_rows: Optional[str] = None, **arch_options) -> "EmbeddingModel":
        """``arch_options``: the (R) switches of a TitaNet, speechbrain ResNet or mel-spectrogram ECAPA model
        (``EmbeddingLoader``)."""
        if isinstance(model, (str, Path)) and Path(model).name.endswith(".onnx"):
            return EmbeddingModel.from_onnx(model)
        if isinstance(model, dict):
            return EmbeddingModel.from_state(model, repeated_rows=repeated_rows, **arch_options)
        return EmbeddingModel.from_pyannote(model, use_hf_token, repeated_rows, **arch_options)

    def __call__(self, waveform: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = super().__call__(waveform, weights)
        if isinstance(out, np.ndarray):
            out = torch.from_numpy(out)
        return out
