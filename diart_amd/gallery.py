"""Who is speaking: a gallery of enrolled voiceprints on the GPU and the rule that turns its answers into labels.

The reference stops at ``speaker0``, ``speaker1``, ...: indices private to one stream.  ``SpeakerGallery`` holds up to
65 536 named voiceprints on the device; ``match`` finds, for every embedding row, the nearest voiceprint by the
clustering's own cosine distance, its distance and the runner-up's (``dz_gallery_match``, ``csrc/k_gallery.hip``: the
exact-f32 matrix instructions).  ``SpeakerNames`` is the host rule of the engines: per stream and
global speaker it keeps the closest match seen so far and hands out each voiceprint's name to one speaker at a time.
``_DiarizationEngine.set_gallery`` (``StreamBatch``, ``WeSpeakerBatch``, ``GroupsBatch``) and
``StreamServer.set_gallery`` attach a gallery to live streams.

There is no default identification threshold: the right ``delta_id`` depends on the embedding model and has not been
measured on real checkpoints here, so every caller gives it.

A gallery may carry a COHORT of impostor voiceprints (``cohort=``, ``with_cohort``).  ``match_normalised`` then
expresses every distance in standard deviations of the distances that its two sides get against their ``top_n`` nearest
cohort members (adaptive s-norm: ``dz_gallery_match_norm``, ``csrc/k_cohort.hip``), a signed quantity
whose threshold transfers across models and channels far better than a raw distance; the engines use it for a gallery
with a cohort.  The cohort should not contain the enrolled speakers: that is the caller's business and is not checked."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_ROWS, MAX_ENTRIES, MIN_DIM, MAX_DIM = 4096, 65536, 64, 512     # dz_gallery_match's domain (include/diart_amd.h)
MAX_COHORT, TOP_N = 8192, 300           # dz_gallery_set_cohort's domain; top_n of the published AS-norm recipes
_RESERVED = re.compile(r"speaker\d+")                               # the labels of speakers nobody has named


def check_delta_id(delta_id, who: str, signed: bool = False) -> float:
    """``signed``: the threshold of a normalised distance (a gallery with a cohort), any finite value."""
    what = "a finite normalised distance" if signed else "a finite distance >= 0"
    try:
        d = float(delta_id)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: delta_id={delta_id!r} ({what}; there is no default)") from None
    if not np.isfinite(d) or (d < 0 and not signed):
        raise ValueError(f"{who}: delta_id={delta_id!r} ({what}; there is no default)")
    return d


def check_cohort(cohort, top_n, D: int, who: str) -> Tuple[np.ndarray, int]:
    """``cohort`` (M, D) as contiguous float32 rows and ``top_n`` as an int, or a ``ValueError`` by name: what
    ``dz_gallery_set_cohort`` refuses, before anything touches the GPU."""
    if isinstance(cohort, torch.Tensor):
        cohort = cohort.detach().cpu().numpy()
    rows = np.ascontiguousarray(cohort, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] != D:
        raise ValueError(f"{who}: a cohort of shape {rows.shape} (expected (M, {D}), the voiceprints' dimension)")
    M = rows.shape[0]
    if not 1 <= M <= MAX_COHORT:
        raise ValueError(f"{who}: a cohort of {M} rows (1 .. {MAX_COHORT})")
    try:
        n = int(top_n)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: top_n={top_n!r} (1 .. the cohort's {M} rows)") from None
    if n != top_n or not 1 <= n <= M:
        raise ValueError(f"{who}: top_n={top_n!r} (1 .. the cohort's {M} rows)")
    finite = np.isfinite(rows).all(axis=1)
    if not finite.all():
        raise ValueError(f"{who}: cohort row {int(np.argmin(finite))} is not finite")
    norms = np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1))
    if not (norms > 0).all():
        raise ValueError(f"{who}: cohort row {int(np.argmin(norms > 0))} has zero norm")
    return rows, n


class _Handle:
    """One ``dz_gallery`` handle: the voiceprints on the device and the scratch of ONE match at a time (a handle per
    HIP stream that matches)."""

    def __init__(self, rows: np.ndarray, device: torch.device, cohort: Optional[np.ndarray] = None, top_n: int = TOP_N):
        self._lib = _lib.load()
        self.h = _lib.vp()
        self.E, D = rows.shape
        _lib.check(self._lib.dz_gallery_create(_lib.context(device.index), rows.ctypes.data, self.E, D, C.byref(self.h)),
                   "dz_gallery_create")
        if cohort is not None:           # uploads it and computes the voiceprints' statistics (synchronous)
            _lib.check(self._lib.dz_gallery_set_cohort(self.h, cohort.ctypes.data, cohort.shape[0], int(top_n)),
                       "dz_gallery_set_cohort")

    def match(self, rows_ptr: int, stride: int, R: int, index_ptr: int, dist_ptr: int, second_ptr: int,
              stream: int) -> None:
        _lib.check(self._lib.dz_gallery_match(self.h, rows_ptr, stride, R, index_ptr, dist_ptr, second_ptr, stream),
                   "dz_gallery_match")

    def match_norm(self, rows_ptr: int, stride: int, R: int, index_ptr: int, dist_ptr: int, second_ptr: int,
                   stream: int) -> None:
        _lib.check(self._lib.dz_gallery_match_norm(self.h, rows_ptr, stride, R, index_ptr, dist_ptr, second_ptr, stream),
                   "dz_gallery_match_norm")

    def cohort_stats(self, rows_ptr: int, stride: int, R: int, mean_ptr: int, std_ptr: int, stream: int) -> None:
        _lib.check(self._lib.dz_gallery_cohort_stats(self.h, rows_ptr, stride, R, mean_ptr, std_ptr, stream),
                   "dz_gallery_cohort_stats")

    def entry_stats(self) -> Tuple[np.ndarray, np.ndarray]:
        mean, std = np.empty(self.E, dtype=np.float32), np.empty(self.E, dtype=np.float32)
        _lib.check(self._lib.dz_gallery_entry_stats(self.h, mean.ctypes.data, std.ctypes.data), "dz_gallery_entry_stats")
        return mean, std

    def __del__(self):
        try:
            self._lib.dz_gallery_destroy(self.h)
        except Exception:
            pass


def _match_rows(handle: _Handle, x: torch.Tensor, normalised: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``x`` (R, D) float32 on the handle's GPU, rows at any stride >= D -> (index int32, distance, second) on that
    GPU, ``MAX_ROWS`` rows per launch, on the current stream."""
    R, D = x.shape
    index = torch.empty(R, dtype=torch.int32, device=x.device)
    dist = torch.empty(R, dtype=torch.float32, device=x.device)
    second = torch.empty(R, dtype=torch.float32, device=x.device)
    stride = x.stride(0) if R > 1 else D
    match = handle.match_norm if normalised else handle.match
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        for r0 in range(0, R, MAX_ROWS):
            n = min(MAX_ROWS, R - r0)
            match(x.data_ptr() + 4 * r0 * stride, stride, n, index[r0:].data_ptr(), dist[r0:].data_ptr(),
                  second[r0:].data_ptr(), st)
    return index, dist, second


def _stats_rows(handle: _Handle, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``_match_rows`` for the cohort statistics alone -> (mean, std) float32 on the handle's GPU."""
    R, D = x.shape
    mean = torch.empty(R, dtype=torch.float32, device=x.device)
    std = torch.empty(R, dtype=torch.float32, device=x.device)
    stride = x.stride(0) if R > 1 else D
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        for r0 in range(0, R, MAX_ROWS):
            n = min(MAX_ROWS, R - r0)
            handle.cohort_stats(x.data_ptr() + 4 * r0 * stride, stride, n, mean[r0:].data_ptr(), std[r0:].data_ptr(), st)
    return mean, std


def _rows_2d(embeddings: torch.Tensor, D: int, who: str) -> torch.Tensor:
    if embeddings.dtype != torch.float32:
        raise ValueError(f"{who}: {embeddings.dtype} embeddings (the kernel takes float32)")
    if embeddings.ndim < 1 or embeddings.shape[-1] != D or embeddings.numel() == 0:
        raise ValueError(f"{who}: embeddings of shape {tuple(embeddings.shape)} against voiceprints of dimension {D}")
    x = embeddings if embeddings.ndim == 2 else embeddings.reshape(-1, D)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < D):
        x = x.contiguous()
    return x


class SpeakerGallery:
    """``names[e]`` is the speaker whose voiceprint is ``voiceprints[e]``: (E, D) float32, 1 <= E <= 65 536, D a
    multiple of 64 from 64 to 512.  The rows are kept as given (``save`` / ``load`` round-trip them); the device copy
    is normalised, each voiceprint divided by its float64 norm and rounded to float32 once.  Refused with a
    ``ValueError``: duplicate names, names of the form ``speaker<digits>`` (what unnamed speakers are called),
    non-finite or zero voiceprints, a bad D or E.  Nothing touches the GPU before the first ``match`` (or an engine's
    ``set_gallery``); ``device=None`` is the current GPU then.

    ``cohort``: (M, D) impostor voiceprints, 1 <= M <= 8 192, validated and stored like voiceprints, with ``top_n`` in
    1 .. M (300: the value of the published AS-norm recipes, not measured here) -> ``match_normalised``,
    ``cohort_stats``, ``entry_stats``; ``match`` stays the raw match.  A cohort is built like a gallery, for example
    ``SpeakerGallery.enrol(model, impostor_audio).voiceprints``; it should not contain the enrolled speakers (not
    checked)."""

    def __init__(self, names: Sequence[str], voiceprints, device: Optional[torch.device] = None, cohort=None,
                 top_n: int = TOP_N):
        if isinstance(voiceprints, torch.Tensor):
            voiceprints = voiceprints.detach().cpu().numpy()
        rows = np.ascontiguousarray(voiceprints, dtype=np.float32)
        names = [n for n in names]
        if rows.ndim != 2:
            raise ValueError(f"SpeakerGallery: voiceprints of shape {rows.shape} (expected (E, D))")
        E, D = rows.shape
        if not 1 <= E <= MAX_ENTRIES:
            raise ValueError(f"SpeakerGallery: {E} voiceprints (1 .. {MAX_ENTRIES})")
        if not (MIN_DIM <= D <= MAX_DIM and D % 64 == 0):
            raise ValueError(f"SpeakerGallery: dimension {D} (a multiple of 64 from {MIN_DIM} to {MAX_DIM})")
        if len(names) != E:
            raise ValueError(f"SpeakerGallery: {len(names)} names for {E} voiceprints")
        bad = [n for n in names if not isinstance(n, str) or not n]
        if bad:
            raise ValueError(f"SpeakerGallery: names must be non-empty strings, got {bad[0]!r}")
        if len(set(names)) != E:
            seen, dup = set(), None
            for n in names:
                if n in seen:
                    dup = n
                    break
                seen.add(n)
            raise ValueError(f"SpeakerGallery: duplicate name {dup!r}")
        reserved = [n for n in names if _RESERVED.fullmatch(n)]
        if reserved:
            raise ValueError(f"SpeakerGallery: name {reserved[0]!r} is what an unnamed speaker is called (speaker<digits>)")
        finite = np.isfinite(rows).all(axis=1)
        if not finite.all():
            raise ValueError(f"SpeakerGallery: the voiceprint of {names[int(np.argmin(finite))]!r} is not finite")
        norms = np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1))
        if not (norms > 0).all():
            raise ValueError(f"SpeakerGallery: the voiceprint of {names[int(np.argmin(norms > 0))]!r} has zero norm")
        self._cohort, self._top_n = (None, top_n) if cohort is None else check_cohort(cohort, top_n, D, "SpeakerGallery")
        self._names: Tuple[str, ...] = tuple(names)
        self._rows = rows
        self.device = None if device is None else torch.device(device)
        self._handle: Optional[_Handle] = None

    # ------------------------------------------------------------------ what it holds
    @property
    def names(self) -> Tuple[str, ...]:
        return self._names

    @property
    def voiceprints(self) -> np.ndarray:
        """The float32 rows as given (not normalised)."""
        return self._rows

    @property
    def dimension(self) -> int:
        return int(self._rows.shape[1])

    def __len__(self) -> int:
        return int(self._rows.shape[0])

    @property
    def cohort(self) -> Optional[np.ndarray]:
        """The cohort's float32 rows as given (not normalised), or ``None``."""
        return self._cohort

    @property
    def top_n(self) -> int:
        return self._top_n

    def with_cohort(self, cohort, top_n: int = TOP_N) -> "SpeakerGallery":
        """A new gallery of the same names and voiceprints with this cohort (``None``: without one)."""
        return SpeakerGallery(self._names, self._rows, self.device, cohort, top_n)

    def save(self, path) -> None:
        """An ``.npz`` of the names and the float32 rows as given; with a cohort also its rows and ``top_n``."""
        extra = {} if self._cohort is None else dict(cohort=self._cohort, top_n=np.asarray(self._top_n, dtype=np.int64))
        with open(path, "wb") as f:
            np.savez(f, names=np.asarray(self._names, dtype=np.str_), voiceprints=self._rows, **extra)

    @staticmethod
    def load(path, device: Optional[torch.device] = None) -> "SpeakerGallery":
        with np.load(path, allow_pickle=False) as z:
            if "cohort" in z.files:
                return SpeakerGallery([str(n) for n in z["names"]], z["voiceprints"], device, z["cohort"], int(z["top_n"]))
            return SpeakerGallery([str(n) for n in z["names"]], z["voiceprints"], device)

    # ------------------------------------------------------------------ on the device
    def _resolve(self, device: Optional[torch.device] = None) -> torch.device:
        """The GPU this gallery lives on: the one it was given, else ``device``, else the current one; fixed from then on."""
        if self.device is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            self.device = dev
        if self.device.type != "cuda":
            raise ValueError(f"SpeakerGallery: device {self.device} (the gallery lives on a GPU)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def new_handle(self, device: Optional[torch.device] = None) -> _Handle:
        """A device copy with scratch of its own (an engine takes one per lane)."""
        return _Handle(self._rows, self._resolve(device), self._cohort, self._top_n)

    def _on_device(self, embeddings, who: str):
        """-> (rows (R, D) on the gallery's GPU, the leading shape, back): ``back`` gives tensors on the GPU their
        leading shape and the caller's kind (a CPU tensor or numpy array was uploaded and gets its own kind back)."""
        as_numpy = not isinstance(embeddings, torch.Tensor)
        x = torch.from_numpy(np.ascontiguousarray(embeddings)) if as_numpy else embeddings
        src = x.device
        dev = self._resolve(src if src.type == "cuda" else None)
        if src.type == "cuda" and src != dev:
            raise ValueError(f"{who}: embeddings on {src}, the gallery on {dev}")
        lead = tuple(x.shape[:-1])
        rows = _rows_2d(x.to(dev), self.dimension, who)
        if self._handle is None:
            self._handle = self.new_handle()

        def back(tensors):
            out = [t.reshape(lead) for t in tensors]
            if src.type != "cuda":
                out = [t.cpu() for t in out]                       # (synchronises)
            return tuple(t.numpy() for t in out) if as_numpy else tuple(out)
        return rows, back

    def _need_cohort(self, who: str) -> None:
        if self._cohort is None:
            raise ValueError(f"{who}: the gallery has no cohort (SpeakerGallery(..., cohort=...) or with_cohort)")

    def match_normalised(self, embeddings):
        """``match`` by the normalised distance (adaptive s-norm against the cohort; ``functional.
        gallery_match_normalised`` states it): ``(index int32, distance f32, second f32)`` shaped ``(...)``, the
        distances signed, lower is closer; -1 / NaN / NaN for an unusable row.  Always the kernels, as ``match``."""
        self._need_cohort("SpeakerGallery.match_normalised")
        rows, back = self._on_device(embeddings, "SpeakerGallery.match_normalised")
        return back(_match_rows(self._handle, rows, normalised=True))

    def cohort_stats(self, embeddings):
        """``(mean f32, std f32)`` shaped ``(...)``: mean and population standard deviation (never below 1e-3) of the
        distances of every row of ``embeddings (..., D)`` to its ``top_n`` nearest cohort members; NaN for an unusable
        row.  The bits of a row's pair depend on the row, the cohort and ``top_n`` only."""
        self._need_cohort("SpeakerGallery.cohort_stats")
        rows, back = self._on_device(embeddings, "SpeakerGallery.cohort_stats")
        return back(_stats_rows(self._handle, rows))

    def entry_stats(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(mean, std)`` of the E voiceprints against the cohort, float32 arrays: computed once per device copy."""
        self._need_cohort("SpeakerGallery.entry_stats")
        if self._handle is None:
            self._handle = self.new_handle()
        return self._handle.entry_stats()

    def match(self, embeddings):
        """The nearest voiceprint of every row of ``embeddings (..., D)`` float32 -> ``(index int32, distance f32,
        second f32)`` shaped ``(...)``: the index of the smallest cosine distance (the lowest among equals), that
        distance and the runner-up's (+inf for a gallery of one); -1 / NaN / NaN for a row with a NaN or Inf element or
        of zero norm.  Always the kernel, on the gallery's GPU: a CUDA tensor there gets tensors back (current stream,
        rows at a common stride read in place), a CPU tensor or numpy array is uploaded and gets its own kind back."""
        rows, back = self._on_device(embeddings, "SpeakerGallery.match")
        return back(_match_rows(self._handle, rows))

    # ------------------------------------------------------------------ enrolment
    @staticmethod
    def enrol(embedding_model, audio: Mapping[str, object], sample_rate: int = 16000, duration: float = 5.0,
              device: Optional[torch.device] = None) -> "SpeakerGallery":
        """A gallery from enrolment audio: ``audio[name]`` is that speaker's mono waveform (1-D, ``(1, S)`` or
        ``(S, 1)``) at ``sample_rate``.  A voiceprint is the normalised mean of the normalised embeddings of the
        consecutive ``duration``-second windows of the audio; a remainder shorter than a window is dropped, audio
        shorter than one window is a single row of its own length.  The model is called as the embedding block calls
        it without weights, ``model(waveform (rows, 1, samples)) -> (rows, D)``, which every embedding class of the
        loader answers.  A non-finite embedding is a ``ValueError`` naming the speaker."""
        W = int(round(sample_rate * duration))
        if W < 1:
            raise ValueError(f"SpeakerGallery.enrol: windows of {W} samples (sample_rate={sample_rate}, duration={duration})")
        if hasattr(embedding_model, "load"):
            embedding_model.load()                              # a LazyModel: the HIP model behind it
        inner = getattr(embedding_model, "model", None) or embedding_model
        dev = getattr(inner, "device", None)
        if dev is None and hasattr(embedding_model, "to"):      # a HIP model that is on no GPU yet
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            embedding_model.to(dev)
        elif dev is None:                                       # any other callable gets the rows where they are
            dev = torch.device("cpu")
        names, prints = [], []
        for name, wave in audio.items():
            w = torch.as_tensor(np.asarray(wave) if not isinstance(wave, torch.Tensor) else wave).detach()
            w = w.to(torch.float32).reshape(-1) if w.ndim <= 1 or 1 in w.shape else None
            if w is None or w.numel() == 0:
                raise ValueError(f"SpeakerGallery.enrol: the audio of {name!r} must be a non-empty mono waveform")
            n = w.numel() // W
            rows = w[:n * W].reshape(n, 1, W) if n >= 1 else w.reshape(1, 1, -1)
            with torch.no_grad():
                emb = embedding_model(rows.to(dev))
            emb = torch.as_tensor(emb).detach().to("cpu", torch.float64).reshape(rows.shape[0], -1)
            if not torch.isfinite(emb).all():
                raise ValueError(f"SpeakerGallery.enrol: the model's embedding of {name!r} is not finite")
            unit = emb / emb.norm(dim=1, keepdim=True)
            mean = unit.mean(dim=0)
            names.append(name)
            prints.append((mean / mean.norm()).to(torch.float32).numpy())
        if not names:
            raise ValueError("SpeakerGallery.enrol: no speakers")
        return SpeakerGallery(names, np.stack(prints), device)


class SpeakerNames:
    """The host rule that turns a step's matches into names, for ``num_streams`` streams of ``max_speakers`` global
    speakers each (vectorised numpy).  Per stream and global speaker g it keeps the closest match seen so far,
    ``(best_d[g], best_e[g])``: after a step's clustering every local speaker k with ``assign[k] = g >= 0``, a match
    ``index[k] = e >= 0`` and a distance ``d <= delta_id`` replaces it when ``d < best_d[g]`` (local speakers in
    ascending k).  A stream's labels are ``names[best_e[g]]`` where set; if several g of a stream hold the same
    voiceprint, the one with the lowest ``best_d`` keeps the name (ties: the lowest g) and the others read
    ``speaker{g}`` for that step, keeping their state.  ``delta_id`` has no default.  ``signed=True``: the distances
    are normalised ones (a gallery with a cohort) and any finite ``delta_id`` is a threshold; the rule is the same."""

    def __init__(self, num_streams: int, max_speakers: int, delta_id: float, signed: bool = False):
        self.delta_id = check_delta_id(delta_id, "SpeakerNames", signed)
        self.n, self.g = int(num_streams), int(max_speakers)
        if self.n < 1 or self.g < 1:
            raise ValueError(f"SpeakerNames: {num_streams} streams of {max_speakers} speakers")
        self.best_d = np.full((self.n, self.g), np.inf, dtype=np.float32)
        self.best_e = np.full((self.n, self.g), -1, dtype=np.int32)
        self._lower = np.tril(np.ones((self.g, self.g), dtype=bool), -1)

    def reset(self, slot: Optional[int] = None) -> None:
        """Forget every stream's matches, or one slot's."""
        sel = slice(None) if slot is None else int(slot)
        self.best_d[sel] = np.inf
        self.best_e[sel] = -1

    def update(self, assign: np.ndarray, index: np.ndarray, distance: np.ndarray, slots=None) -> None:
        """``assign``, ``index``, ``distance``: (N, K) of one step; row i belongs to stream ``slots[i]`` (default: all
        streams in order)."""
        assign, index, distance = np.asarray(assign), np.asarray(index), np.asarray(distance, dtype=np.float32)
        rows = np.arange(self.n) if slots is None else np.asarray(slots, dtype=np.int64)
        assert assign.shape == index.shape == distance.shape and assign.shape[0] == rows.shape[0]
        for k in range(assign.shape[1]):                 # K is the model's local speakers (3): the loop is over k only
            g, e, d = assign[:, k], index[:, k], distance[:, k]
            with np.errstate(invalid="ignore"):
                ok = (g >= 0) & (g < self.g) & (e >= 0) & (d.astype(np.float64) <= self.delta_id)   # (NaN: never)
            gs = np.where(ok, g, 0)
            ok &= d < self.best_d[rows, gs]
            self.best_d[rows[ok], gs[ok]] = d[ok]
            self.best_e[rows[ok], gs[ok]] = e[ok]

    def holders(self, slots=None) -> np.ndarray:
        """(N, G) int32: the voiceprint whose name global speaker g of each row's stream carries now, -1 where none."""
        rows = np.arange(self.n) if slots is None else np.asarray(slots, dtype=np.int64)
        bd, be = self.best_d[rows], self.best_e[rows]
        order = np.argsort(bd, axis=1, kind="stable")                    # lowest best_d first, ties: lowest g
        es = np.take_along_axis(be, order, axis=1)
        earlier = ((es[:, :, None] == es[:, None, :]) & self._lower).any(axis=2)     # a better holder of the same e
        keep = (es >= 0) & ~earlier
        out = np.full_like(be, -1)
        np.put_along_axis(out, order, np.where(keep, es, -1), axis=1)
        return out

    def labels(self, names: Sequence[str], slots=None) -> List[Dict[int, str]]:
        """Per row a dict g -> name of the global speakers that carry a name now."""
        hold = self.holders(slots)
        out: List[Dict[int, str]] = [{} for _ in range(hold.shape[0])]
        r, g = np.nonzero(hold >= 0)
        for ri, gi, e in zip(r.tolist(), g.tolist(), hold[r, g].tolist()):
            out[ri][gi] = names[e]
        return out
