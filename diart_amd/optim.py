"""Hyper-parameter tuning (reference: ``/root/reference/src/diart/optim.py``) by replaying cached model outputs.

``tau_active``, ``rho_update`` and ``delta_new`` — what ``SpeakerDiarization.hyper_parameters()`` returns — act only
after the networks: the segmentation scores, the overlapped-speech-penalty weights and the embeddings do not depend on
them.  The reference runs the whole pipeline over the whole dataset once per trial; here ``TuneCache.collect`` runs
the model half (``SpeakerDiarization.model_outputs``) once per file, and a trial is a replay of the cached
``(chunks, F, K)`` scores and ``(chunks, K, D)`` embeddings: clustering -> permutation -> Hamming aggregation ->
binarisation -> diarization error rate.  The ``T x N`` chains of T trials over N files are independent:

* ``backend="gpu"``: two HIP kernels (``csrc/k_tune.hip``): one wavefront per chain for the clustering, one thread per
  output frame for the aggregation, giving one 32-bit speaker mask per output frame;
* ``backend="host"``: the existing C ABI (``dz_clu_step`` / ``dz_tail_step``), chains on host threads — the same masks,
  bit for bit (``tests/test_gpu_tune.py``); what a machine without a GPU runs.

Either way ``dz_tune_score`` turns the masks into the error-rate components on host threads; with
``scoring="device"`` the GPU backend scores them where they are (``csrc/k_tune_score.hip``) and a batch of trials returns
``T x N x 5`` doubles and the statuses.  DESIGN.md 4.16.

``VoiceActivityDetection`` has ``tau_active`` alone and no clustering: ``VadTuneCache`` keeps one track per chunk (the
max over the local speakers), its aggregated speech score per output frame is computed once per cache, and a trial is
one comparison per frame plus the detection error rate — on the GPU both in HIP kernels (``csrc/k_tune_vad.hip``), so
that a batch of trials returns ``T x N x 5`` doubles and nothing else.

``OverlappedSpeechDetection`` is the same pipeline behind another track (the second largest over the local speakers)
and is scored against another reference (the regions where two different speakers are active): ``OsdTuneCache`` feeds
the VAD tuner's kernels and host code that track and the prefix sums of those regions.  A collected ``TuneCache`` holds
the raw scores both tracks are made of: ``VadTuneCache.from_tune_cache`` / ``OsdTuneCache.from_tune_cache``.

``delta_id``, the distance under which a speaker takes the name of an enrolled voiceprint (``gallery.py``), is tuned
on the same cache: ``TuneCache.with_gallery`` matches the cached embeddings against a ``SpeakerGallery`` once (the match
depends on no hyper-parameter) and returns an ``IdentTuneCache``, whose trials replay ``SpeakerNames`` over the
clustering's assignments and are scored by the identification error rate — names compared as they are, no mapping
(``csrc/k_tune_ident.hip``).
"""
from __future__ import annotations

import copy
import ctypes as C
import json
import re
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .blocks import base
from .features import Annotation, Segment
from .metrics import (DetectionErrorRate, DiarizationErrorRate, IdentificationErrorRate, OverlapDetectionErrorRate,
                      OverlapDetectionFMeasure, _turns, detection_prf, overlap_reference)

TUNABLE = ("tau_active", "rho_update", "delta_new")
IDENT_TUNABLE = TUNABLE + ("delta_id",)
VAD_TUNABLE = ("tau_active",)
# with hysteresis (blocks.base.TauOffset): the track pipelines' second threshold, replayed by tune_vad_score_kernel<TcHystRule>
# and the minimum durations (blocks.base.MinDurationOn / MinDurationOff), which act on a file's merged turns: <TcDurRule>
TRACK_TUNABLE = ("tau_active", "tau_offset", "min_duration_on", "min_duration_off")
DURATIONS = ("min_duration_on", "min_duration_off")
MAX_SPEAKERS = 32          # the hypothesis of a frame is one 32-bit mask
MAX_LOCAL_SPEAKERS = 8
PATCH_COLLAR = 0.05        # PredictionAccumulator's default


class TuneResult(NamedTuple):
    rate: np.ndarray          # (T,)   NaN for a trial with a non-negative status anywhere
    components: np.ndarray    # (T, 5) metrics.COMPONENTS summed over the files
    per_file: np.ndarray      # (T, N, 5)
    status: np.ndarray        # (T, N) -1, or the chunk at which the clustering would raise


def _config_meta(config) -> Dict[str, float]:
    get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
    meta = {k: float(get(k)) for k in ("step", "latency") + TUNABLE}
    meta["max_speakers"] = int(get("max_speakers"))
    return meta


def _reference_turns(reference) -> List[tuple]:
    """(start, end, label) of the reference as the metric sees it: same-label turns that touch are one turn."""
    if isinstance(reference, Annotation):
        return _turns(reference)
    ann = Annotation()
    for n, (s, e, label) in enumerate(reference):
        ann[Segment(float(s), float(e)), n] = str(label)
    return _turns(ann)


class _ReplayCache:
    """What ``TuneCache`` and ``VadTuneCache`` share: the file handling of ``collect``, and the trial-independent
    preparation — the output tail's plan (rows, buffers and cropped rows of every step, first-chunk prepend included),
    the frame middles of every step's output grid and the file's scoring cells (the sorted union of every time at
    which a hypothesis turn can start or end and of the reference's turn boundaries, each with its duration and the
    reference bits active in it).  A subclass sets ``files`` (dicts with ``uri``, ``starts``, ``res``, ``shift``,
    ``turns``), ``meta`` (``step``, ``latency``), ``F`` and ``N``, and says which bit a reference label is."""

    def _reference_bits(self, f: dict) -> Dict[object, int]:
        raise NotImplementedError

    @staticmethod
    def _collect_files(pipeline, speech_path, reference_path, batch_size: int, outputs) -> List[dict]:
        """Every WAV of ``speech_path`` with ``Benchmark.run_single``'s file handling: ``outputs(batch)`` gives the
        model outputs of a batch of chunks as numpy arrays (the first one ``(batch, frames, ...)``); per file their
        concatenation over the chunks, the window starts, ``finalise``'s frame resolution, the shift, the reference."""
        from .features import load_rttm
        speech_path, reference_path = Path(speech_path).expanduser(), Path(reference_path).expanduser()
        assert speech_path.is_dir(), "Speech path must be a directory"
        assert reference_path.is_dir(), "Reference path must be a directory"
        files = []
        for fp in sorted(p for p in speech_path.iterdir() if p.suffix.lower() == ".wav"):
            f = _ReplayCache._collect_file(pipeline, fp, batch_size, outputs)
            f["reference"] = load_rttm(reference_path / f"{fp.stem}.rttm").popitem()[1]
            files.append(f)
        return files

    @staticmethod
    def _collect_file(pipeline, fp, batch_size: int, outputs) -> dict:
        """One WAV of ``_collect_files``, without its reference (``offline.OfflineDiarization`` collects a file alone)."""
        from .inference import file_blocks, read_wav, resample_file, rolling_windows
        fp = Path(fp)
        cfg = pipeline.config
        waveform, sr = read_wav(fp)
        padding = cfg.get_padding(len(waveform) / sr)
        if sr != cfg.sample_rate:
            if getattr(getattr(cfg, "device", None), "type", None) != "cuda":
                raise ValueError(f"{fp} has sample rate {sr}, the pipeline's is {cfg.sample_rate} and the pipeline "
                                 "has no GPU device to resample on; resample the file first")
            waveform, sr = resample_file(waveform, sr, cfg.sample_rate, cfg.device), cfg.sample_rate
        outs, starts, res, batch = [], [], [], []

        def flush():
            arrays = outputs(batch)
            outs.append(arrays)
            starts.extend(w.extent.start for w in batch)
            res.extend([batch[0].extent.duration / arrays[0].shape[1]] * len(batch))     # finalise's seg_resolution
            batch.clear()

        for window in rolling_windows(file_blocks(waveform, sr, padding, cfg.step), cfg.duration, cfg.step, sr):
            batch.append(window)
            if len(batch) == max(1, int(batch_size)):
                flush()
        if batch:
            flush()
        if not outs:
            raise ValueError(f"{fp} is shorter than one chunk")
        return dict(uri=fp.stem, outputs=[np.concatenate(a) for a in zip(*outs)], starts=np.array(starts),
                    res=np.array(res), shift=-padding[0])

    def _prepare_plan(self) -> None:
        lib = _lib.load()
        F, m = self.F, self.meta
        self.nwin = int(round(m["latency"] / m["step"]))
        self.starts = np.concatenate([f["starts"] for f in self.files])
        self.res = np.concatenate([f["res"] for f in self.files])
        counts = [f["starts"].shape[0] for f in self.files]
        self.chunk_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        total = int(self.chunk_off[-1])
        self.hamming = np.ascontiguousarray(np.hamming(F), dtype=np.float64)
        # the tail's plan, file by file
        self.plan = np.zeros((total, 4 + self.nwin), dtype=np.int32)
        self.t0, self.out_res = np.zeros(total), np.zeros(total)
        for n in range(self.N):
            a, b = int(self.chunk_off[n]), int(self.chunk_off[n + 1])
            plan, t0, res = self.plan[a:b], self.t0[a:b], self.out_res[a:b]
            _lib.check(lib.dz_tune_plan(b - a, F, m["step"], m["latency"], self.starts[a:b].ctypes.data,
                                        self.res[a:b].ctypes.data, plan.ctypes.data, t0.ctypes.data, res.ctypes.data),
                       "dz_tune_plan")
        self.step_rows = np.ascontiguousarray(self.plan[:, 0] + self.plan[:, 1], dtype=np.int32)
        self.row_off = np.concatenate([[0], np.cumsum(self.step_rows)]).astype(np.int32)
        self.total_rows = int(self.row_off[-1])
        self.row_chunk = np.repeat(np.arange(total, dtype=np.int32), self.step_rows)
        self.file_row_off = np.ascontiguousarray(self.row_off[self.chunk_off], dtype=np.int32)
        # frame middles of every step's output grid (rows + 1 per step: the row after the last closes open turns),
        # with Binarize's expression, plus the shift
        per = self.step_rows.astype(np.int64) + 1
        step_of = np.repeat(np.arange(total), per)
        first = np.concatenate([[0], np.cumsum(per)])[:-1]
        i = (np.arange(int(per.sum())) - first[step_of]).astype(np.float64)
        s = self.t0[step_of] + i * self.out_res[step_of]
        shift = np.repeat(np.array([f["shift"] for f in self.files]), np.diff(self.chunk_off))[step_of]
        self.mids = np.ascontiguousarray(0.5 * (s + (s + self.out_res[step_of])) + shift)
        # scoring cells
        self.mid_cell = np.zeros(self.mids.shape[0], dtype=np.int32)
        durs, refs, cell_off = [], [], [0]
        self.ref_labels = []
        for n, f in enumerate(self.files):
            a = int(self.file_row_off[n] + self.chunk_off[n])
            b = int(self.file_row_off[n + 1] + self.chunk_off[n + 1]) if n + 1 < self.N else self.mids.shape[0]
            bit = self._reference_bits(f)
            rs = np.array([t[0] for t in f["turns"]], dtype=np.float64)
            re = np.array([t[1] for t in f["turns"]], dtype=np.float64)
            bounds = np.unique(np.concatenate([self.mids[a:b], rs, re]))
            self.mid_cell[a:b] = np.searchsorted(bounds, self.mids[a:b])
            mask = np.zeros(bounds.shape[0] - 1, dtype=np.uint64)
            for (s_, e_, l) in f["turns"]:
                i0, i1 = np.searchsorted(bounds, s_), np.searchsorted(bounds, e_)
                mask[i0:i1] |= np.uint64(1) << np.uint64(bit[l])
            durs.append(np.diff(bounds))
            refs.append(mask)
            cell_off.append(cell_off[-1] + mask.shape[0])
        self.cell_dur = np.ascontiguousarray(np.concatenate(durs), dtype=np.float64)
        self.cell_ref = np.ascontiguousarray(np.concatenate(refs), dtype=np.uint64)
        self.file_cell_off = np.array(cell_off, dtype=np.int32)
        self.max_cells = int(np.diff(self.file_cell_off).max())
        # the scoring kernels take the turns of a file in step order: that is their order by start time when every
        # step's grid starts behind the last row of the step before it (any file the file loop produces)
        first = (self.row_off[:-1] + np.arange(self.row_off.shape[0] - 1))[1:]
        last = (self.row_off[1:] + np.arange(self.row_off.shape[0] - 1) - 1)[:-1]
        inner = np.ones(first.shape[0], dtype=bool)
        inner[self.chunk_off[1:-1] - 1] = False                                        # the first step of a file
        self.sorted_steps = bool((self.mids[first] > self.mids[last])[inner].all())

    def _check_sorted(self, what: str, instead: str = "backend='host'") -> None:
        if not self.sorted_steps:
            raise ValueError(f"{what} scores the turns of a file in step order, and the output grids of "
                             f"this cache's steps are not sorted by time; {instead} sorts them")

    @staticmethod
    def default_backend() -> str:
        return "gpu" if torch.cuda.is_available() else "host"

    def _cells(self, ptr) -> _lib.TuneCells:
        """The scoring geometry as the descriptor the entry points take (``dz_tune_cells``): ``ptr(name)`` is the address
        of the cache's array ``name``, or None for one this cache does not have (which no entry it calls reads).  One
        hypothesis label for a cache without ``G`` (the track caches)."""
        c = _lib.TuneCells()
        for name in _lib.TuneCells.POINTERS:
            setattr(c, name, ptr("chunk_off" if name == "file_chunk_off" else name))
        c.n_files, c.total_rows, c.total_chunks = self.N, self.total_rows, int(self.chunk_off[-1])
        c.max_cells, c.max_speakers, c.collar = self.max_cells, getattr(self, "G", 1), PATCH_COLLAR
        return c

    def _host_cells(self) -> _lib.TuneCells:
        """``_cells`` over the cache's own arrays, built once and kept beside the arrays it points into: it is built
        again when one of them is no longer the cache's (an array replaced, or one this cache gained, as ``cell_step``)."""
        names = ["chunk_off" if n == "file_chunk_off" else n for n in _lib.TuneCells.POINTERS]
        arrays = [getattr(self, n, None) for n in names]
        kept = self.__dict__.get("_cells_host")
        if kept is None or any(a is not b for a, b in zip(kept[1], arrays)):
            at = dict(zip(names, arrays))
            kept = self._cells_host = (self._cells(lambda n: None if at[n] is None else at[n].ctypes.data), arrays)
        return kept[0]

    def _score_bits(self, bits: np.ndarray, num_threads: int) -> np.ndarray:
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        T = bits.shape[0]
        out = np.zeros((T, self.N, 5), dtype=np.float64)
        _lib.check(_lib.load().dz_tune_score(C.byref(self._host_cells()), T, bits.ctypes.data, out.ctypes.data,
                                             int(num_threads)), "dz_tune_score")
        return out

    def _hypothesis(self, bits_row: np.ndarray, n: int, speakers: int, label) -> Annotation:
        ann = Annotation(uri=self.files[n]["uri"], modality="speech")
        p, m = int(self.file_row_off[n]), int(self.file_row_off[n] + self.chunk_off[n])
        for c in range(int(self.chunk_off[n]), int(self.chunk_off[n + 1])):
            rows = int(self.step_rows[c])
            b = bits_row[p:p + rows]
            for g in range(speakers):
                on = np.concatenate([[False], (b >> np.uint32(g)) & np.uint32(1) > 0, [False]])
                edges = np.flatnonzero(on[1:] != on[:-1])
                for s, e in zip(edges[::2], edges[1::2]):
                    ann[Segment(self.mids[m + s], self.mids[m + e]), g] = label(g)
            p, m = p + rows, m + rows + 1
        return ann.support(PATCH_COLLAR)


def _diarization_outputs(pipeline):
    """``outputs(batch)`` of ``_collect_files`` for ``SpeakerDiarization``: the model half's scores and embeddings of a
    batch of chunks as float32 arrays."""
    def outputs(batch):
        s, e = pipeline.model_outputs(batch)
        s = s.detach().cpu().numpy().astype(np.float32, copy=False)
        e = e.detach().cpu().numpy().astype(np.float32, copy=False)
        return s, (e if e.ndim == 3 else e[None])
    return outputs


def _rates(comp: np.ndarray) -> np.ndarray:
    """``_Accumulating._rate`` of ``(T, 5)`` components."""
    err = comp[:, 2] + comp[:, 3] + comp[:, 4]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(comp[:, 0] > 0, err / comp[:, 0], np.where(err == 0, 0.0, 1.0))


class TuneCache(_ReplayCache):
    """The trial-independent half of a tuning run: per file the model outputs, the window start times, the frame
    resolution ``finalise`` was given, the timestamp shift and the reference turns — and, computed once from them on
    the host, what every trial shares: what ``identify`` derives from ``seg`` (float32 max, float32 sequential mean, NaN
    flags), the output tail's plan (rows, buffers and cropped rows of every step, first-chunk prepend included) and the
    file's scoring cells (the sorted union of every time at which a hypothesis turn can start or end and of the
    reference's turn boundaries, each with its duration and the reference speakers active in it)."""

    def __init__(self, files: Sequence[dict], config):
        self.meta = _config_meta(config)
        G = self.meta["max_speakers"]
        if G > MAX_SPEAKERS:
            raise ValueError(f"max_speakers = {G}: the replay keeps one 32-bit mask per frame, at most {MAX_SPEAKERS} speakers")
        if not files:
            raise ValueError("TuneCache needs at least one file")
        self.files = []
        for i, f in enumerate(files):
            seg = np.ascontiguousarray(f["seg"], dtype=np.float32)
            emb = np.ascontiguousarray(f["emb"], dtype=np.float32)
            starts = np.ascontiguousarray(f["starts"], dtype=np.float64)
            C_ = seg.shape[0]
            if seg.ndim != 3 or emb.ndim != 3 or emb.shape[:2] != (C_, seg.shape[2]) or starts.shape != (C_,) or C_ < 1:
                raise ValueError(f"file {i}: seg (C, F, K), emb (C, K, D), starts (C) expected, got {seg.shape}, "
                                 f"{emb.shape}, {starts.shape}")
            res = np.ascontiguousarray(np.broadcast_to(np.asarray(f["res"], dtype=np.float64), (C_,)))
            self.files.append(dict(uri=str(f.get("uri", f"file{i}")), seg=seg, emb=emb, starts=starts, res=res,
                                   shift=float(f.get("shift", 0.0)), turns=_reference_turns(f["reference"])))
        shapes = {(f["seg"].shape[1:], f["emb"].shape[2]) for f in self.files}
        if len(shapes) != 1:
            raise ValueError(f"the files of one cache share frames, local speakers and dimension, got {sorted(shapes)}")
        (self.F, self.K), self.D = next(iter(shapes))
        if self.K > MAX_LOCAL_SPEAKERS:
            raise ValueError(f"{self.K} local speakers per chunk (at most {MAX_LOCAL_SPEAKERS})")
        self.G, self.N = G, len(self.files)
        self._prepare()
        self._dev = {}

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, files: Sequence[dict], config) -> "TuneCache":
        """``files``: dicts with ``seg (C, F, K)``, ``emb (C, K, D)``, ``starts (C)``, ``res`` (the frame resolution
        ``finalise`` computes, one value or one per chunk), ``shift``, ``reference`` (an ``Annotation`` or
        ``(start, end, label)`` tuples) and optionally ``uri``.  ``config``: anything with ``step``, ``latency``,
        ``max_speakers`` and the three hyper-parameters (attributes or keys)."""
        return cls(files, config)

    @classmethod
    def collect(cls, pipeline_class, base_config, speech_path, reference_path, batch_size: int = 32) -> "TuneCache":
        """Run the model half of ``SpeakerDiarization`` once per WAV of ``speech_path`` (no ``finalise``, no
        clustering), with ``Benchmark.run_single``'s file handling."""
        _check_pipeline_class(pipeline_class)
        if int(base_config.max_speakers) > MAX_SPEAKERS:
            raise ValueError(f"max_speakers = {base_config.max_speakers}: the replay keeps one 32-bit mask per frame, "
                             f"at most {MAX_SPEAKERS} speakers")
        pipeline = pipeline_class(base_config)
        files = cls._collect_files(pipeline, speech_path, reference_path, batch_size, _diarization_outputs(pipeline))
        for f in files:
            f["seg"], f["emb"] = f.pop("outputs")
        return cls(files, pipeline.config)

    def _payload(self) -> dict:
        out = {"meta": np.array(json.dumps(self.meta)), "uris": np.array([f["uri"] for f in self.files])}
        for i, f in enumerate(self.files):
            for k in ("seg", "emb", "starts", "res"):
                out[f"{k}_{i}"] = f[k]
            out[f"shift_{i}"] = np.array(f["shift"])
            out[f"ref_times_{i}"] = np.array([[s, e] for s, e, _ in f["turns"]], dtype=np.float64).reshape(-1, 2)
            out[f"ref_labels_{i}"] = np.array([str(l) for _, _, l in f["turns"]], dtype=str)
        return out

    def save(self, path) -> None:
        with open(path, "wb") as fh:
            np.savez(fh, **self._payload())

    @staticmethod
    def _stored(z) -> "TuneCache":
        meta = json.loads(str(z["meta"]))
        files = []
        for i, uri in enumerate(z["uris"]):
            ref = [(s, e, str(l)) for (s, e), l in zip(z[f"ref_times_{i}"], z[f"ref_labels_{i}"])]
            files.append(dict(uri=str(uri), seg=z[f"seg_{i}"], emb=z[f"emb_{i}"], starts=z[f"starts_{i}"],
                              res=z[f"res_{i}"], shift=float(z[f"shift_{i}"]), reference=ref))
        return TuneCache(files, meta)

    @classmethod
    def load(cls, path) -> "TuneCache":
        with np.load(path, allow_pickle=False) as z:
            if "kind" in z.files:
                raise ValueError(f"{path} holds a {str(z['kind'])}, not a TuneCache (SpeakerDiarization)")
            return cls._stored(z)

    def with_gallery(self, gallery, device=None, normalised: bool = False, top_n=None) -> "IdentTuneCache":
        """This cache with the match of every cached embedding against ``gallery`` (a ``SpeakerGallery``): an
        ``IdentTuneCache``, which tunes ``delta_id`` beside the three.  The files, the plan and the device copies are
        shared, not copied.  The match is ``gallery.match`` on the GPU when there is one (``device``: which), else
        ``functional.gallery_match``'s float64 statement rounded to float32.  A gallery with a cohort is refused
        without ``normalised=True``: the live engines match it by the normalised distance, while ``DeltaId``'s range
        and a raw cache's ``match_distance`` are for raw distances.

        ``normalised=True`` (a gallery with a cohort): the stored match is the normalised one, a signed ``dn``, in one
        PLANE per value of ``top_n`` (None: the gallery's own; else 1 to 8 distinct integers in 1 .. the cohort's rows).
        Plane p is ``gallery.with_cohort(gallery.cohort, top_ns[p]).match_normalised(emb)`` on the GPU, the kernels
        the live engines run (one device copy at a time), or ``functional.gallery_match_normalised``'s float64 statement
        rounded to float32 without one."""
        cohort = getattr(gallery, "cohort", None)
        if not normalised:
            if top_n is not None:
                raise ValueError("TuneCache.with_gallery: top_n= chooses the planes of the normalised match; it needs "
                                 "normalised=True")
            if cohort is not None:
                raise ValueError("TuneCache.with_gallery: the gallery has a cohort, so the live engines match it by the "
                                 "normalised distance, and delta_id is tuned on raw distances only; tune gallery."
                                 "with_cohort(None), or tune the normalised threshold with normalised=True")
            return IdentTuneCache(self, gallery, device=device)
        if cohort is None:
            raise ValueError("TuneCache.with_gallery(normalised=True): the gallery has no cohort to normalise against "
                             "(SpeakerGallery(..., cohort=...) or with_cohort)")
        return IdentTuneCache(self, gallery, device=device, top_ns=_check_top_ns(top_n, gallery, "TuneCache.with_gallery"))

    # ------------------------------------------------------------------------------------------ trial-independent parts
    def _reference_bits(self, f: dict) -> Dict[object, int]:
        labels = sorted({l for _, _, l in f["turns"]}, key=str)
        if len(labels) > 64:
            raise ValueError(f"{f['uri']}: {len(labels)} reference speakers (at most 64)")
        self.ref_labels.append(labels)
        return {l: i for i, l in enumerate(labels)}

    def _prepare(self) -> None:
        F, K = self.F, self.K
        self._prepare_plan()
        self.seg = np.concatenate([f["seg"] for f in self.files])
        self.emb = np.concatenate([f["emb"] for f in self.files])
        total = int(self.chunk_off[-1])
        # what identify derives from seg: NaN flag, max, and the float32 mean summed over the frames in order
        seg_nan = np.isnan(self.seg).any(axis=1)
        with np.errstate(invalid="ignore"):
            self.pre_max = np.ascontiguousarray(np.where(seg_nan, np.float32(0), self.seg.max(axis=1)), dtype=np.float32)
            acc = np.zeros((total, K), dtype=np.float32)
            for f in range(F):
                acc += self.seg[:, f, :]
            self.pre_mean = np.ascontiguousarray(acc / np.float32(F), dtype=np.float32)
        self.pre_flags = np.ascontiguousarray(seg_nan.astype(np.uint8) | (np.isnan(self.emb).any(axis=2).astype(np.uint8) << 1))

    def _desc(self, ptr) -> _lib.TuneDesc:
        d = _lib.TuneDesc()
        for name in ("seg", "emb", "pre_max", "pre_mean", "pre_flags", "chunk_off", "plan", "row_off", "row_chunk", "hamming"):
            setattr(d, name, ptr(name))
        d.N, d.F, d.K, d.D, d.G, d.nwin = self.N, self.F, self.K, self.D, self.G, self.nwin
        d.total_chunks, d.total_rows = int(self.chunk_off[-1]), self.total_rows
        return d

    @property
    def bytes_per_trial(self) -> int:
        """Device (and host) memory one trial's results take: the assignments, the frame masks, the statuses."""
        return int(self.chunk_off[-1]) * self.K + 4 * self.total_rows + 4 * self.N

    # ------------------------------------------------------------------------------------------ replay
    @staticmethod
    def _hparams(hparams) -> np.ndarray:
        hp = np.ascontiguousarray(np.atleast_2d(np.asarray(hparams, dtype=np.float64)))
        if hp.ndim != 2 or hp.shape[1] != 3 or hp.shape[0] < 1:
            raise ValueError(f"hparams (T, 3) = (tau_active, rho_update, delta_new) per trial expected, got {hp.shape}")
        return hp

    def replay(self, hparams, backend: Optional[str] = None, num_threads: int = 8):
        """``(assign (T, chunks, K) int8, status (T, N) int32, bits (T, rows) uint32)`` of T trials: the global speaker
        of every local one (-1: none), the chunk at which a chain stopped (-1: it ran to the end) and one speaker mask
        per packed output frame.  ``backend``: "gpu" | "host" | "core" (the kernels' text on the host)."""
        hp = self._hparams(hparams)
        backend = backend or self.default_backend()
        if backend == "gpu":
            a, s, b = self._replay_gpu(hp)
            torch.cuda.synchronize(a.device)
            return a.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy().view(np.uint32)
        if backend not in ("host", "core"):
            raise ValueError(f"backend '{backend}': gpu, host or core")
        T, total = hp.shape[0], int(self.chunk_off[-1])
        assign = np.empty((T, total, self.K), dtype=np.int8)
        status = np.empty((T, self.N), dtype=np.int32)
        bits = np.empty((T, self.total_rows), dtype=np.uint32)
        d = self._desc(lambda name: getattr(self, name).ctypes.data)
        _lib.check(_lib.load().dz_tune_replay_host(C.byref(d), hp.ctypes.data, T, self.meta["step"], self.meta["latency"],
                                                   self.starts.ctypes.data, self.res.ctypes.data, assign.ctypes.data,
                                                   status.ctypes.data, bits.ctypes.data, int(backend == "core"),
                                                   int(num_threads)), "dz_tune_replay_host")
        return assign, status, bits

    def _device(self, device: torch.device):
        key = str(device)
        if key not in self._dev:
            tensors = {name: torch.from_numpy(getattr(self, name)).to(device)
                       for name in ("seg", "emb", "pre_max", "pre_mean", "pre_flags", "chunk_off", "plan", "row_off",
                                    "row_chunk", "hamming", "mids", "mid_cell", "file_cell_off", "cell_dur")}
            tensors["cell_ref"] = torch.from_numpy(self.cell_ref.view(np.int64)).to(device)      # (the 64 bits as they are)
            ptr = lambda name: tensors[name].data_ptr() if name in tensors else None
            self._dev[key] = (tensors, self._desc(ptr), self._cells(ptr))
        return self._dev[key]

    WORK_BLOCKS = 2048          # resident chains: 256 CUs x 8 one-wave workgroups

    def _replay_gpu(self, hp: np.ndarray, device: Optional[torch.device] = None, phases: int = 3, into=None):
        if not torch.cuda.is_available():
            raise _lib.DiartAmdError("backend='gpu' needs a GPU; backend='host' replays on the host")
        device = device or torch.device("cuda", torch.cuda.current_device())
        desc = self._device(device)[1]
        T, total = hp.shape[0], int(self.chunk_off[-1])
        d_hp = torch.from_numpy(hp).to(device)
        if into is not None:                     # (measurements: one phase on the arrays of an earlier call)
            assign, status, bits = into
        else:
            assign = torch.empty((T, total, self.K), dtype=torch.int8, device=device)
            status = torch.empty((T, self.N), dtype=torch.int32, device=device)
            bits = torch.empty((T, self.total_rows), dtype=torch.int32, device=device)
        blocks = min(T * self.N, self.WORK_BLOCKS)
        work = torch.empty((blocks, self.D * self.G), dtype=torch.float64, device=device)
        _lib.check(_lib.load().dz_tune_replay(_lib.context(device.index), C.byref(desc), d_hp.data_ptr(), T,
                                              assign.data_ptr(), status.data_ptr(), bits.data_ptr(), work.data_ptr(), blocks, int(phases),
                                              torch.cuda.current_stream(device).cuda_stream), "dz_tune_replay")
        return assign, status, bits

    SCORE_LANES = 256           # the lanes of tune_score_kernel's workgroup (backend="core" plays them in order)
    SCORE_BLOCKS = 512          # resident scoring workgroups: 256 CUs x 2 (60 KB of LDS each), one scratch slice each
    _SCORE_ERRORS = {4: "dz_tune_score: a speech turn does not start and end on the file's scoring cells",
                     3: "dz_tune_score: the mapping's assignment problem failed",
                     2: "dz_tune_score_gpu: a file has more scoring cells than a scratch slice holds"}

    @staticmethod
    def _check_scoring(scoring: Optional[str], backend: str) -> str:
        if scoring not in (None, "host", "device"):
            raise ValueError(f"scoring '{scoring}': host or device")
        if scoring == "device" and backend not in ("gpu", "core"):
            raise ValueError(f"scoring='device' runs on backend='gpu' (the scoring kernel) or backend='core' (its text on "
                             f"host threads), not on backend '{backend}'")
        return scoring or "host"

    def _score_gpu(self, bits: torch.Tensor, score_blocks: Optional[int] = None):
        """``(out (T, N, 5) float64, err (1,) int32)`` on the device of ``bits (T, rows)``: tune_score_kernel, enqueued."""
        device = bits.device
        cells = self._device(device)[2]
        T = bits.shape[0]
        blocks = max(1, min(T * self.N, int(score_blocks or self.SCORE_BLOCKS)))
        out = torch.empty((T, self.N, 5), dtype=torch.float64, device=device)
        scratch = torch.empty((blocks, self.max_cells + 1), dtype=torch.int32, device=device)
        err = torch.empty(1, dtype=torch.int32, device=device)
        _lib.check(_lib.load().dz_tune_score_gpu(_lib.context(device.index), C.byref(cells), T, bits.data_ptr(), out.data_ptr(),
                                                 scratch.data_ptr(), blocks, err.data_ptr(),
                                                 torch.cuda.current_stream(device).cuda_stream), "dz_tune_score_gpu")
        return out, err

    def _score_fetch(self, out: torch.Tensor, err: torch.Tensor) -> np.ndarray:
        per_file, rc = out.cpu().numpy(), int(err.cpu()[0])
        if rc:
            raise _lib.DiartAmdError(f"dz_tune_score_gpu failed (code {rc}): {self._SCORE_ERRORS.get(rc, 'unknown')}")
        return per_file

    def _score_core(self, bits: np.ndarray, num_threads: int, score_blocks: Optional[int] = None) -> np.ndarray:
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        T = bits.shape[0]
        out = np.zeros((T, self.N, 5), dtype=np.float64)
        _lib.check(_lib.load().dz_tune_score_core(C.byref(self._host_cells()), T, bits.ctypes.data, self.SCORE_LANES,
                                                  int(score_blocks or self.SCORE_BLOCKS), out.ctypes.data,
                                                  int(num_threads)), "dz_tune_score_core")
        return out

    def score(self, bits, num_threads: int = 8, scoring: Optional[str] = None, backend: Optional[str] = None,
              score_blocks: Optional[int] = None) -> np.ndarray:
        """``(T, N, 5)`` error-rate components (``metrics.COMPONENTS``) of the masks of ``replay``.  ``scoring``: None or
        "host" (``dz_tune_score`` on host threads) or "device": the scoring kernel on ``backend="gpu"`` (``bits`` a
        device tensor, or a numpy array that is uploaded), its text on host threads on ``backend="core"`` (the default
        without a GPU).  ``score_blocks``: the workgroups that share the pairs, each with one scratch slice."""
        if scoring == "device" and backend is None:
            backend = "gpu" if isinstance(bits, torch.Tensor) or torch.cuda.is_available() else "core"
        if self._check_scoring(scoring, backend or "host") == "host":
            if isinstance(bits, torch.Tensor):
                bits = bits.cpu().numpy().view(np.uint32)
            return self._score_bits(bits, num_threads)
        self._check_sorted("scoring 'device'", "scoring='host'")
        if backend == "core":
            if isinstance(bits, torch.Tensor):
                bits = bits.cpu().numpy().view(np.uint32)
            return self._score_core(bits, num_threads, score_blocks)
        if not torch.cuda.is_available():
            raise _lib.DiartAmdError("backend='gpu' needs a GPU; backend='core' scores with the kernel's text on the host")
        if not isinstance(bits, torch.Tensor):
            bits = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32)).to(
                torch.device("cuda", torch.cuda.current_device()))
        if bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[1] != self.total_rows or not bits.is_cuda:
            raise ValueError(f"bits (T, {self.total_rows}) int32 on a GPU expected, got {tuple(bits.shape)} {bits.dtype} on "
                             f"{bits.device}")
        return self._score_fetch(*self._score_gpu(bits.contiguous(), score_blocks))

    def evaluate(self, hparams, backend: Optional[str] = None, memory_budget: int = 1 << 30,
                 num_threads: int = 8, scoring: Optional[str] = None) -> TuneResult:
        """The error rate of every trial of ``hparams (T, 3)``, trials in batches whose results fit ``memory_budget``
        bytes (``bytes_per_trial`` each: host and device bytes with host scoring; with ``scoring="device"`` on the GPU
        backend the masks never reach the host and the budget counts device bytes — the scratch of the scoring kernel,
        ``SCORE_BLOCKS`` slices of one word per scoring cell of the largest file, does not grow with the trials and is
        not counted).  ``scoring``: None or "host": the masks are copied to the host and scored by ``dz_tune_score``;
        "device": scored where they are (``backend="gpu"``: only the components and the statuses come back;
        ``backend="core"``: the kernel's text on host threads)."""
        hp = self._hparams(hparams)
        backend = backend or self.default_backend()
        device_scoring = self._check_scoring(scoring, backend) == "device"
        if device_scoring:
            self._check_sorted("scoring 'device'", "scoring='host'")
        per_batch = max(1, int(memory_budget) // max(1, self.bytes_per_trial))
        per_file, status = [], []
        for a in range(0, hp.shape[0], per_batch):
            if device_scoring and backend == "gpu":
                _, st, bits = self._replay_gpu(hp[a:a + per_batch])
                out, err = self._score_gpu(bits)
                per_file.append(self._score_fetch(out, err))
                status.append(st.cpu().numpy())
                continue
            _, st, bits = self.replay(hp[a:a + per_batch], backend, num_threads)
            per_file.append(self._score_core(bits, num_threads) if device_scoring else self.score(bits, num_threads))
            status.append(st)
        per_file, status = np.concatenate(per_file), np.concatenate(status)
        comp = per_file.sum(axis=1)
        rate = np.where((status >= 0).any(axis=1), np.nan, _rates(comp))
        return TuneResult(rate, comp, per_file, status)

    def hypothesis(self, bits_row: np.ndarray, n: int) -> Annotation:
        """File n's hypothesis under one trial as the ``Annotation`` ``PredictionAccumulator`` ends with (tests and
        RTTM output): the speech turns of the masks, same-speaker turns closer than the patch collar merged."""
        return self._hypothesis(bits_row, n, self.G, lambda g: f"speaker{g}")


_RESERVED_LABEL = re.compile(r"speaker\d+")          # gallery.py: what unnamed speakers are called
MAX_PLANES, MAX_POINTS = 8, 256                      # tune_ident_core.h: TI_MAX_PLANES, TI_MAX_POINTS


def _check_top_ns(top_n, gallery, who: str) -> Tuple[int, ...]:
    """The planes of a normalised cache: ``(gallery.top_n,)`` for None, else 1 to 8 distinct integers under
    ``gallery.check_cohort``'s rule."""
    from .gallery import check_cohort
    if top_n is None:
        return (int(gallery.top_n),)
    values = list(np.atleast_1d(np.asarray(top_n, dtype=object)).tolist())
    if not 1 <= len(values) <= MAX_PLANES:
        raise ValueError(f"{who}: top_n= of {len(values)} values (1 .. {MAX_PLANES} planes)")
    out = tuple(check_cohort(gallery.cohort, v, gallery.dimension, who)[1] for v in values)
    if len(set(out)) != len(out):
        raise ValueError(f"{who}: top_n={list(out)} repeats a value; every plane is matched and stored once")
    return out


class SweepResult(NamedTuple):
    """``IdentTuneCache.evaluate_sweep``: entry ``[t, p, q]`` is ``evaluate``'s for clustering trial t with threshold
    ``delta_id[q]`` on the plane of ``top_n[p]``."""
    rate: np.ndarray          # (T, P, Q), NaN where a chain of the trial stopped
    components: np.ndarray    # (T, P, Q, 5)
    per_file: np.ndarray      # (T, P, Q, N, 5)
    status: np.ndarray        # (T, N)
    top_n: np.ndarray         # (P,) int64; empty for a raw cache (its one plane has no top_n)
    delta_id: np.ndarray      # (Q,)


class IdentTuneCache(TuneCache):
    """A ``TuneCache`` plus a gallery: ``delta_id`` is tuned beside ``tau_active``, ``rho_update`` and ``delta_new``.
    Three arrays are added, the same for every trial and read by every backend (two backends can never disagree about a
    distance next to ``delta_id``): ``match_index (chunks, K) int32`` and ``match_distance (chunks, K) float32``, the
    nearest voiceprint of every cached embedding row and its cosine distance (-1 / NaN for a NaN or zero row), and
    ``vp_ref (N, V) int8``, per file the bit of the reference label that equals voiceprint v's name, or -1.

    A trial's names are ``gallery.SpeakerNames(1, G, delta_id)`` run over the file's chunks on the trial's assignments:
    ``hold[c][g]`` is the voiceprint whose name global speaker g carries in step c, or -1.  The named hypothesis is
    ``TuneCache.hypothesis`` with every turn of g cut at the steps' first frame middles ``b_c`` and each piece in
    ``[b_c, b_{c+1})`` labelled ``names[hold[c][g]]``, or ``speaker{g}`` where g holds none (the first step of a file
    also owns what lies before its ``b_c``, the last what lies behind).  It is scored by
    ``metrics.IdentificationErrorRate``: labels compared as they are.  This needs the steps' grids sorted by time
    (``sorted_steps``); a cache without is refused on every backend.  A reference label of the form ``speaker<digits>``
    is refused, as the gallery refuses such names.

    A NORMALISED cache (``TuneCache.with_gallery(gallery, normalised=True, top_n=...)``, a gallery with a cohort) stores
    the cohort-normalised match instead, a signed ``dn``, once per ``top_n``: ``plane_index`` / ``plane_distance
    (P, chunks, K)``, with ``match_index`` / ``match_distance`` plane 0, and ``normalised``, ``top_ns``, ``cohort``.  Its
    thresholds are any finite value and the rule is ``SpeakerNames(..., signed=True)``.  A raw cache has one plane and
    ``top_ns == ()``.  ``evaluate_sweep`` scores every clustering trial at many (plane, threshold) points for little
    more than one replay."""

    KIND = "IdentTuneCache"
    NAME_BLOCKS = 8192          # resident naming chains: 256 CUs x 32 one-wave workgroups
    IDENT_BLOCKS = 1024         # resident ident-scoring workgroups (15 KB of LDS each), one scratch slice each
    _IDENT_ERRORS = {4: "a speech turn or a step does not lie on the file's scoring cells",
                     2: "a file has more scoring cells than a scratch slice holds"}

    def __init__(self, cache: TuneCache, gallery, device=None, match=None, top_ns: Tuple[int, ...] = ()):
        if not isinstance(cache, TuneCache):
            raise ValueError(f"IdentTuneCache takes a TuneCache, got a {type(cache).__name__}")
        if gallery.dimension != cache.D:
            raise ValueError(f"IdentTuneCache: a gallery of dimension {gallery.dimension} against cached embeddings of "
                             f"dimension {cache.D}")
        for f in cache.files:
            bad = [l for _, _, l in f["turns"] if _RESERVED_LABEL.fullmatch(str(l))]
            if bad:
                raise ValueError(f"IdentTuneCache: {f['uri']}: reference label {bad[0]!r} is what an unnamed speaker is "
                                 "called (speaker<digits>)")
        self.__dict__.update(cache.__dict__)                 # the files, the plan, the device copies: shared
        self.names = tuple(gallery.names)
        self.voiceprints = gallery.voiceprints
        self.top_ns = tuple(int(n) for n in top_ns)
        self.normalised = bool(self.top_ns)
        self.cohort = gallery.cohort if self.normalised else None
        if self.normalised and self.cohort is None:
            raise ValueError("IdentTuneCache: a normalised match (top_ns=) needs a gallery with a cohort")
        total = int(self.chunk_off[-1])
        if match is not None:
            index, distance = match
        elif not self.normalised:
            if torch.cuda.is_available():
                if device is not None:
                    gallery._resolve(device)
                index, distance, _ = gallery.match(self.emb)
            else:
                from .functional import gallery_match
                index, distance, _ = gallery_match(self.emb, gallery.voiceprints)
        else:
            index, distance = [], []
            for n in self.top_ns:                            # one device copy of the gallery at a time
                if torch.cuda.is_available():
                    g = gallery.with_cohort(self.cohort, n)
                    if device is not None:
                        g._resolve(device)
                    i, d, _ = g.match_normalised(self.emb)
                    del g
                else:
                    from .functional import gallery_match_normalised
                    i, d, _ = gallery_match_normalised(self.emb, gallery.voiceprints, self.cohort, n)
                index.append(i)
                distance.append(d)
        P = max(1, len(self.top_ns))
        self.plane_index = np.ascontiguousarray(index, dtype=np.int32).reshape(P, total, self.K)
        self.plane_distance = np.ascontiguousarray(distance, dtype=np.float32).reshape(P, total, self.K)
        self.match_index, self.match_distance = self.plane_index[0], self.plane_distance[0]     # (views: plane 0)
        V = len(self.names)
        if ((self.plane_index < -1) | (self.plane_index >= V)).any():
            raise ValueError(f"IdentTuneCache: a stored match names a voiceprint outside 0 .. {V - 1}")
        self.vp_ref = np.full((self.N, V), -1, dtype=np.int8)
        for n, labels in enumerate(self.ref_labels):
            bit = {str(l): i for i, l in enumerate(labels)}
            for v, name in enumerate(self.names):
                self.vp_ref[n, v] = bit.get(name, -1)
        # the step that owns every scoring cell: step c owns the cells from the one that starts at its first frame
        # middle to the next step's (the first step of a file everything before, the last everything behind)
        self.cell_step = np.zeros(int(self.file_cell_off[-1]), dtype=np.int32)
        if self.sorted_steps:
            for n in range(self.N):
                c0, c1 = int(self.chunk_off[n]), int(self.chunk_off[n + 1])
                first = self.mid_cell[self.row_off[c0:c1] + np.arange(c0, c1)]
                a, b = int(self.file_cell_off[n]), int(self.file_cell_off[n + 1])
                own = np.searchsorted(first, np.arange(b - a), side="right") - 1
                self.cell_step[a:b] = c0 + np.clip(own, 0, c1 - c0 - 1)
        self._ident_dev = {}

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, files, config):
        raise TypeError("IdentTuneCache: TuneCache.from_arrays(files, config).with_gallery(gallery)")

    @classmethod
    def collect(cls, pipeline_class, base_config, speech_path, reference_path, batch_size: int = 32, gallery=None,
                device=None, normalised: bool = False, top_n=None) -> "IdentTuneCache":
        if gallery is None:
            raise ValueError("IdentTuneCache.collect needs gallery= (a SpeakerGallery)")
        return TuneCache.collect(pipeline_class, base_config, speech_path, reference_path, batch_size).with_gallery(
            gallery, device, normalised=normalised, top_n=top_n)

    def save(self, path) -> None:
        """A raw cache writes the keys it always wrote; a normalised one adds its cohort, ``top_ns`` and planes (and
        keeps ``match_index`` / ``match_distance``, plane 0)."""
        out = self._payload()
        out.update(kind=np.array(self.KIND), gallery_names=np.asarray(self.names, dtype=np.str_),
                   gallery_voiceprints=self.voiceprints, match_index=self.match_index, match_distance=self.match_distance)
        if self.normalised:
            out.update(gallery_cohort=self.cohort, top_ns=np.asarray(self.top_ns, dtype=np.int64),
                       plane_index=self.plane_index, plane_distance=self.plane_distance)
        with open(path, "wb") as fh:
            np.savez(fh, **out)

    @classmethod
    def load(cls, path) -> "IdentTuneCache":
        from .gallery import SpeakerGallery
        with np.load(path, allow_pickle=False) as z:
            kind = str(z["kind"]) if "kind" in z.files else None
            if kind != cls.KIND:
                holds = "TuneCache (SpeakerDiarization)" if kind is None else kind
                raise ValueError(f"{path} holds a {holds}, not an IdentTuneCache (SpeakerDiarization with a gallery)")
            names = [str(n) for n in z["gallery_names"]]
            if "top_ns" in z.files:
                top_ns = tuple(int(n) for n in z["top_ns"])
                gallery = SpeakerGallery(names, z["gallery_voiceprints"], cohort=z["gallery_cohort"], top_n=top_ns[0])
                return cls(cls._stored(z), gallery, match=(z["plane_index"], z["plane_distance"]), top_ns=top_ns)
            gallery = SpeakerGallery(names, z["gallery_voiceprints"])
            return cls(cls._stored(z), gallery, match=(z["match_index"], z["match_distance"]))

    # ------------------------------------------------------------------------------------------ replay
    @property
    def bytes_per_trial(self) -> int:
        """``TuneCache.bytes_per_trial`` plus a trial's names: one byte per (chunk, global speaker)."""
        return self.sweep_bytes_per_trial(1)

    def sweep_bytes_per_trial(self, points: int) -> int:
        """``TuneCache.bytes_per_trial`` plus one plane of identities (``chunks * G`` bytes) per point of a sweep."""
        return TuneCache.bytes_per_trial.fget(self) + int(points) * int(self.chunk_off[-1]) * self.G

    def _check_delta(self, delta: np.ndarray, what: str) -> None:
        """Any finite threshold on a normalised cache (``dn`` is signed); a finite distance >= 0 on a raw one."""
        bad = np.flatnonzero(~np.isfinite(delta) | ((delta < 0) & (not self.normalised)))
        if bad.size:
            raise ValueError(f"{what} {int(bad[0])}: delta_id={float(delta[bad[0]])!r} "
                             f"({'a finite threshold' if self.normalised else 'a finite distance >= 0'})")

    def _hparams4(self, hparams) -> np.ndarray:
        hp = np.ascontiguousarray(np.atleast_2d(np.asarray(hparams, dtype=np.float64)))
        if hp.ndim != 2 or hp.shape[1] != 4 or hp.shape[0] < 1:
            raise ValueError(f"hparams (T, 4) = (tau_active, rho_update, delta_new, delta_id) per trial expected, got "
                             f"{hp.shape}")
        self._check_delta(hp[:, 3], "trial")
        return hp

    def _planes(self, top_n, who: str, several: bool = False) -> List[int]:
        """The planes a call names: ``top_n=None`` is plane 0 (``several``: every plane); a value (``several``: or a
        sequence of distinct values) must be among ``top_ns``."""
        if top_n is None:
            return list(range(self.plane_index.shape[0])) if several else [0]
        values = np.atleast_1d(np.asarray(top_n, dtype=object)).tolist()
        if not self.normalised:
            raise ValueError(f"{who}: top_n={top_n!r} on a raw cache, which has one plane and no top_n (top_n=None)")
        if not several and len(values) != 1:
            raise ValueError(f"{who}: top_n={top_n!r}: one plane per call (one of {list(self.top_ns)})")
        for v in values:
            if isinstance(v, bool) or v not in self.top_ns:
                raise ValueError(f"{who}: top_n={v!r} is no plane of this cache (top_ns = {list(self.top_ns)})")
        if not 1 <= len(values) <= MAX_PLANES or len(set(values)) != len(values):
            raise ValueError(f"{who}: top_n={top_n!r}: 1 .. {MAX_PLANES} distinct planes")
        return [self.top_ns.index(v) for v in values]

    def delta_range(self) -> Tuple[float, float]:
        """The lowest and the highest finite stored distance over all planes of a normalised cache: a threshold
        outside changes no name.  A raw cache answers ``DeltaId``'s range."""
        if not self.normalised:
            return float(base.DeltaId.low), float(base.DeltaId.high)
        d = self.plane_distance[np.isfinite(self.plane_distance)]
        if d.size == 0:
            raise ValueError("IdentTuneCache.delta_range: no stored distance is finite")
        return float(d.min()), float(d.max())

    def _check_steps(self) -> None:
        if not self.sorted_steps:
            raise ValueError("IdentTuneCache: a step owns the time from its first output frame to the next step's, and the "
                             "output grids of this cache's steps are not sorted by time")

    def _ident_device(self, device: torch.device):
        """``(tensors, cells)``: what this cache adds to the TuneCache's device copies, and the TuneCache's descriptor of
        the scoring geometry with ``cell_step`` in it."""
        key = str(device)
        if key not in self._ident_dev:
            tensors = {name: torch.from_numpy(getattr(self, name)).to(device)
                       for name in ("plane_index", "plane_distance", "vp_ref", "cell_step")}
            cells = _lib.TuneCells.from_buffer_copy(self._device(device)[2])
            cells.cell_step = tensors["cell_step"].data_ptr()
            self._ident_dev[key] = (tensors, cells)
        return self._ident_dev[key]

    @staticmethod
    def _take_planes(index, distance, planes: List[int]):
        """``(planes, chunks, K)`` contiguous: the whole store, one plane of it in place, or a gathered copy."""
        if planes == list(range(index.shape[0])):
            return index, distance
        if len(planes) == 1:
            return index[planes[0]:planes[0] + 1], distance[planes[0]:planes[0] + 1]
        if isinstance(index, torch.Tensor):
            sel = torch.as_tensor(planes, device=index.device)
            return index.index_select(0, sel).contiguous(), distance.index_select(0, sel).contiguous()
        return np.ascontiguousarray(index[planes]), np.ascontiguousarray(distance[planes])

    def _names_gpu(self, assign: torch.Tensor, status: torch.Tensor, delta_id: np.ndarray, want_hold: bool = False,
                   planes: Sequence[int] = (0,)):
        """``(ident, hold or None)`` on the device: tune_name_kernel, enqueued.  ``delta_id (T,)``: one point on
        ``planes[0]`` -> ``(T, chunks, G)`` int8 / int32.  ``delta_id (T, J)``: the sweep, J points plane-major over
        ``planes`` -> ``(T, J, chunks, G)``."""
        device = assign.device
        t, i = self._device(device)[0], self._ident_device(device)[0]
        T, total = assign.shape[0], int(self.chunk_off[-1])
        delta_id = np.ascontiguousarray(delta_id, dtype=np.float64)
        d_delta = torch.from_numpy(delta_id).to(device)
        shape = (T,) + delta_id.shape[1:] + (total, self.G)
        ident = torch.empty(shape, dtype=torch.int8, device=device)
        hold = torch.empty(shape, dtype=torch.int32, device=device) if want_hold else None
        index, distance = self._take_planes(i["plane_index"], i["plane_distance"], list(planes))
        _lib.check(_lib.load().dz_tune_name(
            _lib.context(device.index), T, delta_id.size // T, len(planes), self.N, total, self.K, self.G, len(self.names),
            t["chunk_off"].data_ptr(), assign.data_ptr(), status.data_ptr(), index.data_ptr(), distance.data_ptr(),
            i["vp_ref"].data_ptr(), d_delta.data_ptr(), ident.data_ptr(), None if hold is None else hold.data_ptr(),
            self.NAME_BLOCKS, torch.cuda.current_stream(device).cuda_stream), "dz_tune_name")
        return ident, hold

    def _names_host(self, assign: np.ndarray, status: np.ndarray, delta_id: np.ndarray, want_hold: bool, num_threads: int,
                    planes: Sequence[int] = (0,)):
        """``_names_gpu`` on host threads: ``dz_tune_name_host``."""
        T, total = assign.shape[0], int(self.chunk_off[-1])
        delta_id = np.ascontiguousarray(delta_id, dtype=np.float64)
        shape = (T,) + delta_id.shape[1:] + (total, self.G)
        ident = np.empty(shape, dtype=np.int8)
        hold = np.empty(shape, dtype=np.int32) if want_hold else None
        index, distance = self._take_planes(self.plane_index, self.plane_distance, list(planes))
        _lib.check(_lib.load().dz_tune_name_host(
            T, delta_id.size // T, len(planes), self.N, total, self.K, self.G, len(self.names), self.chunk_off.ctypes.data,
            assign.ctypes.data, status.ctypes.data, index.ctypes.data, distance.ctypes.data, self.vp_ref.ctypes.data,
            delta_id.ctypes.data, ident.ctypes.data, None if hold is None else hold.ctypes.data, int(num_threads)),
            "dz_tune_name_host")
        return ident, hold

    def replay_names(self, hparams, backend: Optional[str] = None, num_threads: int = 8, top_n=None):
        """``(assign, status, bits, hold (T, chunks, G) int32)``: ``TuneCache.replay`` of the first three columns of
        ``hparams (T, 4)``, and the voiceprint whose name every global speaker carries in every step under the
        trial's ``delta_id`` (-1: none) on the plane of ``top_n`` (None: plane 0).  ``backend``: "gpu" | "host" |
        "core"; the naming rule has one text, which "host" and "core" both run on host threads."""
        hp = self._hparams4(hparams)
        planes = self._planes(top_n, "IdentTuneCache.replay_names")
        backend = backend or self.default_backend()
        if backend == "gpu":
            a, s, b = self._replay_gpu(np.ascontiguousarray(hp[:, :3]))
            _, hold = self._names_gpu(a, s, hp[:, 3], want_hold=True, planes=planes)
            torch.cuda.synchronize(a.device)
            return a.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy().view(np.uint32), hold.cpu().numpy()
        a, s, b = TuneCache.replay(self, hp[:, :3], backend, num_threads)
        return a, s, b, self._names_host(a, s, hp[:, 3], True, num_threads, planes)[1]

    def _ident_score_gpu(self, bits: torch.Tensor, ident: torch.Tensor):
        """``(out, err)`` on the device: tune_ident_score_kernel, enqueued.  ``ident (T, chunks, G)`` -> ``out
        (T, N, 5)``; ``ident (T, J, chunks, G)``, the sweep -> ``out (T, J, N, 5)``."""
        device = bits.device
        cells = self._ident_device(device)[1]
        T = bits.shape[0]
        blocks = max(1, min(T * self.N, self.IDENT_BLOCKS))
        out = torch.empty(tuple(ident.shape[:-2]) + (self.N, 5), dtype=torch.float64, device=device)
        scratch = torch.empty((blocks, self.max_cells + 1), dtype=torch.int32, device=device)
        err = torch.empty(1, dtype=torch.int32, device=device)
        _lib.check(_lib.load().dz_tune_ident_score_gpu(
            _lib.context(device.index), C.byref(cells), T, self._points(ident), bits.data_ptr(), ident.data_ptr(),
            out.data_ptr(), scratch.data_ptr(), blocks, err.data_ptr(), torch.cuda.current_stream(device).cuda_stream),
            "dz_tune_ident_score_gpu")
        return out, err

    @staticmethod
    def _points(ident) -> int:
        """The points of ``ident (T, chunks, G)`` (one) or ``(T, J, chunks, G)``."""
        return 1 if len(ident.shape) == 3 else int(ident.shape[1])

    def _ident_score_host(self, bits: np.ndarray, ident: np.ndarray, core: bool, num_threads: int) -> np.ndarray:
        """``_ident_score_gpu`` on host threads.  ``core``: the kernel's text (``ident`` of one point or of a sweep);
        else ``dz_tune_ident_score``, the sequential text, one point."""
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        T = bits.shape[0]
        out = np.zeros(ident.shape[:-2] + (self.N, 5), dtype=np.float64)
        lib, cells = _lib.load(), C.byref(self._host_cells())
        if core:
            _lib.check(lib.dz_tune_ident_score_core(cells, T, self._points(ident), bits.ctypes.data, ident.ctypes.data,
                                                    self.SCORE_LANES, self.IDENT_BLOCKS, out.ctypes.data, int(num_threads)),
                       "dz_tune_ident_score_core")
        else:
            _lib.check(lib.dz_tune_ident_score(cells, T, bits.ctypes.data, ident.ctypes.data, out.ctypes.data,
                                               int(num_threads)), "dz_tune_ident_score")
        return out

    def _ident_fetch(self, out: torch.Tensor, err: torch.Tensor) -> np.ndarray:
        rc = int(err.cpu()[0])
        if rc:
            raise _lib.DiartAmdError(f"dz_tune_ident_score_gpu failed (code {rc}): {self._IDENT_ERRORS.get(rc, 'unknown')}")
        return out.cpu().numpy()

    def evaluate(self, hparams, backend: Optional[str] = None, memory_budget: int = 1 << 30,
                 num_threads: int = 8, top_n=None) -> TuneResult:
        """The identification error rate of every trial of ``hparams (T, 4)`` = (tau_active, rho_update, delta_new,
        delta_id), trials in batches whose results fit ``memory_budget`` bytes (``bytes_per_trial`` each).  Scored
        where it is replayed: ``backend="gpu"`` leaves ``T x N x 5`` doubles and the statuses; "host": the clustering
        and the tail through their handles, the names and the score on host threads; "core": the kernels' text on host
        threads.  A trial whose chain stopped has rate NaN.  ``top_n``: the plane of a normalised cache that the call
        is matched on (None: plane 0)."""
        hp = self._hparams4(hparams)
        planes = self._planes(top_n, "IdentTuneCache.evaluate")
        backend = backend or self.default_backend()
        if backend not in ("gpu", "host", "core"):
            raise ValueError(f"backend '{backend}': gpu, host or core")
        self._check_steps()
        per_batch = max(1, int(memory_budget) // max(1, self.bytes_per_trial))
        per_file, status = [], []
        for a in range(0, hp.shape[0], per_batch):
            h3, delta = np.ascontiguousarray(hp[a:a + per_batch, :3]), hp[a:a + per_batch, 3]
            if backend == "gpu":
                assign, st, bits = self._replay_gpu(h3)
                ident, _ = self._names_gpu(assign, st, delta, planes=planes)
                per_file.append(self._ident_fetch(*self._ident_score_gpu(bits, ident)))
                status.append(st.cpu().numpy())
                continue
            assign, st, bits = TuneCache.replay(self, h3, backend, num_threads)
            ident, _ = self._names_host(assign, st, delta, False, num_threads, planes)
            per_file.append(self._ident_score_host(bits, ident, backend == "core", num_threads))
            status.append(st)
        per_file, status = np.concatenate(per_file), np.concatenate(status)
        comp = per_file.sum(axis=1)
        rate = np.where((status >= 0).any(axis=1), np.nan, _rates(comp))
        return TuneResult(rate, comp, per_file, status)

    def _sweep_args(self, hparams, delta_id, top_n, who: str):
        hp = self._hparams(hparams)
        delta = np.ascontiguousarray(np.atleast_1d(np.asarray(delta_id, dtype=np.float64)))
        if delta.ndim != 1:
            raise ValueError(f"{who}: delta_id (Q,) thresholds expected, got {delta.shape}")
        if top_n is not None and not self.normalised:
            raise ValueError(f"{who}: top_n={top_n!r} on a raw cache, which has one plane and no top_n (top_n=None)")
        planes = self._planes(top_n, who, several=True)
        points = len(planes) * delta.shape[0]
        if not 1 <= points <= MAX_POINTS:
            raise ValueError(f"{who}: {len(planes)} planes x {delta.shape[0]} thresholds = {points} points (1 .. {MAX_POINTS})")
        self._check_delta(delta, "point")
        return hp, delta, planes

    def replay_names_sweep(self, hparams, delta_id, top_n=None, backend: Optional[str] = None, num_threads: int = 8):
        """``(assign, status, bits, hold (T, P, Q, chunks, G) int32)``: ``replay_names`` of every clustering trial of
        ``hparams (T, 3)`` at every point of ``evaluate_sweep``."""
        hp, delta, planes = self._sweep_args(hparams, delta_id, top_n, "IdentTuneCache.replay_names_sweep")
        backend = backend or self.default_backend()
        T, P, Q = hp.shape[0], len(planes), delta.shape[0]
        thr = np.tile(delta, (T, P))                           # (T, P * Q): plane-major, the same for every trial
        shape = (T, P, Q, int(self.chunk_off[-1]), self.G)
        if backend == "gpu":
            a, s, b = self._replay_gpu(hp)
            _, hold = self._names_gpu(a, s, thr, want_hold=True, planes=planes)
            torch.cuda.synchronize(a.device)
            return a.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy().view(np.uint32), hold.cpu().numpy().reshape(shape)
        a, s, b = TuneCache.replay(self, hp, backend, num_threads)
        if backend == "core":
            return a, s, b, self._names_host(a, s, thr, True, num_threads, planes)[1].reshape(shape)
        hold = np.empty(shape, dtype=np.int32)
        for p, plane in enumerate(planes):
            for q in range(Q):
                hold[:, p, q] = self._names_host(a, s, np.full(T, delta[q]), True, num_threads, [plane])[1]
        return a, s, b, hold

    def evaluate_sweep(self, hparams, delta_id, top_n=None, backend: Optional[str] = None, memory_budget: int = 1 << 30,
                       num_threads: int = 8) -> SweepResult:
        """Every clustering trial of ``hparams (T, 3)`` = (tau_active, rho_update, delta_new) scored at every point of
        ``top_n (P,)`` x ``delta_id (Q,)``: entry ``[t, p, q]`` of every array is what ``evaluate`` returns for the
        trial ``hparams[t] + [delta_id[q]]`` on the plane of ``top_n[p]``.  The names depend on the clustering through
        its assignments only and the scoring cells on its masks only, so a trial is replayed ONCE: the naming kernel
        walks one chain per (trial, point, file), the scoring kernel builds a pair's cells once and adds every point's
        components from them.  ``top_n=None``: every plane of the cache (a raw cache has one and
        takes None only).  ``P * Q``: 1 .. 256 points, plane-major.  ``backend``: "gpu" and "core" run that text;
        "host" is the loop over the points of ``dz_tune_name_host`` and ``dz_tune_ident_score``, the yardstick.
        A trial's results take ``sweep_bytes_per_trial(P * Q)`` bytes, most of them identities; ``memory_budget`` is
        split: three quarters hold the replays' results of a batch of trials, one quarter the identities of a slice of
        that batch.  No result depends on the batches."""
        who = "IdentTuneCache.evaluate_sweep"
        hp, delta, planes = self._sweep_args(hparams, delta_id, top_n, who)
        backend = backend or self.default_backend()
        if backend not in ("gpu", "host", "core"):
            raise ValueError(f"backend '{backend}': gpu, host or core")
        self._check_steps()
        P, Q = len(planes), delta.shape[0]
        # Two levels of batches.  The clustering replay is latency-bound (a batch of 64 trials costs little more than a
        # batch of one), and the identities of a sweep are by far the largest result: so three quarters of the budget
        # go to the replays' results, in batches as large as they allow, and one quarter to the identities, which are
        # named and scored in slices of each replayed batch.
        J = P * Q
        per_batch = max(1, (3 * int(memory_budget) // 4) // max(1, TuneCache.bytes_per_trial.fget(self)))
        per_slice = max(1, (int(memory_budget) // 4) // max(1, J * int(self.chunk_off[-1]) * self.G))
        per_file, status = [], []
        for a in range(0, hp.shape[0], per_batch):
            h3 = np.ascontiguousarray(hp[a:a + per_batch])
            T = h3.shape[0]
            thr = np.tile(delta, (min(T, per_slice), P))           # (slice, P * Q): plane-major, the same for every trial
            slices = [slice(b, min(b + per_slice, T)) for b in range(0, T, per_slice)]
            if backend == "gpu":
                assign, st, bits = self._replay_gpu(h3)
                outs = []
                for sl in slices:
                    ident, _ = self._names_gpu(assign[sl], st[sl], thr[:sl.stop - sl.start], planes=planes)
                    outs.append(self._ident_score_gpu(bits[sl], ident))
                    del ident
                per_file += [self._ident_fetch(out, err) for out, err in outs]
                status.append(st.cpu().numpy())
                continue
            assign, st, bits = TuneCache.replay(self, h3, backend, num_threads)
            for sl in slices:
                n = sl.stop - sl.start
                if backend == "core":
                    ident, _ = self._names_host(assign[sl], st[sl], thr[:n], False, num_threads, planes)
                    per_file.append(self._ident_score_host(bits[sl], ident, True, num_threads))
                    continue
                out = np.empty((n, J, self.N, 5), dtype=np.float64)
                for j in range(J):
                    ident, _ = self._names_host(assign[sl], st[sl], thr[:n, j], False, num_threads, [planes[j // Q]])
                    out[:, j] = self._ident_score_host(bits[sl], ident, False, num_threads)
                per_file.append(out)
            status.append(st)
        per_file, status = np.concatenate(per_file), np.concatenate(status)
        per_file = per_file.reshape(hp.shape[0], P, Q, self.N, 5)
        comp = per_file.sum(axis=3)
        rate = np.where((status >= 0).any(axis=1)[:, None, None], np.nan, _rates(comp.reshape(-1, 5)).reshape(comp.shape[:3]))
        tops = np.asarray([self.top_ns[p] for p in planes] if self.normalised else [], dtype=np.int64)
        return SweepResult(rate, comp, per_file, status, tops, delta)

    def score(self, *args, **kw):
        raise TypeError("IdentTuneCache scores names, not an optimal mapping: evaluate(hparams (T, 4)); the diarization "
                        "error rate of the same outputs is the TuneCache's it was made from")

    def hypothesis(self, bits_row: np.ndarray, hold_row: np.ndarray, n: int) -> Annotation:
        """File n's NAMED hypothesis under one trial (``bits_row``, ``hold_row (chunks, G)`` of ``replay_names``): the
        turns of ``TuneCache.hypothesis`` cut at the steps' first frame middles, every piece labelled with the name its
        speaker carries in the step that owns it, or ``speaker{g}``."""
        self._check_steps()
        c0, c1 = int(self.chunk_off[n]), int(self.chunk_off[n + 1])
        b = self.mids[self.row_off[c0:c1] + np.arange(c0, c1)]
        ann = Annotation(uri=self.files[n]["uri"], modality="speech")
        for i, (seg, _, label) in enumerate(TuneCache.hypothesis(self, bits_row, n).itertracks(yield_label=True)):
            g = int(label[len("speaker"):])
            cuts = [seg.start] + [float(x) for x in b[1:] if seg.start < x < seg.end] + [seg.end]
            for j, (s, e) in enumerate(zip(cuts[:-1], cuts[1:])):
                c = min(max(int(np.searchsorted(b, s, side="right")) - 1, 0), c1 - c0 - 1)
                v = int(hold_row[c0 + c][g])
                ann[Segment(s, e), f"{i}_{j}"] = self.names[v] if v >= 0 else label
        return ann


class _TrackTuneCache(_ReplayCache):
    """What ``VadTuneCache`` and ``OsdTuneCache`` share, which is everything behind the track: per file a track
    ``(C, F)`` (what ``finalise`` aggregates), the window starts, the frame resolution, the shift and a reference; the
    meta fields ``step``, ``latency`` and ``tau_active``.  A scoring cell has one reference bit.  The aggregated score of
    every packed output frame (``agg``) does not depend on ``tau_active``; it is computed once per cache (and once per
    device), a trial compares it with its tau.  A subclass names its pipeline (``KIND``, ``REPLAY``, ``PIPELINE``,
    ``LABEL``), says which turns of a reference are stored and which build the scoring cells (``_reference``), and
    what a file of another kind is told (``_check_kind``)."""

    SCORE_LANES = 256           # the lanes of tune_vad_score_kernel's workgroup (backend="core" plays them in order)
    KIND = REPLAY = PIPELINE = LABEL = ELSEWHERE = None

    def __init__(self, files: Sequence[dict], config):
        get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
        self.meta = {k: float(get(k)) for k in ("step", "latency", "tau_active")}
        name = type(self).__name__
        if not files:
            raise ValueError(f"{name} needs at least one file")
        self.files = []
        for i, f in enumerate(files):
            track = np.ascontiguousarray(f["track"], dtype=np.float32)
            if track.ndim == 3 and track.shape[2] == 1:
                track = np.ascontiguousarray(track[:, :, 0])
            starts = np.ascontiguousarray(f["starts"], dtype=np.float64)
            C_ = track.shape[0]
            if track.ndim != 2 or starts.shape != (C_,) or C_ < 1 or track.shape[1] < 1:
                raise ValueError(f"file {i}: track (C, F), starts (C) expected, got {track.shape}, {starts.shape}")
            res = np.ascontiguousarray(np.broadcast_to(np.asarray(f["res"], dtype=np.float64), (C_,)))
            stored, turns = self._reference(f["reference"])
            self.files.append(dict(uri=str(f.get("uri", f"file{i}")), track=track, starts=starts, res=res,
                                   shift=float(f.get("shift", 0.0)), stored=stored, turns=turns))
        frames = {f["track"].shape[1] for f in self.files}
        if len(frames) != 1:
            raise ValueError(f"the files of one cache share the frames per chunk, got {sorted(frames)}")
        self.F, self.N = next(iter(frames)), len(self.files)
        self._prepare()
        self._dev = {}
        self._agg = None

    @staticmethod
    def _reference(reference):
        """``(stored, turns)``: the turns ``save`` writes (``load`` hands them back as the reference) and the turns whose
        boundaries and activity make the scoring cells."""
        raise NotImplementedError

    @classmethod
    def _check_kind(cls, path, kind: Optional[str]) -> None:
        """Raise the ValueError of a file whose kind tag (None: no tag, a ``TuneCache``) is not this class's."""
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, files: Sequence[dict], config):
        """``files``: dicts with ``track (C, F)`` (or ``(C, F, 1)``), ``starts (C)``, ``res``, ``shift``, ``reference``
        and optionally ``uri``, as ``TuneCache.from_arrays`` takes them.  ``config``: anything with ``step``,
        ``latency`` and ``tau_active`` (attributes or keys)."""
        return cls(files, config)

    @classmethod
    def _from_scores(cls, cache: "TuneCache", tau_active: Optional[float], track):
        """A collected ``TuneCache`` as this class's cache: ``track(scores)`` turns a file's raw segmentation scores
        ``(C, F, K)`` (a float32 tensor) into the track ``(C, F)`` or ``(C, F, 1)``; the starts, the resolutions, the
        shift and the reference turns are the diarization cache's own."""
        if not isinstance(cache, TuneCache):
            raise ValueError(f"{cls.__name__}.from_tune_cache takes a TuneCache, got a {type(cache).__name__}")
        files = [dict(uri=f["uri"], track=track(torch.from_numpy(f["seg"])).cpu().numpy(), starts=f["starts"], res=f["res"],
                      shift=f["shift"], reference=f["turns"]) for f in cache.files]
        tau = cache.meta["tau_active"] if tau_active is None else float(tau_active)
        return cls(files, dict(step=cache.meta["step"], latency=cache.meta["latency"], tau_active=tau))

    @classmethod
    def collect(cls, pipeline_class, base_config, speech_path, reference_path, batch_size: int = 32):
        """Run the model half of the class's pipeline (``model_outputs``) once per WAV of ``speech_path``."""
        if _replay_kind(pipeline_class) != cls.REPLAY:
            raise ValueError(f"pipeline class {pipeline_class.__name__}: {cls.KIND} collects {cls.PIPELINE}; "
                             f"{cls.ELSEWHERE}")
        pipeline = pipeline_class(base_config)
        files = cls._collect_files(pipeline, speech_path, reference_path, batch_size,
                                   lambda batch: (pipeline.model_outputs(batch).detach().cpu().numpy()
                                                  .astype(np.float32, copy=False),))
        for f in files:
            f["track"] = f.pop("outputs")[0]
        return cls(files, pipeline.config)

    def save(self, path) -> None:
        out = {"kind": np.array(self.KIND), "meta": np.array(json.dumps(self.meta)),
               "uris": np.array([f["uri"] for f in self.files])}
        for i, f in enumerate(self.files):
            for k in ("track", "starts", "res"):
                out[f"{k}_{i}"] = f[k]
            out[f"shift_{i}"] = np.array(f["shift"])
            out[f"ref_times_{i}"] = np.array([[s, e] for s, e, _ in f["stored"]], dtype=np.float64).reshape(-1, 2)
            out[f"ref_labels_{i}"] = np.array([str(l) for _, _, l in f["stored"]], dtype=str)
        with open(path, "wb") as fh:
            np.savez(fh, **out)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            kind = str(z["kind"]) if "kind" in z.files else None
            if kind != cls.KIND:
                cls._check_kind(path, kind)
            meta = json.loads(str(z["meta"]))
            files = []
            for i, uri in enumerate(z["uris"]):
                ref = [(s, e, str(l)) for (s, e), l in zip(z[f"ref_times_{i}"], z[f"ref_labels_{i}"])]
                files.append(dict(uri=str(uri), track=z[f"track_{i}"], starts=z[f"starts_{i}"], res=z[f"res_{i}"],
                                  shift=float(z[f"shift_{i}"]), reference=ref))
        return cls(files, meta)

    # ------------------------------------------------------------------------------------------ trial-independent parts
    def _reference_bits(self, f: dict) -> Dict[object, int]:
        self.ref_labels.append([self.LABEL] if f["turns"] else [])
        return {l: 0 for _, _, l in f["turns"]}

    def _prepare(self) -> None:
        self._prepare_plan()
        self.seg = np.concatenate([f["track"] for f in self.files])                 # (chunks, F): one local speaker
        # prefix sums of the cells' durations, and of the durations where the reference is active: cells + 1 per file
        dur, ref = [], []
        for n in range(self.N):
            a, b = int(self.file_cell_off[n]), int(self.file_cell_off[n + 1])
            d = self.cell_dur[a:b]
            dur.append(np.concatenate([[0.0], np.cumsum(d)]))
            ref.append(np.concatenate([[0.0], np.cumsum(np.where(self.cell_ref[a:b] != 0, d, 0.0))]))
        self.dur_prefix = np.ascontiguousarray(np.concatenate(dur), dtype=np.float64)
        self.ref_prefix = np.ascontiguousarray(np.concatenate(ref), dtype=np.float64)

    def _desc(self, ptr) -> _lib.TuneDesc:
        d = _lib.TuneDesc()
        for name in ("seg", "chunk_off", "plan", "row_off", "row_chunk", "hamming"):
            setattr(d, name, ptr(name))
        d.N, d.F, d.K, d.D, d.G, d.nwin = self.N, self.F, 1, 1, 1, self.nwin
        d.total_chunks, d.total_rows = int(self.chunk_off[-1]), self.total_rows
        return d

    @property
    def bytes_per_trial(self) -> int:
        """Host memory one trial's masks take (backend="host"); the GPU backend keeps 40 bytes per (trial, file)."""
        return 4 * self.total_rows

    # ------------------------------------------------------------------------------------------ replay
    SHAPES = ("(T,) or (T, 1) = tau_active per trial, (T, 2) = (tau_active, tau_offset) per trial or (T, 4) = "
              "(tau_active, tau_offset, min_duration_on, min_duration_off) per trial")

    @classmethod
    def _taus(cls, taus) -> np.ndarray:
        """``(T,)`` — ``(T, 1)`` too — = tau_active per trial: the single threshold, today's kernels.  ``(T, 2)`` =
        (tau_active, tau_offset) per trial: hysteresis, and the array stays two-dimensional.  ``(T, 4)`` = (tau_active,
        tau_offset, min_duration_on, min_duration_off): the minimum durations (seconds) on the hysteresis rows; a trial
        without hysteresis passes tau_offset == tau_active."""
        try:
            t = np.asarray(taus, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"taus {cls.SHAPES} expected: numbers") from None
        if t.ndim == 2 and t.shape[1] == 1:
            t = t[:, 0]
        if t.ndim == 2 and t.shape[1] == 2 and t.shape[0] >= 1:
            if not np.isfinite(t[:, 1]).all():
                raise ValueError("taus (T, 2): tau_offset must be finite in every trial")
            return np.ascontiguousarray(t)
        if t.ndim == 2 and t.shape[1] == 4 and t.shape[0] >= 1:
            if not np.isfinite(t[:, 1]).all():
                raise ValueError("taus (T, 4): tau_offset must be finite in every trial")
            for k, name in ((2, "min_duration_on"), (3, "min_duration_off")):
                bad = np.flatnonzero(~(np.isfinite(t[:, k]) & (t[:, k] >= 0)))
                if len(bad):
                    raise ValueError(f"taus (T, 4): {name} of trial {int(bad[0])} is {t[bad[0], k]}: a duration is a "
                                     "finite number >= 0")
            return np.ascontiguousarray(t)
        if t.ndim != 1 or t.shape[0] < 1:
            raise ValueError(f"taus {cls.SHAPES} expected, got {np.shape(taus)}")
        return np.ascontiguousarray(t)

    def _host(self, taus: np.ndarray, bits: bool, components: bool, num_threads: int, core: bool = True):
        """``(agg, bits, components)`` on host threads, from the kernels' text: ``dz_tune_vad_host`` under the rule of
        the columns of ``taus`` — ``(T,)``; ``(T, 2)``, the lanes' state maps included; ``(T, 4)``, the lanes' span
        summaries too.  ``core=False`` with ``(T, 2)`` or ``(T, 4)`` (backend="host"):
        the masks come from an independent text instead — one ``dz_tail`` handle with ``dz_tail_set_offset`` per (trial,
        file), fed the track step by step, which reads the first two columns — and there are no components."""
        T = taus.shape[0]
        tails = taus.ndim == 2 and not core
        assert not (tails and components)
        pairs = np.ascontiguousarray(taus[:, :2]) if tails else None
        agg = np.empty(self.total_rows, dtype=np.float64)
        b = np.empty((T, self.total_rows), dtype=np.uint32) if bits else None
        out = np.zeros((T, self.N, 5), dtype=np.float64) if components else None
        d = self._desc(lambda name: getattr(self, name).ctypes.data)
        ptr = lambda a: None if a is None else a.ctypes.data
        lib = _lib.load()
        thresholds = np.ascontiguousarray(taus[:, 0]) if tails else taus          # (the aggregation reads none of them)
        _lib.check(lib.dz_tune_vad_host(C.byref(d), C.byref(self._host_cells()), thresholds.size // T, thresholds.ctypes.data,
                                        T, agg.ctypes.data, None if tails else ptr(b), self.SCORE_LANES, ptr(out),
                                        int(num_threads)), "dz_tune_vad_host")
        if tails and bits:
            starts = np.ascontiguousarray(self.starts, dtype=np.float64)
            res = np.ascontiguousarray(self.res, dtype=np.float64)
            _lib.check(lib.dz_tune_vad_replay_tails(C.byref(d), pairs.ctypes.data, T, self.meta["step"], self.meta["latency"],
                                                    starts.ctypes.data, res.ctypes.data, b.ctypes.data, int(num_threads)),
                       "dz_tune_vad_replay_tails")
        return agg, b, out

    def _device(self, device: torch.device):
        """The cache's device tensors, ``agg`` among them: tune_vad_rows_kernel runs once per cache and device."""
        key = str(device)
        if key not in self._dev:
            tensors = {name: torch.from_numpy(getattr(self, name)).to(device)
                       for name in ("seg", "chunk_off", "plan", "row_off", "row_chunk", "hamming", "mids", "mid_cell",
                                    "file_cell_off", "dur_prefix", "ref_prefix")}
            tensors["agg"] = torch.empty(self.total_rows, dtype=torch.float64, device=device)
            ptr = lambda name: tensors[name].data_ptr() if name in tensors else None
            desc = self._desc(ptr)
            _lib.check(_lib.load().dz_tune_vad_rows(_lib.context(device.index), C.byref(desc), tensors["agg"].data_ptr(),
                                                    torch.cuda.current_stream(device).cuda_stream), "dz_tune_vad_rows")
            self._dev[key] = (tensors, desc, self._cells(ptr))
        return self._dev[key]

    def _gpu(self, taus: np.ndarray, bits: bool, components: bool, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise _lib.DiartAmdError("backend='gpu' needs a GPU; backend='host' replays on the host")
        device = device or torch.device("cuda", torch.cuda.current_device())
        t, _, cells = self._device(device)
        T = taus.shape[0]
        d_taus = torch.from_numpy(taus).to(device)
        b = torch.empty((T, self.total_rows), dtype=torch.int32, device=device) if bits else None
        out = torch.empty((T, self.N, 5), dtype=torch.float64, device=device) if components else None
        ptr = lambda a: None if a is None else a.data_ptr()
        # the columns select the instantiation of tune_vad_score_kernel; (T, 4) is checked in host memory too (the other
        # rules take no host pointer: `ndarray.ctypes` costs a microsecond between the upload and the launch)
        cols = taus.size // T
        _lib.check(_lib.load().dz_tune_vad_score(_lib.context(device.index), C.byref(cells), cols, T, t["agg"].data_ptr(),
                                                 taus.ctypes.data if cols == 4 else None, d_taus.data_ptr(), ptr(out), ptr(b),
                                                 torch.cuda.current_stream(device).cuda_stream), "dz_tune_vad_score")
        return t["agg"], b, out

    def replay(self, taus, backend: Optional[str] = None, num_threads: int = 8):
        """``(agg (rows,) float64, bits (T, rows) uint32)``: the aggregated speech score of every packed output frame
        and, per trial, whether it is above the trial's tau.  ``backend``: "gpu" | "host".  ``taus (T, 2)`` =
        (tau_active, tau_offset): whether the frame is on under the hysteresis rule, the state off at every file's first
        frame; then "core" too, the kernel's text on host threads ("host" goes through ``dz_tail_set_offset``).
        ``taus (T, 4)`` = (tau_active, tau_offset, min_duration_on, min_duration_off): the masks BEFORE the durations
        act, which are the ``(T, 2)`` masks of the first two columns — a mask says which frames are on, and a gap that
        ``min_duration_off`` fills lies between two steps' rows as often as inside one: a filled gap is not a row, and
        a dropped turn keeps its rows.  ``hypothesis(bits_row, n, min_duration_on, min_duration_off)`` applies them."""
        taus = self._taus(taus)
        backend = backend or self.default_backend()
        hyst = taus.ndim == 2
        if backend == "gpu":
            agg, bits, _ = self._gpu(taus, True, False)
            torch.cuda.synchronize(agg.device)
            return agg.cpu().numpy(), bits.cpu().numpy().view(np.uint32)
        if backend != "host" and not (hyst and backend == "core"):
            raise ValueError(f"backend '{backend}': gpu or host" + (" or core" if hyst else ""))
        agg, bits, _ = self._host(taus, True, False, num_threads, core=backend == "core")
        return agg, bits

    def score(self, bits: np.ndarray, num_threads: int = 8) -> np.ndarray:
        """``(T, N, 5)`` detection error rate components of the masks of ``replay``, by ``dz_tune_score`` with one
        hypothesis speaker on the collapsed reference cells."""
        return self._score_bits(bits, num_threads)

    def evaluate(self, taus, backend: Optional[str] = None, memory_budget: int = 1 << 30,
                 num_threads: int = 8) -> TuneResult:
        """The detection error rate of every trial of ``taus``.  ``backend``: "gpu" (the two kernels; only the
        components come back), "host" (the same aggregation on host threads, then ``dz_tune_score``; trials in batches
        whose masks fit ``memory_budget`` bytes) or "core" (the scoring kernel's text on host threads).  ``taus (T, 2)``
        = (tau_active, tau_offset) per trial: hysteresis — "gpu" runs ``tune_vad_score_kernel`` under the stateful rule,
        "core" its text, "host" one ``dz_tail`` handle with ``dz_tail_set_offset`` per (trial, file), then
        ``dz_tune_score``.  ``(T,)`` is the same pair routine under the stateless rule.  ``taus (T, 4)`` = (tau_active,
        tau_offset, min_duration_on, min_duration_off): the file's turns merged with the collar ``max(PATCH_COLLAR,
        min_duration_off)``, then the merged turns shorter than ``min_duration_on`` dropped
        (``functional.min_duration``) — "gpu" runs the pair routine's third instantiation, "core" its text, "host" the
        ``dz_tail`` masks and then ``dz_tune_track_score_dur``, one sequential walk per (trial, file)."""
        taus = self._taus(taus)
        backend = backend or self.default_backend()
        if backend == "gpu":
            self._check_sorted(f"backend '{backend}'")
            out = self._gpu(taus, False, True)[2]
            per_file = out.cpu().numpy()
        elif backend == "core":
            self._check_sorted(f"backend '{backend}'")
            per_file = self._host(taus, False, True, num_threads)[2]
        elif backend == "host":
            per_batch = max(1, int(memory_budget) // max(1, self.bytes_per_trial))
            durations = taus.ndim == 2 and taus.shape[1] == 4
            score = (lambda bits, t: self._score_durations(bits, t, num_threads)) if durations else \
                (lambda bits, t: self.score(bits, num_threads))
            per_file = np.concatenate([score(self._host(taus[a:a + per_batch], True, False, num_threads, core=False)[1],
                                             taus[a:a + per_batch]) for a in range(0, taus.shape[0], per_batch)])
        else:
            raise ValueError(f"backend '{backend}': gpu, host or core")
        comp = per_file.sum(axis=1)
        return TuneResult(_rates(comp), comp, per_file, np.full((taus.shape[0], self.N), -1, dtype=np.int32))

    def _score_durations(self, bits: np.ndarray, taus: np.ndarray, num_threads: int = 8) -> np.ndarray:
        """``(T, N, 5)`` components of the masks of ``replay`` under the durations of ``taus (T, 4)``, by
        ``dz_tune_track_score_dur``: one sequential walk per (trial, file), no lanes."""
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        taus = np.ascontiguousarray(taus, dtype=np.float64)
        out = np.zeros((bits.shape[0], self.N, 5), dtype=np.float64)
        _lib.check(_lib.load().dz_tune_track_score_dur(C.byref(self._host_cells()), bits.shape[0], bits.ctypes.data,
                                                       taus.ctypes.data, out.ctypes.data, int(num_threads)),
                   "dz_tune_track_score_dur")
        return out

    def hypothesis(self, bits_row: np.ndarray, n: int, min_duration_on: float = 0.0,
                   min_duration_off: float = 0.0) -> Annotation:
        """File n's hypothesis under one trial as ``PredictionAccumulator`` ends with it: turns labelled "speech"
        (``VadTuneCache``) or "overlap" (``OsdTuneCache``); with durations, filtered by ``functional.min_duration``."""
        ann = self._hypothesis(bits_row, n, 1, lambda g: self.LABEL)
        if min_duration_on == 0.0 and min_duration_off == 0.0:
            return ann
        from .functional import min_duration
        return min_duration(ann, min_duration_on, min_duration_off, PATCH_COLLAR)


class VadTuneCache(_TrackTuneCache):
    """``TuneCache``'s sibling for ``VoiceActivityDetection``: the track is the max of the segmentation over the local
    speakers.  The reference is collapsed to speech / non-speech: a scoring cell's one reference bit is "any reference
    speaker active"."""

    KIND, REPLAY, PIPELINE, LABEL = "VadTuneCache", "vad", "VoiceActivityDetection", "speech"
    ELSEWHERE = "TuneCache collects SpeakerDiarization"

    @staticmethod
    def _reference(reference):
        turns = _reference_turns(reference)
        return turns, turns

    @classmethod
    def _check_kind(cls, path, kind: Optional[str]) -> None:
        holds = "TuneCache (SpeakerDiarization)" if kind is None else kind
        raise ValueError(f"{path} holds a {holds}, not a VadTuneCache")

    @classmethod
    def from_tune_cache(cls, cache: "TuneCache", tau_active: Optional[float] = None) -> "VadTuneCache":
        """The ``VadTuneCache`` of a collected ``TuneCache``, whose raw scores are the same model's: the track is their
        float32 max over the speakers (NaN propagates), what ``VoiceActivityDetection.model_outputs`` returns.
        ``tau_active``: the base value; None takes the diarization cache's."""
        return cls._from_scores(cache, tau_active, lambda scores: torch.max(scores, dim=-1)[0])


class OsdTuneCache(_TrackTuneCache):
    """``VadTuneCache``'s sibling for ``OverlappedSpeechDetection``: the track is the second largest of the segmentation
    over the local speakers (``functional.overlap_track``).  The reference is an ordinary speaker annotation; a scoring
    cell's one reference bit is "at least two DIFFERENT reference speakers active" — the cells are built from
    ``metrics.overlap_reference`` of it (touching regions merged), what ``OverlapDetectionErrorRate`` scores against.
    ``save`` keeps the speaker turns as given, so that ``load`` builds the same cells.  The replay, both kernels and the
    host backends are the VAD tuner's: they see another track and other reference prefix sums."""

    KIND, REPLAY, PIPELINE, LABEL = "OsdTuneCache", "osd", "OverlappedSpeechDetection", "overlap"
    ELSEWHERE = "VadTuneCache collects VoiceActivityDetection, TuneCache collects SpeakerDiarization"

    @staticmethod
    def _reference(reference):
        if isinstance(reference, Annotation):
            reference = [(seg.start, seg.end, label) for seg, _, label in reference.itertracks(yield_label=True)]
        stored = [(float(s), float(e), str(label)) for s, e, label in reference]
        ann = Annotation()
        for n, (s, e, label) in enumerate(stored):
            ann[Segment(s, e), n] = label
        return stored, _turns(overlap_reference(ann))

    @classmethod
    def _check_kind(cls, path, kind: Optional[str]) -> None:
        holds = "TuneCache (SpeakerDiarization)" if kind is None else f"{kind}"
        raise ValueError(f"{path} holds a {holds}, not an OsdTuneCache (OverlappedSpeechDetection)")

    @classmethod
    def from_tune_cache(cls, cache: "TuneCache", tau_active: float = 0.5, device=None) -> "OsdTuneCache":
        """The ``OsdTuneCache`` of a collected ``TuneCache``: the track is ``functional.overlap_track`` of its raw scores
        — the defining torch statement on the host, ``overlap_track_kernel`` with ``device`` a GPU (the same values:
        a selection, no arithmetic).  ``tau_active``: the base value, this pipeline's default."""
        if isinstance(cache, TuneCache) and cache.K < 2:
            raise ValueError(f"OsdTuneCache.from_tune_cache: a cache of {cache.K} local speaker per chunk has no overlap "
                             "track (at least 2 speakers)")
        from .functional import overlap_track
        return cls._from_scores(cache, tau_active,
                                lambda scores: overlap_track(scores if device is None else scores.to(device)))


def _pipeline_kind(pipeline_class) -> str:
    """Which of the two original caches: "dia" for ``SpeakerDiarization`` (``TuneCache``), "vad" for
    ``VoiceActivityDetection`` (``VadTuneCache``), a ValueError for anything else.  ``_replay_kind`` is the question
    "is this class tuned by replay, and how"."""
    from .blocks.diarization import SpeakerDiarization
    from .blocks.vad import VoiceActivityDetection
    if pipeline_class is SpeakerDiarization:
        return "dia"
    if pipeline_class is VoiceActivityDetection:
        return "vad"
    name = getattr(pipeline_class, "__name__", repr(pipeline_class))
    raise ValueError(f"pipeline class {name}: neither SpeakerDiarization (TuneCache) nor VoiceActivityDetection "
                     "(VadTuneCache)")


def _replay_kind(pipeline_class) -> str:
    """"dia" for ``SpeakerDiarization``, "vad" for ``VoiceActivityDetection``, "osd" for
    ``OverlappedSpeechDetection``; nothing else is tuned by replay (a subclass may change what the cached outputs
    mean)."""
    from .blocks.osd import OverlappedSpeechDetection
    if pipeline_class is OverlappedSpeechDetection:
        return "osd"
    try:
        return _pipeline_kind(pipeline_class)
    except ValueError:
        name = getattr(pipeline_class, "__name__", repr(pipeline_class))
        raise ValueError(f"pipeline class {name}: only SpeakerDiarization, VoiceActivityDetection and "
                         "OverlappedSpeechDetection are tuned by replaying cached model outputs") from None


def _check_pipeline_class(pipeline_class) -> None:
    kind = _replay_kind(pipeline_class)
    if kind != "dia":
        other = "VadTuneCache" if kind == "vad" else "OsdTuneCache"
        raise ValueError(f"pipeline class {pipeline_class.__name__}: TuneCache replays SpeakerDiarization; "
                         f"{other} is the cache of {pipeline_class.__name__}")


def trial_config(base_config, values: Dict[str, float]):
    """``base_config`` with the tuned hyper-parameters of one trial (the models are shared, not copied)."""
    cfg = copy.copy(base_config)
    for name, v in values.items():
        setattr(cfg, name, float(v))
    return cfg


_MATCH_DEFAULTS = dict(sweep=None, top_n=None, normalised=False)     # Optimizer: a study file without these keys


class Optimizer:
    """The reference's ``Optimizer`` (``optim.py:17-141``) on a ``TuneCache``: same constructor, ``objective`` value
    (the metric in percent), ``__call__(num_iter, show_progress)``, ``best_performance`` and ``best_hparams``.  optuna
    is replaced by a directory: ``<path>/<stem>.json`` holds every trial and is loaded if it exists, a second call
    continues the numbering and never evaluates a stored trial again.  ``sampler``: "random" (uniform over each
    parameter's range, from ``seed``) or "grid" (``num_iter`` as a total: the largest cube not above it).  Trials are
    evaluated ``trials_per_batch`` at a time; ``cache``: a collected ``TuneCache`` (the models then never run);
    ``scoring``: ``TuneCache.evaluate``'s (None and "host": on host threads, "device": on the replay's backend).
    ``pipeline_class``: ``SpeakerDiarization``, or ``VoiceActivityDetection`` — then ``tau_active`` alone is tuned (the
    default; ``hparams=`` may name ``TauOffset``, ``MinDurationOn`` and ``MinDurationOff`` beside or instead of it), the
    metric is the detection error rate and the cache a ``VadTuneCache`` — or ``OverlappedSpeechDetection``:
    ``tau_active`` alone, an ``OsdTuneCache``, and as the metric ``OverlapDetectionErrorRate`` (the default) or, with
    ``direction="maximize"``, ``OverlapDetectionFMeasure``: the objective is then ``100 * F`` of the components summed
    over the files (``metrics.detection_prf``).  ``gallery``: a ``SpeakerGallery`` (``SpeakerDiarization`` only) — then
    ``delta_id`` is tuned beside the three (``blocks.base.DeltaId``), the cache is an ``IdentTuneCache`` (a ``TuneCache``
    is matched against the gallery on first use), the metric is the ``IdentificationErrorRate`` and ``delta_id=`` is
    required: the value of the kick-start trial, and of every trial when ``DeltaId`` is not among ``hparams``.  There is
    no default.  ``normalised=True`` (a gallery with a cohort): the match is the cohort-normalised one, ``delta_id`` is a
    signed threshold, a ``TuneCache`` is matched with ``with_gallery(gallery, normalised=True, top_n=top_n)`` and
    ``base.DeltaId`` is sampled over ``cache.delta_range()`` (a ``HyperParameter("delta_id", lo, hi)`` of the caller's
    is taken as given).  ``sweep=Q``: ``delta_id`` is not sampled; every sampled clustering trial is scored by
    ``IdentTuneCache.evaluate_sweep`` on every plane at the constructor's ``delta_id`` followed by Q equally spaced
    interior values of ``cache.delta_range()``, its value is the best finite point (ties: the lowest point index) and
    its stored ``params`` gain the winner's ``delta_id`` and, with more than one plane, ``top_n``.  The planes of a study
    are those of a matched cache, else ``top_n=``, else the gallery's own; more than one needs ``sweep=``; the study file
    records them (with ``sweep`` and ``normalised``) and is continued with the same only."""

    def __init__(self, pipeline_class: type, speech_path, reference_path, study_or_path, batch_size: int = 32,
                 hparams: Optional[Sequence[base.HyperParameter]] = None, base_config=None,
                 do_kickstart_hparams: bool = True, metric=None, direction: str = "minimize", sampler: str = "random",
                 seed: int = 0, trials_per_batch: int = 256, cache=None, backend: Optional[str] = None,
                 scoring: Optional[str] = None, gallery=None, delta_id=None, normalised: bool = False, top_n=None,
                 sweep: Optional[int] = None):
        self.kind = _replay_kind(pipeline_class)
        self.normalised, self.top_n, self.sweep = bool(normalised), None, None
        if gallery is None:
            for name, given in (("normalised", bool(normalised)), ("top_n", top_n is not None), ("sweep", sweep is not None)):
                if given:
                    raise ValueError(f"{name}= is about the match against gallery=, which is not given")
        if top_n is not None:
            if not normalised:
                raise ValueError("top_n= chooses the planes of the normalised match; it needs normalised=True")
            self.top_n = list(_check_top_ns(top_n, gallery, "Optimizer(gallery=...)"))
        if sweep is not None:
            if isinstance(sweep, bool) or not isinstance(sweep, (int, np.integer)) or sweep < 1:
                raise ValueError(f"sweep={sweep!r}: the number of thresholds per trial, an integer of at least 1")
            self.sweep = int(sweep)
        track = self.kind != "dia"                 # a track pipeline: tau_active alone, scored where it is replayed
        if scoring not in (None, "host", "device"):
            raise ValueError(f"scoring '{scoring}': host or device")
        self.gallery, self.delta_id = gallery, None
        if gallery is not None:
            if track:
                raise ValueError(f"gallery=: {pipeline_class.__name__} has no speakers to name; only SpeakerDiarization is "
                                 "tuned against a gallery")
            if scoring is not None:
                raise ValueError("scoring: with gallery= the trials are scored where they are replayed (backend), like the "
                                 "track pipelines")
            from .gallery import check_delta_id
            if self.normalised and getattr(gallery, "cohort", None) is None:
                raise ValueError("normalised=True: gallery= has no cohort to normalise against")
            self.delta_id = check_delta_id(delta_id, "Optimizer(gallery=...)", signed=self.normalised)
            self.kind = "ident"
        elif delta_id is not None:
            raise ValueError("delta_id= is the identification distance of gallery=, which is not given")
        elif isinstance(metric, IdentificationErrorRate):
            raise ValueError("metric IdentificationErrorRate compares names: it needs gallery= (a SpeakerGallery) and "
                             "delta_id=")
        if track and scoring is not None:
            raise ValueError(f"scoring: {pipeline_class.__name__} is scored where it is replayed (backend); only "
                             "SpeakerDiarization takes scoring='host' or 'device'")
        self.scoring = scoring
        self.cache_class = {"dia": TuneCache, "ident": IdentTuneCache, "vad": VadTuneCache, "osd": OsdTuneCache}[self.kind]
        self.tunable = TRACK_TUNABLE if track else IDENT_TUNABLE if gallery is not None else TUNABLE
        if gallery is not None and type(cache) is TuneCache:
            pass                                   # matched against the gallery on first use (the cache property)
        elif gallery is not None and isinstance(cache, IdentTuneCache) and cache.names != tuple(gallery.names):
            raise ValueError("cache: this IdentTuneCache was matched against another gallery (other names) than gallery=")
        elif gallery is not None and isinstance(cache, IdentTuneCache) and cache.normalised != self.normalised:
            raise ValueError(f"cache: this IdentTuneCache holds the {'normalised' if cache.normalised else 'raw'} match, "
                             f"and normalised={self.normalised}")
        elif gallery is not None and isinstance(cache, IdentTuneCache) and self.top_n is not None and \
                list(cache.top_ns) != self.top_n:
            raise ValueError(f"cache: this IdentTuneCache holds the planes top_ns = {list(cache.top_ns)}, and "
                             f"top_n={self.top_n}")
        elif gallery is None and isinstance(cache, IdentTuneCache):
            raise ValueError("cache: an IdentTuneCache is tuned with gallery= and delta_id=; the TuneCache it was made "
                             "from tunes the diarization error rate")
        elif cache is not None and not isinstance(cache, self.cache_class):
            raise ValueError(f"pipeline class {pipeline_class.__name__}: cache must be a {self.cache_class.__name__}, "
                             f"got a {type(cache).__name__}")
        # the planes of the study: those of a matched cache, else top_n=, else the gallery's own (a raw match has none);
        # they are what the study file records, so a study cannot be continued on other planes unnoticed
        if self.normalised:
            self.top_n = (list(cache.top_ns) if isinstance(cache, IdentTuneCache) else
                          self.top_n if self.top_n is not None else [int(gallery.top_n)])
            if len(self.top_n) > 1 and self.sweep is None:
                raise ValueError(f"top_n={self.top_n}: a trial without sweep= is scored on one plane; several planes are "
                                 "compared by sweep=")
        self.pipeline_class = pipeline_class
        self.speech_path, self.reference_path, self.batch_size = speech_path, reference_path, batch_size
        wanted = {"dia": DiarizationErrorRate, "ident": IdentificationErrorRate, "vad": DetectionErrorRate,
                  "osd": OverlapDetectionErrorRate}[self.kind]
        self.fmeasure = self.kind == "osd" and isinstance(metric, OverlapDetectionFMeasure)
        if metric is not None and not isinstance(metric, wanted) and not self.fmeasure:
            raise ValueError(f"metric {type(metric).__name__}: the replay of {pipeline_class.__name__} "
                             f"{'with a gallery ' if gallery is not None else ''}scores the "
                             f"{wanted.name} ({wanted.__name__}) only"
                             + (", or OverlapDetectionFMeasure with direction='maximize'" if self.kind == "osd" else ""))
        if direction not in ("minimize", "maximize"):
            raise ValueError(f"direction '{direction}': minimize or maximize")
        if self.fmeasure and direction != "maximize":
            raise ValueError(f"metric OverlapDetectionFMeasure with direction '{direction}': an F-measure is maximised "
                             "(direction='maximize')")
        if sampler not in ("random", "grid"):
            raise ValueError(f"sampler '{sampler}': random or grid")
        self.metric, self.direction, self.sampler, self.seed = metric, direction, sampler, int(seed)
        self.trials_per_batch, self.backend = max(1, int(trials_per_batch)), backend
        self.base_config, self.do_kickstart_hparams = base_config, do_kickstart_hparams
        if self.base_config is None:
            self.base_config = pipeline_class.get_config_class()()
            self.do_kickstart_hparams = False
        default = list(pipeline_class.hyper_parameters()) + ([base.DeltaId] if gallery is not None and self.sweep is None
                                                             else [])
        self.hparams = list(default if hparams is None else hparams)
        if self.sweep is not None and any(p.name == "delta_id" for p in self.hparams):
            raise ValueError(f"hyper-parameter delta_id (DeltaId) with sweep={self.sweep}: the sweep covers delta_id at "
                             "every trial, so it is not sampled; leave it out of hparams=")
        if self.sweep is not None and self.direction != "minimize":
            raise ValueError("sweep= keeps every trial's lowest point: direction='minimize'")
        self._space: Optional[List[base.HyperParameter]] = None
        possible = vars(self.base_config)
        if not track and (hasattr(self.base_config, "tau_offset") or any(p.name == "tau_offset" for p in self.hparams)):
            from .blocks.diarization import refuse_tau_offset
            refuse_tau_offset({"tau_offset": None}, f"Optimizer({pipeline_class.__name__})")
        if not track:
            base.refuse_min_duration({name: None for name in DURATIONS if hasattr(self.base_config, name) or
                                      any(p.name == name for p in self.hparams)}, f"Optimizer({pipeline_class.__name__})")
        if track:
            base.check_tau_offset(getattr(self.base_config, "tau_offset", None), "Optimizer: base_config")
            for name in DURATIONS:
                base.check_min_duration(getattr(self.base_config, name, 0.0), name, "Optimizer: base_config")
        for param in self.hparams:
            if param.name == "delta_id" and gallery is None:
                raise ValueError("hyper-parameter delta_id is the identification distance of a gallery: gallery= and "
                                 "delta_id= are not given")
            if param.name not in self.tunable:
                raise ValueError(f"hyper-parameter {param.name} changes the model outputs: only "
                                 f"{', '.join(self.tunable)} are tuned by replaying them")
            assert param.name in possible or param.name == "delta_id", (f"Hyper-parameter {param.name} not found in configuration "
                                            f"{self.base_config.__class__.__name__}")
        if not track and int(self.base_config.max_speakers) > MAX_SPEAKERS:
            raise ValueError(f"max_speakers = {self.base_config.max_speakers}: the replay keeps one 32-bit mask per "
                             f"frame, at most {MAX_SPEAKERS} speakers")
        if not isinstance(study_or_path, (str, Path)):
            raise TypeError(f"Expected a path-like study directory, but got {type(study_or_path).__name__}: optuna "
                            "studies are not supported, trials are kept in <path>/<stem>.json")
        self.study_path = Path(study_or_path)
        self.study_file = self.study_path / f"{self.study_path.stem}.json"
        self.trials: List[dict] = []
        if self.study_file.exists():
            stored = json.loads(self.study_file.read_text())
            names = [p.name for p in self.hparams]
            if stored.get("direction") != self.direction or stored.get("hparams") != names:
                raise ValueError(f"{self.study_file} holds a study of {stored.get('hparams')} ({stored.get('direction')}), "
                                 f"not of {names} ({self.direction}): its trials cannot be continued with other "
                                 "hyper-parameters or the other direction")
            for key, mine in self._match_keys().items():           # (a study without them: the defaults)
                if stored.get(key, _MATCH_DEFAULTS[key]) != mine:
                    raise ValueError(f"{self.study_file} holds a study with {key}={stored.get(key, _MATCH_DEFAULTS[key])!r}, "
                                     f"not {key}={mine!r}: its trials cannot be continued with another {key}")
            self.trials = stored["trials"]
        self._cache = cache

    @property
    def cache(self):
        if self._cache is None:
            kw = {} if self.gallery is None else dict(gallery=self.gallery, normalised=self.normalised, top_n=self.top_n)
            self._cache = self.cache_class.collect(self.pipeline_class, self.base_config, self.speech_path, self.reference_path,
                                            self.batch_size, **kw)
        if self.gallery is not None and type(self._cache) is TuneCache:
            self._cache = self._cache.with_gallery(self.gallery, normalised=self.normalised, top_n=self.top_n)
        return self._cache

    def _match_keys(self) -> dict:
        """What the study file records about the match: a study continues with the same values only."""
        return dict(sweep=self.sweep, top_n=self.top_n, normalised=self.normalised)

    def _ranges(self) -> List[base.HyperParameter]:
        """``hparams`` as they are sampled: ``base.DeltaId`` itself stands for the range of the stored normalised
        distances of a normalised cache (its own (0, 2) is for raw distances)."""
        if self._space is None:
            self._space = [base.HyperParameter("delta_id", *self.cache.delta_range())
                           if p is base.DeltaId and self.normalised else p for p in self.hparams]
        return self._space

    def sweep_thresholds(self) -> np.ndarray:
        """The thresholds of every trial of a ``sweep=Q`` study: the constructor's ``delta_id``, then Q equally spaced
        interior values of ``cache.delta_range()``."""
        lo, hi = self.cache.delta_range()
        return np.concatenate([[self.delta_id], np.linspace(lo, hi, self.sweep + 2)[1:-1]])

    def objective_sweep(self, params: Sequence[Dict[str, float]]):
        """``(values, winners)`` of a ``sweep=Q`` study: the metric in percent at every trial's best finite point (NaN
        where no point is finite), and what that point adds to the trial's parameters."""
        hp = np.array([[float(p.get(name, self._base_value(name))) for name in TUNABLE] for p in params], dtype=np.float64)
        result = self.cache.evaluate_sweep(hp, self.sweep_thresholds(), backend=self.backend)
        T, P, Q = result.rate.shape
        flat = result.rate.reshape(T, P * Q)
        best = np.argmin(np.where(np.isnan(flat), np.inf, flat), axis=1)          # (the first among equals)
        values = 100.0 * flat[np.arange(T), best]
        winners = []
        for j in best:
            won = dict(delta_id=float(result.delta_id[j % Q]))
            if P > 1:
                won["top_n"] = int(result.top_n[j // Q])
            winners.append(won)
        return values, winners

    def _complete(self) -> List[dict]:
        return [t for t in self.trials if t["value"] is not None]

    @property
    def best_trial(self) -> dict:
        done = self._complete()
        if not done:
            raise ValueError("no completed trial yet")
        pick = min if self.direction == "minimize" else max
        return pick(done, key=lambda t: t["value"])

    @property
    def best_performance(self) -> float:
        return self.best_trial["value"]

    @property
    def best_hparams(self) -> Dict[str, float]:
        return dict(self.best_trial["params"])

    def _values(self, params: Dict[str, float]) -> List[float]:
        """(tau, rho, delta) of a trial ((tau) of a track pipeline): the sampled parameters, the base config's
        value for the others."""
        if self.kind in ("vad", "osd"):
            # (tau_active,) — today's kernels — unless tau_offset is tuned or the base configuration sets one; an offset
            # that is not tuned is the base configuration's in every trial, and the trial's own tau_active without one
            tau = float(params.get("tau_active", self.base_config.tau_active))
            fixed = getattr(self.base_config, "tau_offset", None)
            offset = tau if "tau_offset" not in params and fixed is None else float(params.get("tau_offset", fixed))
            if self._durations():
                # four columns: a duration that is not tuned is the base configuration's in every trial, and a trial
                # without hysteresis carries its own tau_active as the offset
                return [tau, offset] + [float(params.get(name, getattr(self.base_config, name, 0.0))) for name in DURATIONS]
            if "tau_offset" not in params and fixed is None:
                return [tau] if not self._hysteresis() else [tau, tau]
            return [tau, offset]
        return [float(params.get(name, self._base_value(name))) for name in self.tunable]

    def _hysteresis(self) -> bool:
        """Does a trial of this study carry (tau_active, tau_offset)?"""
        return (any(p.name == "tau_offset" for p in self.hparams) or
                getattr(self.base_config, "tau_offset", None) is not None)

    def _durations(self) -> bool:
        """Does a trial of this study carry (tau_active, tau_offset, min_duration_on, min_duration_off)?  Only when a
        duration is tuned or the base configuration sets one non-zero: otherwise the kernels launched are those of a
        study without them."""
        return any(p.name in DURATIONS for p in self.hparams) or \
            any(float(getattr(self.base_config, name, 0.0)) != 0.0 for name in DURATIONS)

    def _base_value(self, name: str) -> float:
        """The base configuration's value; delta_id is no field of a configuration: the constructor's.  A tau_offset of
        None is the configuration's tau_active."""
        if name == "tau_offset" and getattr(self.base_config, "tau_offset", None) is None:
            return self.base_config.tau_active
        return self.delta_id if name == "delta_id" else getattr(self.base_config, name)

    def objective(self, params: Sequence[Dict[str, float]]) -> np.ndarray:
        """The metric in percent of every trial of ``params`` (NaN where the clustering would raise); with an
        ``OverlapDetectionFMeasure``, 100 x F of the components summed over the files."""
        hp = np.array([self._values(p) for p in params], dtype=np.float64)
        kw = {} if self.scoring is None else dict(scoring=self.scoring)
        result = self.cache.evaluate(hp, backend=self.backend, **kw)
        return 100.0 * (detection_prf(result.components)[2] if self.fmeasure else result.rate)

    def _grid(self, total: int) -> List[Dict[str, float]]:
        """The largest cube of at most ``total`` points: the same number of equally spaced interior values per axis."""
        side = 1
        while (side + 1) ** len(self.hparams) <= total:
            side += 1
        axes = [np.linspace(p.low, p.high, side + 2)[1:-1] for p in self._ranges()]
        mesh = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(self.hparams))
        return [{p.name: float(v) for p, v in zip(self.hparams, row)} for row in mesh]

    def _random(self, number: int) -> Dict[str, float]:
        """The draw of trial ``number`` depends on (seed, number) only, so a resumed study continues the sequence."""
        rng = np.random.default_rng([self.seed, number])
        return {p.name: float(rng.uniform(p.low, p.high)) for p in self._ranges()}

    def _sampled(self, params: Dict[str, float]) -> Dict[str, float]:
        """A stored trial's sampled keys: a sweep adds the winning point's ``delta_id`` and ``top_n`` to them."""
        if self.sweep is None:
            return params
        names = {p.name for p in self.hparams}
        return {k: v for k, v in params.items() if k in names}

    def _store(self) -> None:
        self.study_path.mkdir(parents=True, exist_ok=True)
        payload = dict(direction=self.direction, hparams=[p.name for p in self.hparams], trials=self.trials)
        if self._match_keys() != _MATCH_DEFAULTS:              # (a study without them keeps the keys it always had)
            payload.update(self._match_keys())
        tmp = self.study_file.with_suffix(".json.tmp")
        tmp.write_text(json.dumps(payload, indent=1))
        tmp.replace(self.study_file)

    def __call__(self, num_iter: int, show_progress: bool = True):
        queue: List[Dict[str, float]] = []
        if self.do_kickstart_hparams:
            kick = {p.name: float(self._base_value(p.name)) for p in self.hparams}
            if not any(self._sampled(t["params"]) == kick for t in self.trials):
                queue.append(kick)
        if self.sampler == "grid":
            stored = [self._sampled(t["params"]) for t in self.trials]
            queue += [p for p in self._grid(int(num_iter)) if p not in stored and p not in queue]
        else:
            first = len(self.trials)
            queue += [self._random(first + j) for j in range(len(queue), int(num_iter))]
        for a in range(0, len(queue), self.trials_per_batch):
            batch = queue[a:a + self.trials_per_batch]
            if self.sweep is not None:
                values, winners = self.objective_sweep(batch)
                batch = [{**params, **won} if not np.isnan(v) else params for params, won, v in zip(batch, winners, values)]
            else:
                values = self.objective(batch)
            for params, v in zip(batch, values):
                self.trials.append(dict(number=len(self.trials), params=params, value=None if np.isnan(v) else float(v)))
            self._store()
            if show_progress:
                done = self._complete()
                best = f"best {self.best_performance:.3f}" if done else "no completed trial"
                print(f"[tune] trial {len(self.trials)}: {best}", flush=True)
        return self
