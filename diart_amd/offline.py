"""Whole-file speaker diarization: the models of the streaming pipeline, the clustering of a batch system.

``SpeakerDiarization`` decides each chunk's speakers from the past alone.  Where a recording is known from end to end
this module instead embeds every (chunk, local speaker), clusters all of the embeddings at once — agglomerative,
centroid linkage, float64, on the GPU (``csrc/k_agglo.hip``) — and rebuilds the timeline from the clustered chunks,
the way pyannote's file pipeline uses the same checkpoints.  The model half is ``TuneCache.collect``'s: a collected
``TuneCache`` holds everything this mode reads, and ``from_cache`` runs no model.

The linkage does not depend on ``threshold``: ``linkage`` returns one dendrogram per file, which ``functional.cut_linkage``
cuts at any threshold afterwards.  There is no default threshold and none is recommended; the error rate of this mode on
real recordings has not been measured (DESIGN.md 4.24 states the definition and what rests on a reading of pyannote's
published code rather than on a run of it).

``python -m diart_amd.offline wav/ --output rttm/ --segmentation SEG --embedding EMB --threshold T [--reference rttm/]
[--cache FILE]`` writes one RTTM per file.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, functional
from .features import Annotation, Segment

MIN_CLUSTER_SIZE = 12        # pyannote's AgglomerativeClustering default, read from its published code
MIN_CLEAN_RATIO = 0.2        # pyannote's SpeakerDiarization.filter_embeddings, likewise


class CollectedFiles:
    """What this mode reads of a ``TuneCache``, and nothing else: ``files`` (dicts with ``uri``, ``seg (C, F, K)``,
    ``emb (C, K, D)``, ``starts (C)``, ``res (C)``, ``shift``) and their common ``F``, ``K``, ``D``.  ``from_cache``,
    ``linkage``, ``clusters`` and ``activity`` take either."""

    def __init__(self, files: Sequence[dict]):
        self.files = list(files)
        self.N = len(self.files)
        shapes = {(f["seg"].shape[1:], f["emb"].shape[2]) for f in self.files}
        if len(shapes) != 1:
            raise ValueError(f"the files share frames, local speakers and dimension, got {sorted(shapes)}")
        (self.F, self.K), self.D = next(iter(shapes))


class OfflineDiarization:
    """``config``: a ``SpeakerDiarizationConfig`` (``tau_active`` and ``max_speakers`` are what the clustering reads;
    ``__call__`` builds the pipeline's model half from the rest).  ``threshold``: the height at which the dendrogram
    is cut, a Euclidean distance between centroids of unit embeddings; required and finite.  ``backend``: ``"gpu"``,
    ``"core"`` (the kernels' text on host threads) or ``None``, the GPU when there is one."""

    def __init__(self, config, threshold: float, min_cluster_size: int = MIN_CLUSTER_SIZE,
                 min_clean_ratio: float = MIN_CLEAN_RATIO, backend: Optional[str] = None,
                 memory_budget: int = functional.LINKAGE_MEMORY_BUDGET, num_threads: int = 8):
        if threshold is None or not math.isfinite(float(threshold)):
            raise ValueError(f"threshold must be a finite number, got {threshold} (there is no default)")
        if int(min_cluster_size) < 1:
            raise ValueError(f"min_cluster_size must be at least 1, got {min_cluster_size}")
        if not 0.0 <= float(min_clean_ratio) <= 1.0:
            raise ValueError(f"min_clean_ratio must lie in [0, 1], got {min_clean_ratio}")
        get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
        self.max_speakers = int(get("max_speakers"))
        if self.max_speakers < 1:
            raise ValueError(f"max_speakers must be at least 1, got {self.max_speakers}")
        if backend not in (None, "gpu", "core"):
            raise ValueError(f"backend must be 'gpu', 'core' or None, got {backend!r}")
        self.config = config
        self.tau_active = float(get("tau_active"))
        self.threshold, self.min_cluster_size = float(threshold), int(min_cluster_size)
        self.min_clean_ratio = float(min_clean_ratio)
        self.backend, self.memory_budget, self.num_threads = backend, int(memory_budget), int(num_threads)
        self._pipeline = None

    # ------------------------------------------------------------------------------------------------------- rows
    def _rows(self, f: dict):
        """The usable (chunk, local speaker) rows of a cached file in row-major order, scaled to unit length in
        float64, which of them are clustered, and the chunk-level facts the reconstruction needs."""
        seg, emb = f["seg"], f["emb"]
        F = seg.shape[1]
        valid = np.isfinite(seg).all(axis=(1, 2))
        with np.errstate(invalid="ignore"):
            on = (seg > np.float64(self.tau_active)) & valid[:, None, None]
        clean = on & (on.sum(axis=2) == 1)[:, :, None]
        e = emb.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            norm = np.sqrt((e * e).sum(axis=2))
            usable = np.isfinite(e).all(axis=2) & np.isfinite(norm) & (norm > 0) & (on.sum(axis=1) >= 1)
        is_train = usable & (clean.sum(axis=1) >= math.ceil(self.min_clean_ratio * F))
        x = np.ascontiguousarray(e[usable] / norm[usable][:, None])
        return x, usable, np.flatnonzero(is_train[usable]).astype(np.int32)

    def _check_cache(self, cache) -> None:
        if cache.D > functional.LINKAGE_MAX_DIM:
            raise ValueError(f"embeddings of dimension {cache.D}: whole-file clustering takes at most "
                             f"{functional.LINKAGE_MAX_DIM}")

    def _linkages(self, rows):
        return functional.linkage_unit_rows([x[train] for x, _, train in rows], self.backend, getattr(self.config, "device", None)
                                            if self._on_gpu() else None, self.memory_budget, self.num_threads)

    def _on_gpu(self) -> bool:
        import torch
        return self.backend == "gpu" or (self.backend is None and torch.cuda.is_available())

    def linkage(self, cache) -> List[np.ndarray]:
        """One dendrogram ``(N - 1, 4)`` per file of ``cache`` (a ``TuneCache``), over the file's train rows: cut it at
        any threshold with ``functional.cut_linkage``."""
        self._check_cache(cache)
        return self._linkages([self._rows(f) for f in cache.files])

    # ---------------------------------------------------------------------------------------------- from a cache
    def from_cache(self, cache) -> List[Annotation]:
        """One ``Annotation`` per file of ``cache``; no model runs."""
        return [self._annotation(f, active) for f, active in zip(cache.files, self.activity(cache))]

    def activity(self, cache) -> List[np.ndarray]:
        """Per file of ``cache`` the ``(T, G)`` array behind its ``Annotation``: output frame t has speaker g on."""
        lib = _lib.load()
        N, F, K = cache.N, cache.F, cache.K
        assigns, offsets, kept, frames, actives = [], [], [], [], []
        for f, (assign_ck, G) in zip(cache.files, self.clusters(cache)):
            res = float(f["res"][0])
            off = np.rint((f["starts"] - f["starts"][0]) / res).astype(np.int32)
            T = int(off[-1]) + F
            assigns.append(np.ascontiguousarray(assign_ck))
            offsets.append(np.ascontiguousarray(off))
            kept.append(G)
            frames.append(T)
            actives.append(np.zeros((T, G), dtype=np.uint8))
        ptrs = lambda arrays: (C.c_void_p * N)(*[a.ctypes.data for a in arrays])
        ints = lambda values: np.ascontiguousarray(values, dtype=np.int32)
        chunks, kept_a, frames_a = ints([f["seg"].shape[0] for f in cache.files]), ints(kept), ints(frames)
        _lib.check(lib.dz_offline_reconstruct(N, ptrs([f["seg"] for f in cache.files]), ptrs(assigns), ptrs(offsets),
                                              chunks.ctypes.data, F, K, kept_a.ctypes.data, self.tau_active,
                                              frames_a.ctypes.data, ptrs(actives), self.num_threads),
                   "dz_offline_reconstruct")
        return [a.astype(bool) for a in actives]

    def clusters(self, cache) -> List[tuple]:
        """Per file of ``cache`` ``(assign, G)``: the cluster ``0 .. G - 1`` of every (chunk, local speaker), ``(C, K)``
        int32, -1 where the row is not usable."""
        self._check_cache(cache)
        lib = _lib.load()
        rows = [self._rows(f) for f in cache.files]
        Zs = self._linkages(rows)                       # every refusal of the linkage comes before the GPU is touched
        out = []
        for (x, usable, train), Z in zip(rows, Zs):
            R = x.shape[0]
            assign = np.zeros(R, dtype=np.int32)
            if R == 0:
                G = 0
            elif train.shape[0] == 0:
                G = 1                                    # nothing to cluster: the usable rows form one cluster
            else:
                labels, G = functional.cut_linkage(Z, self.threshold, self.min_cluster_size, self.max_speakers,
                                                   n=train.shape[0])
                labels = np.ascontiguousarray(labels, dtype=np.int32)
                centroids = np.zeros((G, cache.D), dtype=np.float64)
                _lib.check(lib.dz_offline_assign(x.ctypes.data, R, cache.D, train.ctypes.data, labels.ctypes.data,
                                                 train.shape[0], G, assign.ctypes.data, centroids.ctypes.data),
                           "dz_offline_assign")
            assign_ck = np.full(usable.shape, -1, dtype=np.int32)
            assign_ck[usable] = assign
            out.append((assign_ck, G))
        return out

    @staticmethod
    def _annotation(f: dict, active: np.ndarray) -> Annotation:
        """Runs of on-frames -> turns between frame middles (``Binarize``'s convention), labelled ``speaker{g}``."""
        ann = Annotation(uri=f["uri"], modality="speech")
        res, t0 = float(f["res"][0]), float(f["starts"][0]) + float(f["shift"])
        for g in range(active.shape[1]):
            on = np.concatenate([[False], active[:, g] > 0, [False]])
            edges = np.flatnonzero(on[1:] != on[:-1])
            for n, (s, e) in enumerate(zip(edges[::2], edges[1::2])):
                ann[Segment(t0 + (s + 0.5) * res, t0 + (e + 0.5) * res), f"speaker{g}_{n}"] = f"speaker{g}"
        return ann

    # ------------------------------------------------------------------------------------------------ from a file
    def collect(self, wav_path, batch_size: int = 32) -> "CollectedFiles":
        """The model half over one WAV, as ``TuneCache.collect`` runs it over a directory: the file's scores,
        embeddings, window starts, resolution and shift, with none of the tuner's plans."""
        from .blocks.diarization import SpeakerDiarization
        from .optim import _ReplayCache, _diarization_outputs
        if self._pipeline is None:
            self._pipeline = SpeakerDiarization(self.config)
        f = _ReplayCache._collect_file(self._pipeline, wav_path, batch_size, _diarization_outputs(self._pipeline))
        f["seg"], f["emb"] = f.pop("outputs")
        return CollectedFiles([f])

    def __call__(self, wav_path, batch_size: int = 32) -> Annotation:
        return self.from_cache(self.collect(wav_path, batch_size))[0]


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m diart_amd.offline", description=__doc__.split("\n\n")[0])
    ap.add_argument("root", type=str, help="Directory with audio files CONVERSATION.wav")
    ap.add_argument("--output", required=True, type=str, help="Directory that gets one CONVERSATION.rttm per file")
    ap.add_argument("--segmentation", default="pyannote/segmentation", type=str, help="Segmentation checkpoint file")
    ap.add_argument("--embedding", default="pyannote/embedding", type=str, help="Embedding checkpoint file")
    ap.add_argument("--threshold", required=True, type=float,
                    help="Height at which the dendrogram is cut (Euclidean distance of unit centroids). No default")
    ap.add_argument("--min-cluster-size", default=MIN_CLUSTER_SIZE, type=int)
    ap.add_argument("--min-clean-ratio", default=MIN_CLEAN_RATIO, type=float)
    ap.add_argument("--reference", type=str, default=None,
                    help="Directory with CONVERSATION.rttm references: prints the diarization error rate")
    ap.add_argument("--duration", type=float, default=5, help="Chunk duration in seconds. Defaults to 5")
    ap.add_argument("--step", default=0.5, type=float, help="Sliding window step in seconds. Defaults to 0.5")
    ap.add_argument("--tau-active", default=0.5, type=float, help="Activity threshold. Defaults to 0.5")
    ap.add_argument("--gamma", default=3, type=float, help="Overlapped-speech-penalty gamma. Defaults to 3")
    ap.add_argument("--beta", default=10, type=float, help="Overlapped-speech-penalty beta. Defaults to 10")
    ap.add_argument("--max-speakers", default=20, type=int, help="Maximum number of speakers. Defaults to 20")
    ap.add_argument("--batch-size", default=32, type=int, help="Chunks per model call. Defaults to 32")
    ap.add_argument("--backend", default=None, choices=("gpu", "core"), help="Where the linkage runs. Defaults to the GPU")
    ap.add_argument("--cache", type=str, help="File of the collected model outputs: loaded if it exists, written if not "
                                              "(collecting needs --reference)")
    return ap


def run(args: argparse.Namespace, models=None) -> List[Annotation]:
    """``models``: (segmentation, embedding) to use in place of the checkpoints the arguments name."""
    from . import models as m
    from .blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig
    from .features import load_rttm
    from .metrics import DiarizationErrorRate
    from .optim import TuneCache
    if not math.isfinite(args.threshold):
        raise SystemExit(f"--threshold must be finite, got {args.threshold}")
    root, out = Path(args.root).expanduser(), Path(args.output).expanduser()
    cache = TuneCache.load(args.cache) if args.cache and Path(args.cache).exists() else None
    if cache is not None:
        config = dict(tau_active=args.tau_active, max_speakers=args.max_speakers)
    else:
        seg, emb = models if models is not None else (m.SegmentationModel.from_pretrained(args.segmentation),
                                                      m.EmbeddingModel.from_pretrained(args.embedding))
        config = SpeakerDiarizationConfig(segmentation=seg, embedding=emb, duration=args.duration, step=args.step,
                                          latency=args.step, tau_active=args.tau_active, gamma=args.gamma, beta=args.beta,
                                          max_speakers=args.max_speakers, device=None)
    offline = OfflineDiarization(config, args.threshold, args.min_cluster_size, args.min_clean_ratio, args.backend)
    out.mkdir(parents=True, exist_ok=True)
    if cache is None and args.cache:
        if args.reference is None:
            raise SystemExit("--cache FILE is written from a collected TuneCache, which keeps the references: give --reference")
        cache = TuneCache.collect(SpeakerDiarization, config, root, args.reference, args.batch_size)
        cache.save(args.cache)
    if cache is not None:
        annotations = offline.from_cache(cache)
    else:
        annotations = [offline(fp, args.batch_size) for fp in sorted(p for p in root.iterdir() if p.suffix.lower() == ".wav")]
    for ann in annotations:
        with open(out / f"{ann.uri}.rttm", "w") as fh:
            ann.write_rttm(fh)
    if args.reference is not None:
        metric = DiarizationErrorRate()
        for ann in annotations:
            metric(load_rttm(Path(args.reference).expanduser() / f"{ann.uri}.rttm").popitem()[1], ann)
        print(f"[offline] {len(annotations)} files, DER {100 * abs(metric):.2f} %", flush=True)
    return annotations


if __name__ == "__main__":
    run(parser().parse_args())
