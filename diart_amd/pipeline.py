"""Cross-stream driver of the hot path: N concurrent audio streams, one chunk each per step.

The reference batches consecutive windows of ONE stream (``inference.py:126-128``) and keeps one
pipeline object per stream (``blocks/diarization.py:121-125``); 64 concurrent real-time streams
(BASELINE.json config 2) therefore need a driver the reference does not have.  ``StreamBatch``
stacks the current window of every stream into one segmentation / embedding launch sequence and
steps N independent clustering states and (``tail=True``) N aggregation / binarisation states,
producing for each stream exactly what its own ``SpeakerDiarization.__call__`` computes at lines
186-232: segmentation, overlap-aware normalised embeddings, the permuted ``(frames,
max_speakers)`` scores and the speech turns of the region the step finalises.  ``AudioRing`` keeps
the rolling windows of host-fed streams on the device (only new samples are uploaded).

GPU schedule per step (``seg_split`` + ``emb_split`` HIP streams per lane; ``depth`` lanes so that
``depth`` consecutive steps can be in flight at once — the GPU halves of different steps are
independent, only the host-side clustering is sequential per stream):

    stream A_i : sub-batch i: dz_seg_forward (SincNet -> 4 x {x-projection GEMM, persistent
                 LSTM} -> MLP) -> dz_osp  --event-->        (the GEMMs of one sub-batch run
                 under the latency-bound recurrence of the other)
    stream B   : dz_emb_frames (SincNet -> 5 TDNN; independent of the segmentation, fills the
                 CUs the LSTM leaves idle)  <--wait all--  dz_emb_pool -> D2H (pinned)
    host       : clustering + output tail of step t-1 (C++ threads, fp64) while the GPU runs step t

``VadBatch`` is the segmentation-only form for ``VoiceActivityDetection``: no embedding, no clustering; the head kernel
writes each stream's speech track and only that track reaches the host's output tails; ``OverlapBatch`` is the same step
for ``OverlappedSpeechDetection``, the head writing the overlap track (the second largest score).  The other embeddings share the
two-chain engine: ``WeSpeakerBatch`` for the WeSpeaker ResNet34 embedding, whose trunk is the long chain of the step (the
segmentation runs under it), and ``GroupsBatch`` for the groups form (``HipEcapaEmbedding``, BASELINE.json config 3,
``HipSbXvectorEmbedding``, ``HipTitaNetEmbedding``, ``HipSbResNetEmbedding``, ``HipEcapaMelEmbedding``), which ``StreamBatch(seg, emb, ...)``
constructs for them.
"""
from __future__ import annotations

import ctypes as C
import os
import time as _time
from contextlib import contextmanager
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .blocks.aggregation import BatchedOutputTail
from .blocks.clustering import BatchedSpeakerClustering
from .features import Annotation, Segment
from .pcm import PCM_FORMATS
from .models import HipEmbedding, HipSegmentation, HipWeSpeakerEmbedding, _HipGroupsEmbedding, _as_rows

# sample formats of raw client audio (``dz_ring_push_rows_pcm``: the DZ_PCM_* constants; definitions in diart_amd.pcm)
PCM_F32, PCM_S16, PCM_U8, PCM_S32, PCM_ULAW, PCM_ALAW = range(6)
_PCM_OF_DTYPE = {torch.float32: "f32", torch.int16: "s16", torch.int32: "s32"}      # what push_rows infers

# lanes of a throughput engine (>= 64 streams per step on the matrix-core recurrence): profiles/r06*_lanes_grid.json
THROUGHPUT_LANES = 6


class AudioRing:
    """Device-resident rolling window of N streams (``dz_ring_*``): per step only the ``hop`` new
    samples of every stream are uploaded (32 KB instead of the 320 KB window the reference moves
    per chunk, ``blocks/segmentation.py:47``); ``StreamBatch.launch`` reads the window in place.
    The role of ``rearrange_audio_stream`` (reference ``operators.py:44-100``) for N streams."""

    def __init__(self, num_streams: int, window: int = 80000, hop: int = 8000, slack_blocks: int = 2,
                 device: Optional[torch.device] = None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.n, self.window, self.hop, self.slack = num_streams, window, hop, slack_blocks
        self._lib = _lib.load()
        self._h = _lib.vp()
        _lib.check(self._lib.dz_ring_create(_lib.context(self.device.index), num_streams, window, hop,
                                            slack_blocks, C.byref(self._h)), "dz_ring_create")
        self._keep: List[torch.Tensor] = []          # pinned blocks of in-flight copies
        self._readers: List[List[torch.cuda.Event]] = []   # per step: events after its forward passes

    def __del__(self):
        try:
            self._lib.dz_ring_destroy(self._h)
        except Exception:
            pass

    def reset(self):
        _lib.check(self._lib.dz_ring_reset(self._h), "dz_ring_reset")
        self._readers = []

    @staticmethod
    def _mode(block: torch.Tensor) -> int:
        """Where a push finds ``block``: 1 = device memory, 0 = host memory (a staged copy), 2 = pinned host memory.
        Pinned host memory is mapped into the GPU's address space: the scatter kernel reads it IN PLACE over PCIe
        (32 KB per stream per step; if the runtime cannot map it, a staged copy), which keeps the upload off the SDMA
        queue — there it can queue behind the D2H copy of a step whose results are not ready yet, and the next step's
        forward passes then wait for the previous step's (measured: -17 %)."""
        if block.is_cuda:
            return 1
        return 2 if block.is_pinned() and _lib.exp_env("DZ_RING_ZERO_COPY", "1") != "0" else 0

    def push(self, block) -> bool:
        """``block``: (N, hop) float32 — a CPU tensor / ndarray (pinned memory makes the copy
        asynchronous) or a tensor on the ring's GPU.  Enqueued on the current HIP stream, after the
        forward passes of the window it is about to overwrite.  True once the window is complete."""
        if isinstance(block, np.ndarray):
            block = torch.from_numpy(block)
        assert block.dtype == torch.float32 and tuple(block.shape) == (self.n, self.hop), block.shape
        assert block.stride(1) == 1, "rows of the block must be contiguous"
        cur = torch.cuda.current_stream(self.device)
        # block t+1 overwrites samples of windows <= t - slack: wait for that window's readers
        while len(self._readers) > self.slack + 1:
            self._readers.pop(0)
        if len(self._readers) == self.slack + 1:
            for ev in self._readers[0]:
                cur.wait_event(ev)
        _lib.check(self._lib.dz_ring_push(self._h, block.data_ptr(), block.stride(0), self._mode(block),
                                          cur.cuda_stream), "dz_ring_push")
        self._keep = (self._keep + [block])[-4:]
        return self.filled == self.window

    def _read_by(self, streams: List[torch.cuda.Stream]):
        """Called right after forward passes that read the current window were enqueued on
        ``streams``: records the ring's OWN events there (a caller's per-slot events are re-recorded
        when the slot is reused — waiting on such an event later means waiting for the NEWEST step
        that used the slot, which silently serialised consecutive steps)."""
        evs = []
        for st in streams:
            ev = torch.cuda.Event()
            ev.record(st)
            evs.append(ev)
        self._readers.append(evs)

    # ---- streams that advance at their own pace (StreamServer) -------------------------------
    def push_rows(self, block: torch.Tensor, rows: Sequence[int], channels: int = 1, format: Optional[str] = None) -> None:
        """Row j of ``block`` is the next block of stream ``rows[j]`` (each row keeps its own write position).
        ``block``: (k, hop) float32 — or raw client audio of shape (k, hop * channels) or (k, hop, channels) with
        interleaved frames, which the push kernel converts (int16: ``v / 32768``; every format: ``diart_amd.pcm``)
        and averages over the channels (``dz_ring_push_rows_pcm``).  ``format=None`` infers the format from the dtype
        (``torch.float32``, ``torch.int16``, ``torch.int32``); a ``torch.uint8`` block means nothing by itself and
        needs ``format="u8" | "ulaw" | "alaw"``.  Enqueued on the current HIP stream; a pinned host block is read in
        place by the GPU and must stay untouched until that stream has passed this point."""
        k = len(rows)
        if format is None:
            format = _PCM_OF_DTYPE.get(block.dtype)
            if format is None:
                raise TypeError(f"AudioRing.push_rows: {block.dtype} blocks (expected float32, int16 or int32; "
                                "uint8 blocks need format='u8' | 'ulaw' | 'alaw')")
        if format not in PCM_FORMATS:
            raise ValueError(f"AudioRing.push_rows: format={format!r} (expected one of {tuple(PCM_FORMATS)})")
        fmt, dtype = PCM_FORMATS[format]
        if torch.from_numpy(np.zeros(0, dtype)).dtype != block.dtype:
            raise TypeError(f"AudioRing.push_rows: {block.dtype} blocks for format={format!r} (expected {dtype.name})")
        if block.dim() == 3:
            assert tuple(block.shape) == (k, self.hop, channels) and block.stride(2) == 1 \
                and block.stride(1) == channels, "frames of a (k, hop, channels) block must be contiguous"
        else:
            assert tuple(block.shape) == (k, self.hop * channels) and block.stride(1) == 1
        arr = (C.c_int * k)(*[int(r) for r in rows])
        _lib.check(self._lib.dz_ring_push_rows_pcm(self._h, block.data_ptr(), block.stride(0) * block.element_size(), fmt,
                                                   int(channels), self._mode(block), arr, k,
                                                   torch.cuda.current_stream(self.device).cuda_stream),
                   "dz_ring_push_rows_pcm")
        self._keep = (self._keep + [block])[-4:]

    def filled_row(self, row: int) -> int:
        f = C.c_int()
        _lib.check(self._lib.dz_ring_filled_row(self._h, int(row), C.byref(f)), "dz_ring_filled_row")
        return int(f.value)

    def gather(self, rows: Sequence[int], out: torch.Tensor) -> torch.Tensor:
        """``out[j]`` <- the current window of stream ``rows[j]`` (device to device, current HIP
        stream); every listed stream must hold a complete window."""
        k = len(rows)
        assert out.is_cuda and out.dtype == torch.float32 and out.shape[0] >= k and out.shape[1] == self.window
        arr = (C.c_int * k)(*[int(r) for r in rows])
        _lib.check(self._lib.dz_ring_gather(self._h, arr, k, out.data_ptr(), out.stride(0),
                                            torch.cuda.current_stream(self.device).cuda_stream), "dz_ring_gather")
        return out[:k]

    def reset_row(self, row: int) -> None:
        _lib.check(self._lib.dz_ring_reset_row(self._h, int(row)), "dz_ring_reset_row")

    def raw(self) -> Tuple[int, int]:
        ptr, stride = _lib.vp(), C.c_longlong()
        _lib.check(self._lib.dz_ring_window(self._h, C.byref(ptr), C.byref(stride), None), "dz_ring_window")
        return int(ptr.value), int(stride.value)

    @property
    def filled(self) -> int:
        if self.hop % 4:          # no in-place window (dz_ring_window); lock-step pushes advance every row alike
            return self.filled_row(0)
        ptr, stride, f = _lib.vp(), C.c_longlong(), C.c_int()
        _lib.check(self._lib.dz_ring_window(self._h, C.byref(ptr), C.byref(stride), C.byref(f)), "dz_ring_window")
        return int(f.value)

    def snapshot(self) -> torch.Tensor:
        """Contiguous copy (N, window) of the current window (what ``rearrange_audio_stream`` would
        emit); the forward passes do not need it, they read the ring in place."""
        out = torch.empty((self.n, self.window), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.dz_ring_read(self._h, out.data_ptr(),
                                          torch.cuda.current_stream(self.device).cuda_stream), "dz_ring_read")
        return out


class _StepEngine:
    """What the N-stream engines (``StreamBatch``, ``VadBatch``, ``WeSpeakerBatch``) share: the engine choice and the
    bookkeeping state (``_setup``), how the host waits for a step, the front half of ``launch`` (rows, slots, start
    times), the prelude of a window size's first launch (``_prepare``), the pool of result slots, the warm-up on silence,
    the guarded host half of ``finish`` and the teardown of the C handles.  A subclass provides its GPU schedule
    (``_launch_rows``), ``finish`` and ``reset``, and the hooks ``_handles``, ``_new_slot`` and ``_make_tail``."""

    xvector_experiments = False     # does this engine honour the x-vector engine's experiment switches?
    lag = 0                         # slots beyond `max_inflight` (a StreamBatch with shared embedding streams)

    def _timing(self, duration: float, step: float, latency) -> None:
        """``duration``, ``step`` and ``latency`` as the blocks pipelines read them; a latency outside [step, duration]
        is refused."""
        from .blocks.diarization import _latency
        self.duration, self.step = float(duration), float(step)
        self.latency = float(_latency(latency, self.step, self.duration))
        if not self.step <= self.latency <= self.duration:
            raise ValueError(f"{type(self).__name__}: latency should be in the range [{self.step}, {self.duration}], "
                             f"got {self.latency}")

    def _setup(self, segmentation: HipSegmentation, embedding, num_streams: int, device: Optional[torch.device], *,
               lanes: Optional[int], recurrence: Optional[str], inflight: Optional[int], wait: Optional[str],
               warmup: Optional[int], lanes_follow_recurrence: bool) -> None:
        """The engine under a subclass: argument checks first (nothing has touched a device when one refuses), then the
        models on the device, the engine choice and the bookkeeping state.  ``lanes_follow_recurrence``: a matrix-core
        recurrence at >= 64 streams gets ``THROUGHPUT_LANES`` lanes (an engine whose lanes are heavy in memory stays at
        2 whatever the recurrence)."""
        from .config import setting
        if not self.xvector_experiments:
            self._refuse_xvector_experiments()
        self._host_wait(wait)
        # ---- from here on the device
        self.n = int(num_streams)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.seg = segmentation.to(self.device)
        if embedding is not None:
            self.emb = embedding.to(self.device)
        self.device = self.seg.device
        # `depth` lanes, each with its own HIP streams and scratch arenas: step t runs on lane
        # t % depth, so a caller that keeps `depth` tickets between launch() and finish() has that
        # many steps on the GPU at once (the latency-bound recurrence of one step under the GEMMs
        # of the others).  A lane is reused in stream order, which also orders its arenas.
        # Round 5: with >= 64 streams per step the recurrence runs on the matrix cores (16 chains per workgroup: a
        # seventh of the CU-time, twice the latency of a layer) and SIX steps are in flight instead of two — the longer
        # dependent chain of a lane hides under five other steps, and the 128 CUs the one-chain-per-CU recurrence held
        # for most of a step go to the GEMM-shaped kernels: 30 300 -> 33 500 xRT in same-visit pairs
        # (profiles/r05u_recurrence_lanes_grid.json; in round 4, with the slower front end, the same pair measured
        # equal).  Fewer streams (FileBatch's 32 windows per step lost 11 % with it), the exact-f32 precision and an
        # explicit DZ_LSTM keep what they had; the synchronous blocks API always runs the low-latency recurrence.
        rec = setting("recurrence", recurrence, None)
        split = getattr(self.seg, "precision", "f32") == "f16x3"
        self.throughput = self.n >= 64 and rec is None and split and getattr(self.seg, "recurrence", "valu") == "valu"
        # the kernel this engine's handles run: None = the model's own struct
        self.recurrence = self.seg.throughput_recurrence() if self.throughput else (str(rec) if rec is not None and split else None)
        matrix_core = self.recurrence not in (None, "valu")
        many = lanes_follow_recurrence and (self.throughput or (matrix_core and self.n >= 64))
        self.depth = max(1, int(setting("lanes", lanes, THROUGHPUT_LANES if many else 2, int)))
        # How many launched-but-unfinished steps a throughput caller (bench.py, FileBatch) keeps: `depth` lanes
        # run concurrently, the steps beyond that wait IN THE STREAMS of their lane, so that a lane's next
        # step starts the moment the previous one ends instead of after the host has come back from
        # finish() (clustering of an older step + launch overhead: ~0.5 ms per step, during which the
        # lane's segmentation stream sat empty).
        # Round 6: a throughput engine keeps lanes + 2 (the second spare ticket covers the host's own launch + tail time of
        # a step: +3 % in the 20-step form, profiles/r06l_inflight_grid.json); the two-lane engines keep lanes + 1.
        self.max_inflight = max(self.depth, int(setting("inflight", inflight, self.depth + (2 if many else 1), int)))
        self.warmup_steps = max(0, int(setting("warmup", warmup, 10, int)))
        self._t = 0                                        # launches so far (lane selection)
        self._steps = np.zeros(self.n, dtype=np.int64)     # windows seen by each stream slot
        # where finish() spends its time: waiting for the GPU vs clustering + output tail on the host
        self.host_seconds = {"wait": 0.0, "work": 0.0}
        self.tail: Optional[BatchedOutputTail] = None      # built at the first launch, when the frames per chunk are known
        self._sub: dict = {}                               # (S, lane) -> (segmentation handles, embedding handles, ...)
        self._slots: List[dict] = []
        self._warmed: set = set()
        self._warming, self._real_steps = False, 0       # (see _warm_up)
        self._real_launches = 0                          # launches issued for a caller (not by _warm_up)
        self._lib = _lib.load()
        self._ctx = _lib.context(self.device.index)

    def _host_wait(self, wait: Optional[str]) -> None:
        """How the host waits.  With cores to spare the launching thread spins on the step's `done` event (lowest
        latency) and the pool's workers poll 40 us for the next job; a rank that has ~2 cores for itself (8 ranks
        on a node's 16 usable cores) cannot afford either: the event is then a blocking one (the thread sleeps in
        the driver until the GPU signals) and the workers sleep at once.  ``wait`` = spin | block | auto."""
        from .config import setting
        from .hostinfo import usable_cores
        try:
            ranks_here = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
        except ValueError:
            ranks_here = 1
        self.cores_per_rank = usable_cores() / ranks_here
        mode = str(setting("wait", wait, "auto"))
        if mode not in ("auto", "spin", "block"):
            raise ValueError(f"{type(self).__name__}: wait={mode!r} (expected auto | spin | block)")
        self.blocking_wait = mode == "block" or (mode == "auto" and self.cores_per_rank < 4)
        # idle pool workers poll 40 us for the next job when this rank has cores to spare, else they sleep at once
        # (process-wide setting: the newest engine's situation decides)
        _lib.load().dz_host_pool_set_spin(0 if self.cores_per_rank < 4 else 40)

    def _refuse_xvector_experiments(self) -> None:
        """The experiment switches of the x-vector engine (experiments build only) mean nothing to its siblings."""
        who = type(self).__name__
        for name in ("DZ_SEG_FRONT", "DZ_SHARED_EMB", "DZ_CONV0_PAIR"):
            if _lib.exp_env(name, "0") != "0":
                raise ValueError(f"{who}: {name} is an experiment of the x-vector engine; it has no meaning here")
        if _lib.exp_env("DZ_ABLATE", ""):
            raise ValueError(f"{who}: DZ_ABLATE is an experiment of the x-vector engine; it has no meaning here")

    def launch(self, waves, starts=None, slots: Optional[Sequence[int]] = None) -> dict:
        """Enqueue the GPU work for one step.  ``waves``: (N, S) or (N, 1, S) float32 on the GPU
        (a strided rolling-window view is used in place) or an ``AudioRing`` holding a complete
        window.  ``starts``: start time in seconds of each
        stream's window (default: the number of windows that stream slot has seen since its last
        ``reset`` x ``step``), used by the output tail only.
        ``slots``: which of the ``num_streams`` clustering / tail states the rows belong to, for a
        step in which only some streams have a new window (``len(slots)`` rows; default: all, in
        order).  Returns a ticket for ``finish``; does not wait for the GPU."""
        ring = waves if isinstance(waves, AudioRing) else None
        if ring is not None:
            assert ring.filled == ring.window, "the ring does not hold a complete window yet"
            rows, N, S = None, ring.n, ring.window
            base, stride = ring.raw()
        else:
            rows = _as_rows(waves)
            N, S = rows.shape
            base, stride = rows.data_ptr(), (rows.stride(0) if N > 1 else S)
        if slots is None:
            assert N == self.n, f"expected {self.n} streams, got {N}"
        else:
            slots = [int(i) for i in slots]
            assert N == len(slots) and 1 <= N <= self.n and len(set(slots)) == N, "bad slots"
            assert all(0 <= i < self.n for i in slots), "slot out of range"
        slot = self._launch_rows(base, stride, N, S, rows, ring)
        slot["slots"] = slots
        idx = np.arange(self.n) if slots is None else np.asarray(slots, dtype=np.int64)
        slot["starts"] = self._steps[idx] * self.step if starts is None else starts
        self._steps[idx] += 1
        return slot

    def _prepare(self, S: int, shape: tuple) -> int:
        """The top of every ``_launch_rows`` -> the lane of this step.  Everything a window size allocates happens here,
        at its first launch and before its first kernel is enqueued; ``shape``: the step's slot shape, frames first."""
        if S not in self._warmed:
            # The scratch arenas of EVERY lane before the first kernel of this window size is enqueued
            # (~0.85 GB of hipMalloc + hipMemset per lane): no device allocation while kernels run.  (This
            # did NOT remove the 21 - 39 ms start-up stall some runs show in their third step — it persisted
            # with the arenas allocated up front; profiles/README.md)
            for lane in range(self.depth):
                self._handles(S, lane)
            # ... and the output tail's host state NOW, while the GPU is idle: built lazily in the first
            # finish() — 64 aggregation states (30 MB of fresh host memory, mapped and first touched) + 7.5 MB
            # of result buffers while two steps were on the GPU — it froze every resident kernel for 20 - 40 ms
            # (tools/stall_probe.py: gone when only this is moved; the first clustering call, which starts the
            # worker threads, is not the trigger).  This was the start-up stall of rounds 1 - 3.
            if self.tail is None:
                self.tail = self._make_tail(shape[0])
            # ... and the slots (the first take of a shape allocates all of them), then the warm-up.  One order for
            # every engine: the warm-up's own launches would allocate the slots anyway, before their first kernel.
            self._release(self._take_slot(shape))
            self._warmed.add(S)
            self._warm_up(S)
        if not self._warming:
            self._real_launches += 1
        return self._t % self.depth

    def _take_slot(self, shape: tuple) -> dict:
        """The first free slot of this shape, marked busy: a step's device and pinned result buffers and its events,
        the ticket ``launch`` returns.  A subclass's ``_new_slot(shape)`` supplies its own tensors and events."""
        pool = [s for s in self._slots if s["shape"] == shape]
        if not pool:
            # every in-flight slot up front: a pinned-memory allocation made while kernels are
            # running stalls the queues for tens of milliseconds (seen as one 40 ms "kernel" in the
            # rocprofv3 trace of the second step)
            pool = [self._add_slot(shape) for _ in range(self.max_inflight + self.lag)]
        slot = next((s for s in pool if not s["busy"]), None) or self._add_slot(shape)
        slot["busy"] = True
        return slot

    def _add_slot(self, shape: tuple) -> dict:
        stats = torch.empty((self.n, self._lib.dz_wave_stats_floats()), dtype=torch.float32, device=self.device)
        slot = dict(self._new_slot(shape), shape=shape, busy=False, stats=stats, ev_in=torch.cuda.Event(),
                    done=torch.cuda.Event(blocking=self.blocking_wait))
        if getattr(self, "_gallery", None) is not None:
            self._match_buffers(slot)
        self._slots.append(slot)
        return slot

    def _release(self, ticket: dict) -> None:
        """Hand a ticket's slot back to the pool.  EVERY path out of a step ends here: a slot left busy makes each
        later launch allocate a new pinned one while kernels are running."""
        ticket["busy"] = False
        ticket["keep"] = None

    @contextmanager
    def _host_half(self, ticket: dict):
        """The guarded host half of a step: wait for its GPU half, then the body, then the slot is ALWAYS handed back
        (an exception in the body used to leak it).  The range flag (an f16x3 operand beyond +-65504 is an error, not
        a clamp) is checked first: a flagged step's results are clamped garbage and must not reach the
        clustering state of the streams; the caller gets error 6 for THIS step and the streams
        skip one window.  The flag is one word per device: with `depth` steps in flight it may have
        been raised by a kernel of a later step, whose own finish() then passes — over-reporting by
        at most `depth - 1` steps, never under-reporting."""
        self._wait(ticket)
        t1 = _time.perf_counter()
        try:
            _lib.range_check(self.device.index)
            yield
        finally:
            self._release(ticket)
            self.host_seconds["work"] += _time.perf_counter() - t1

    def __del__(self):
        try:
            for hsegs, hembs, *_ in self._sub.values():
                for h in hsegs:
                    self.seg._destroy(h)
                for h in hembs:
                    self.emb._destroy(h)
        except Exception:
            pass

    def _warm_up(self, S: int) -> None:
        """A few overlapped steps on silence before the first real one of this window size.  Besides the
        start-up stall proper (the output tail's host buffers, allocated before the first launch: see
        `_prepare`), a fresh process shows two 7 - 12 ms intervals within its first ~8 steps
        (tools/stall_probe.py, no tracer; profiles/r03_f_stall_probe.txt): one-time set-up for the first
        launches of each kernel on each queue — gone after warm steps, while warming the streams, the copy
        path and the events alone did not move them.  Complete steps (GPU + host half: the worker pool's
        threads start here too) while no stream has any state yet, GPU-only steps for a second window size
        later on; ~0.1 s of construction time instead of latency spikes in a live stream.  ``warmup=<steps>``
        (0 = off).

        Complete steps (and the reset() that forgets them) only while NO launch has been issued for a caller:
        counting finished steps instead (round 3) let a second window size, or a first finish() that comes
        after several launches (FileBatch never calls finish), wipe the clustering / tail state and the
        step counters under tickets that were still in flight."""
        steps = self.warmup_steps
        if steps <= 0:
            return
        zeros = torch.zeros((self.n, S), dtype=torch.float32, device=self.device)
        saved = dict(self.host_seconds)
        inflight: List[dict] = []
        t_saved = self._t
        self._warming = True
        try:
            if self._real_launches == 0:                     # complete steps, then forget them
                for _ in range(steps):
                    inflight.append(self.launch(zeros))
                    if len(inflight) >= self.max_inflight:
                        self.finish(inflight.pop(0))
                while inflight:
                    self.finish(inflight.pop(0))
            else:                                            # GPU-only steps: no stream state is touched
                for _ in range(steps):
                    inflight.append(self._launch_rows(zeros.data_ptr(), zeros.stride(0), self.n, S, zeros))
                    if len(inflight) >= self.max_inflight:
                        self._wait(inflight[0])
                        self._release(inflight.pop(0))
                for t in inflight:
                    self._wait(t)
                    self._release(t)
        finally:
            self._warming = False
        torch.cuda.synchronize(self.device)
        if self._real_launches == 0:
            self.reset()
            self._t = 0
        else:
            self._t = t_saved
        self.host_seconds.update(saved)

    def _wait(self, ticket: dict) -> None:
        """Block until the GPU half of the step is done and its results are in pinned host memory."""
        t0 = _time.perf_counter()
        ticket["done"].synchronize()
        self.host_seconds["wait"] += _time.perf_counter() - t0

    def __call__(self, waves):
        return self.finish(self.launch(waves))


class _DiarizationEngine(_StepEngine):
    """The host half of the engines that diarize (``StreamBatch``, ``WeSpeakerBatch``): N clustering states and
    (``tail=True``) N aggregation / binarisation states, stepped on the C++ workers from a ticket's pinned
    segmentation scores and embeddings."""

    def __new__(cls, *args, **kwargs):
        # ``tau_offset=`` is refused by name by every engine that diarizes (StreamBatch, its GroupsBatch front door,
        # WeSpeakerBatch): hysteresis is VadBatch's and OverlapBatch's.  Here and not as a keyword of the ``__init__``s,
        # whose parameter lists are held equal to one another name by name (tests/test_wespeaker_engine_host.py): a
        # parameter that exists only to be refused does not belong in them.
        from .blocks.diarization import refuse_tau_offset
        refuse_tau_offset(kwargs, cls.__name__)
        return super().__new__(cls)

    def _setup_host(self, tau_active, rho_update, delta_new, gamma, beta, max_speakers, normalize_embedding_weights,
                    cluster_threads, tail, duration, step, latency) -> None:
        """The N clustering states and the parameters of the output tail (DelayedAggregation + Binarize of every stream,
        C++; built at the first launch, when the number of frames per chunk is known)."""
        self.gamma, self.beta, self.norm_w = float(gamma), float(beta), bool(normalize_embedding_weights)
        self.clustering = BatchedSpeakerClustering(self.n, tau_active, rho_update, delta_new, max_speakers,
                                                   cluster_threads)
        self.max_speakers, self.tau_active, self.cluster_threads = max_speakers, tau_active, cluster_threads
        self.with_tail, self.duration, self.step = bool(tail), float(duration), float(step)
        self.latency = self.step if latency is None else float(latency)
        self._gallery, self._names, self._gallery_handles = None, None, []     # (set_gallery)
        self._match_norm = False                # the gallery has a cohort: dz_gallery_match_norm, a signed delta_id

    def _make_tail(self, F: int) -> Optional[BatchedOutputTail]:
        if not self.with_tail:
            return None
        return BatchedOutputTail(self.n, F, self.max_speakers, self.step, self.latency, self.tau_active,
                                 num_threads=self.cluster_threads)

    def set_host_threads(self, n: int) -> int:
        """Host threads of the per-stream CPU stages (clustering, aggregation + binarisation) from now on."""
        n = max(1, int(n))
        self.cluster_threads = self.clustering.num_threads = n
        if self.tail is not None:
            self.tail.num_threads = n
        return n

    def reset(self, slot: Optional[int] = None):
        """Forget the clustering / aggregation state of every stream, or of one slot."""
        self.clustering.reset(slot)
        if self.tail is not None:
            self.tail.reset(slot)
        if self._names is not None:
            self._names.reset(slot)
        if slot is None:
            self._steps[:] = 0
        else:
            self._steps[slot] = 0

    # ------------------------------------------------------------------ speaker gallery
    def set_gallery(self, gallery, delta_id=None) -> None:
        """Name the speakers against ``gallery`` (a ``gallery.SpeakerGallery``) from the next launch on; ``None``
        removes it.  ``delta_id``: the largest cosine distance at which a match counts (no default: it depends on the
        embedding model).  With a gallery every launch enqueues one ``dz_gallery_match`` over the step's (N * K, D)
        embeddings, behind the embedding on the stream that carries the results to the host, its answers written to
        pinned memory by the kernel itself; ``finish`` adds ``ticket["match"] = (index, distance, second)``, each
        (N, K), and ``ticket["names"]``, per row a dict g -> name (``gallery.SpeakerNames`` after this step's
        assignment); ``diarize`` labels its turns with them.  Each lane gets a handle of its own (a device copy of the
        voiceprints + the scratch of one match).  Refused by name: a gallery of another dimension than the embedding's,
        or on another device.  Setting another gallery (or None) forgets every stream's names; call it with no step
        between ``launch`` and ``finish``.

        A gallery WITH A COHORT (``SpeakerGallery(..., cohort=...)``) is matched by ``dz_gallery_match_norm`` instead:
        ``ticket["match"]`` then carries the normalised distances (adaptive s-norm, ``csrc/k_cohort.hip``: signed, lower
        is closer), ``ticket["match_normalised"]`` is ``True`` and ``delta_id`` is a threshold on that quantity, any
        finite value.  The rule is the same; a gallery without a cohort takes the raw path and refuses a negative
        ``delta_id`` as before."""
        who = type(self).__name__
        if gallery is not None:
            from .gallery import SpeakerGallery, SpeakerNames, check_delta_id
            if not isinstance(gallery, SpeakerGallery):
                raise ValueError(f"{who}.set_gallery: expected a SpeakerGallery or None, got {type(gallery).__name__}")
            delta = check_delta_id(delta_id, f"{who}.set_gallery", signed=gallery.cohort is not None)
            if gallery.dimension != self.emb.dimension:
                raise ValueError(f"{who}.set_gallery: the gallery's voiceprints have dimension {gallery.dimension}, the "
                                 f"embedding model's embeddings {self.emb.dimension}")
            if gallery.device is not None and torch.device(gallery.device) != self.device:
                raise ValueError(f"{who}.set_gallery: the gallery is on {gallery.device}, the engine on {self.device}")
        if any(s["busy"] for s in self._slots):
            raise RuntimeError(f"{who}.set_gallery: a step is between launch and finish")
        torch.cuda.synchronize(self.device)               # no kernel of an older step reads the handles dropped here
        self._gallery, self._names, self._gallery_handles, self._match_norm = None, None, [], False
        for s in self._slots:
            s.pop("match_h", None)
            s.pop("match", None)
            s.pop("names", None)
            s["matched"] = False
        if gallery is None:
            return
        handles = [gallery.new_handle(self.device) for _ in range(self.depth)]
        self._match_norm = gallery.cohort is not None
        self._names = SpeakerNames(self.n, self.max_speakers, delta, signed=self._match_norm)
        self._gallery, self._gallery_handles = gallery, handles
        for s in self._slots:
            self._match_buffers(s)

    def _match_buffers(self, slot: dict) -> None:
        """A slot's pinned (index | distance | second) rows, (3, N, K) of 4-byte values."""
        n, K = slot["emb"].shape[:2]
        slot["match_h"] = torch.empty((3, n, K), dtype=torch.int32).pin_memory()
        slot["matched"] = False

    def _enqueue_match(self, slot: dict, ln: int, N: int, stream) -> None:
        """One nearest-voiceprint search over the step's N * K embeddings on ``stream``, behind the embedding; the
        kernel writes its answers to the slot's pinned rows (no copy call: csrc/ring.hip, dz_results_to_host)."""
        K, D = slot["emb"].shape[1:]
        m = slot["match_h"]
        h = self._gallery_handles[ln]
        (h.match_norm if self._match_norm else h.match)(slot["emb"].data_ptr(), D, N * K, m[0].data_ptr(),
                                                        m[1].data_ptr(), m[2].data_ptr(), stream.cuda_stream)
        slot["matched"] = True

    def finish(self, ticket: dict, want_scores: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Wait for the step's GPU work, run the N clustering updates.
        -> (segmentation (N,F,K) f32, embeddings (N,K,D) f32, scores (N,F,G) f64 | None, assign (N,K)).
        The arrays (and ``ticket["tail"]``) are views of buffers that a later ``launch`` / ``finish``
        reuses: copy what has to outlive the next step."""
        if not self._warming:
            self._real_steps += 1
        with self._host_half(ticket):
            N, slots = ticket["rows"], ticket["slots"]
            seg = ticket["seg_h"].numpy()[:N]
            emb = ticket["emb_h"].numpy()[:N]
            scores, assign = self.clustering(seg, emb, want_scores or self.with_tail, slots=slots)
            if self.with_tail:
                # diarization.py:190,203-232 for every stream: aggregate the overlapping windows of the
                # region [t - latency, t - latency + step) and binarise it
                if self.tail is None:
                    self.tail = self._make_tail(seg.shape[1])
                ticket["tail"] = self.tail(scores, ticket["starts"], self.duration / seg.shape[1], slots=slots)
            if self._gallery is not None and ticket.get("matched"):
                m = ticket["match_h"].numpy()
                ticket["match"] = (m[0, :N], m[1, :N].view(np.float32), m[2, :N].view(np.float32))
                ticket["match_normalised"] = self._match_norm
                self._names.update(assign, ticket["match"][0], ticket["match"][1], slots)
                ticket["names"] = self._names.labels(self._gallery.names, slots)
        return seg, emb, scores, assign

    def diarize(self, waves: torch.Tensor, starts=None):
        """One step of every stream, end to end: -> list of N ``Annotation`` (the speech turns of the
        region this step finalises, what ``SpeakerDiarization.__call__`` returns per chunk) —
        requires ``tail=True``."""
        assert self.with_tail, f"construct {type(self).__name__}(tail=True)"
        ticket = self.launch(waves, starts)
        self.finish(ticket, want_scores=False)
        _, _, _, _, turns, nturns = ticket["tail"]
        names = ticket["names"] if self._gallery is not None else [None] * self.n
        return [BatchedOutputTail.annotation(turns[i], int(nturns[i]), names=names[i]) for i in range(self.n)]


class StreamBatch(_DiarizationEngine):
    xvector_experiments = True

    def __new__(cls, segmentation=None, embedding=None, *args, **kwargs):
        # The front door of the groups form too: its callers construct ``StreamBatch(seg, emb, n, ...)``.  What comes
        # back then is a GroupsBatch, no StreamBatch, so Python does not call StreamBatch.__init__ on it.
        if cls is StreamBatch and isinstance(embedding, _HipGroupsEmbedding):
            return GroupsBatch(segmentation, embedding, *args, **kwargs)
        return super().__new__(cls, **kwargs)     # (_DiarizationEngine.__new__ looks at the keywords)

    def __init__(self, segmentation: HipSegmentation, embedding: HipEmbedding, num_streams: int,
                 tau_active: float = 0.6, rho_update: float = 0.3, delta_new: float = 1.0,
                 gamma: float = 3, beta: float = 10, max_speakers: int = 20,
                 normalize_embedding_weights: bool = False,
                 device: Optional[torch.device] = None, cluster_threads: int = 8,
                 seg_split: Optional[int] = None, emb_split: Optional[int] = None,
                 tail: bool = False, duration: float = 5.0, step: float = 0.5,
                 latency: Optional[float] = None, depth: Optional[int] = None, *, lanes: Optional[int] = None,
                 recurrence: Optional[str] = None, inflight: Optional[int] = None, wait: Optional[str] = None,
                 warmup: Optional[int] = None, serial: bool = False):
        """Engine parameters (``DZ_ENGINE`` overrides them, config.py):
        ``lanes`` (= ``depth``): steps the GPU works on at once, each with its own HIP streams, handles and scratch
        arenas (~0.85 GB per lane at 64 streams) — default 2, or ``THROUGHPUT_LANES`` for a throughput engine;
        ``recurrence``: the LSTM recurrence kernel, "valu" | "0" | "3" | "4" — default: the matrix-core kernel of
        ``weights.THROUGHPUT_LSTM_VARIANT`` for a throughput engine (>= 64 streams per step, default precision),
        else the model's own;
        ``inflight``: steps a throughput caller keeps between ``launch`` and ``finish`` (default lanes + 1; lanes + 2 for a
        throughput engine);
        ``wait``: how the host waits for a step, "spin" | "block" | "auto" (by the cores this rank has);
        ``warmup``: warm steps on silence before the first real step of a window size (default 10, 0 = off);
        ``serial``: MEASUREMENT engine — one lane whose segmentation and embedding chains share ONE HIP stream, so
        that no two kernels ever overlap and a kernel's bracketed duration is its alone-time (what
        ``rocprofv3 --kernel-trace --stats`` of the same run reports): ``bench.py``'s roofline pass.

        With a groups-form ``embedding`` (ECAPA-TDNN, speechbrain x-vector, TitaNet-L, speechbrain ResNet, mel-spectrogram ECAPA) this call constructs a
        ``GroupsBatch``: see there."""
        if isinstance(embedding, HipWeSpeakerEmbedding):
            raise ValueError("StreamBatch does not run the WeSpeaker ResNet34 embedding; it runs "
                             "HipEmbedding (pyannote/embedding), HipEcapaEmbedding (speechbrain/spkrec-ecapa-voxceleb) and "
                             "HipSbXvectorEmbedding (speechbrain/spkrec-xvect-voxceleb). "
                             "Use WeSpeakerBatch (the N-stream engine of pyannote/wespeaker-voxceleb-resnet34-LM)")
        # sub-batches per network, each on its own HIP stream with its own scratch arena: the
        # x-projection GEMM of one sub-batch runs under the latency-bound recurrence of another
        self.seg_split = max(1, min(int(_lib.exp_env("DZ_SEG_SPLIT", "1") if seg_split is None else seg_split), num_streams))
        self.emb_split = max(1, min(int(_lib.exp_env("DZ_EMB_SPLIT", "1") if emb_split is None else emb_split), num_streams))
        if depth is not None and lanes is not None and int(depth) != int(lanes):
            raise ValueError(f"StreamBatch: depth={depth} and lanes={lanes} name the same thing")
        self._setup(segmentation, embedding, num_streams, device, lanes=lanes if lanes is not None else depth,
                    recurrence=recurrence, inflight=inflight, wait=wait, warmup=warmup, lanes_follow_recurrence=True)
        self._setup_host(tau_active, rho_update, delta_new, gamma, beta, max_speakers, normalize_embedding_weights,
                         cluster_threads, tail, duration, step, latency)
        # HIP stream priorities (0 normal, -1 high).  The segmentation chain is the long dependent one
        # (4 recurrences + their projections: ~2.2 ms in the pipeline, two lanes): its streams get the
        # high priority — round 3, two same-visit pairs: 1.215 vs 1.233 and 1.159 vs 1.180 ms per step
        # (gpurun_out/visit_r3l.log; in round 2, with longer small kernels in that chain, the effect was
        # inside the noise).  The embedding chain waits for the segmentation anyway and stays normal.
        pa, pb = int(_lib.exp_env("DZ_PRIO_A", "-1")), int(_lib.exp_env("DZ_PRIO_B", "0"))
        # DZ_SHARED_EMB=1: ONE set of embedding streams serves every lane in step order and the
        # pooling of step t is enqueued `lag` = depth - 1 launches later, behind the frame features
        # of the following steps (only the last two kernels of the embedding network wait for the
        # segmentation; by then it has finished, so the stream never blocks on it).  That is what a
        # latency-heavy segmentation needs (the matrix-core recurrence, DZ_LSTM=0..3, with depth >= 3:
        # fewer streams than lanes x 2, the runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware
        # queues).  With the default recurrence kernel two full lanes measured 8 % faster (24.7 k vs
        # 22.8 k xRT), so the default is one embedding stream per lane.
        # DZ_ABLATE=noemb | noseg: TIMING EXPERIMENT (results are wrong): one of the two networks is not launched,
        # to see what the step costs when the other one has the chip to itself
        self._ablate = _lib.exp_env("DZ_ABLATE", "")
        self.shared_stats = _lib.exp_env("DZ_SHARED_STATS", "1") != "0"
        self.shared_emb = _lib.exp_env("DZ_SHARED_EMB", "0") != "0"
        self.lag = self.depth - 1 if self.shared_emb else 0
        # DZ_SEG_FRONT=1: the stateless front half of the segmentation network (SincNet + the first
        # x-projection, dz_seg_front) gets a stream of its own per lane.  launch(t + depth) is called
        # before finish(t), so on one stream the front half of step t + depth queues BEHIND the
        # recurrences of step t; on its own stream it runs under them and the lane's dependent chain is
        # the back half only (dz_seg_back: 4 recurrences, 3 projections, the MLP head).
        self.seg_front = _lib.exp_env("DZ_SEG_FRONT", "0") != "0"
        pf = int(_lib.exp_env("DZ_PRIO_F", "0"))
        mk = lambda prio, k: [torch.cuda.Stream(self.device, priority=prio) for _ in range(k)]
        shared_b = mk(pb, self.emb_split) if self.shared_emb else None
        self.lanes = [dict(a=mk(pa, self.seg_split), b=shared_b or mk(pb, self.emb_split),
                           f=mk(pf, self.seg_split) if self.seg_front else None)
                      for _ in range(self.depth)]
        self.serial = bool(serial)
        if self.serial:
            if self.depth != 1 or self.seg_split != 1 or self.emb_split != 1 or self.seg_front:
                raise ValueError("StreamBatch(serial=True) is one lane with one stream: lanes=1, no sub-batches")
            self.lanes[0]["b"] = self.lanes[0]["a"]
        self.streams_a, self.streams_b = self.lanes[0]["a"], self.lanes[0]["b"]
        self.stream_a, self.stream_b = self.streams_a[0], self.streams_b[0]
        self.num_hip_streams = self.depth * self.seg_split + self.emb_split * (1 if self.shared_emb else self.depth)
        # DZ_CONV0_PAIR=1 (experiments build): the first SincNet stage of BOTH networks in one launch
        # (dz_sinc_conv0_pair: one split of the normalised window, 160 filters, one parking of the samples) on the
        # lane's first segmentation stream, the embedding stream waits for it.  Correct, and slower: 1.23 vs 1.15 ms
        # per step (csrc/k_front.hip has the numbers).
        self.conv0_pair = (_lib.exp_env("DZ_CONV0_PAIR", "0") == "1" and self.shared_stats
                           and getattr(self.seg, "precision", "") == "f16x3" and getattr(self.emb, "precision", "") == "f16x3"
                           and self.seg_split == 1 and self.emb_split == 1 and not self.seg_front and not self._ablate
                           and hasattr(self.emb, "_state") and type(self.emb).__name__ == "HipEmbedding")
        self._pair = None                                  # PackedConv0Pair, built at the first launch
        self._pending: List[dict] = []                     # launched, pooling not enqueued yet
        # measurement (bench.py sets it to a list): launches that took the host more than 2 ms, by the call they sat in
        self.slow_launches: Optional[list] = None
        self.d2h_by_kernel = True          # (False: the hipMemcpyAsync pair, kept for the A/B of profiles/r06z_launch_stalls.json)

    # ------------------------------------------------------------------ GPU half
    def _new_slot(self, shape: tuple) -> dict:
        (F, K, D), n, dev = shape, self.n, self.device
        return dict(seg=torch.empty((n, F, K), dtype=torch.float32, device=dev),
                    w=torch.empty((n, K, F), dtype=torch.float32, device=dev),
                    emb=torch.empty((n, K, D), dtype=torch.float32, device=dev),
                    seg_h=torch.empty((n, F, K), dtype=torch.float32).pin_memory(),
                    emb_h=torch.empty((n, K, D), dtype=torch.float32).pin_memory(),
                    ev_seg=[torch.cuda.Event() for _ in range(self.seg_split)],
                    ev_front=[torch.cuda.Event() for _ in range(self.seg_split)],
                    ev_emb=[torch.cuda.Event() for _ in range(self.emb_split - 1)],
                    ev_frames=[torch.cuda.Event() for _ in range(self.emb_split)],
                    ev_conv0=torch.cuda.Event())

    @staticmethod
    def _ranges(n: int, parts: int) -> List[Tuple[int, int]]:
        return [(n * i // parts, n * (i + 1) // parts) for i in range(parts)]

    def _handles(self, S: int, lane: int):
        """C handles (one scratch arena each, owned by this object) of the sub-batches of one lane
        for windows of S samples."""
        got = self._sub.get((S, lane))
        if got is None:
            sa, sb = self._ranges(self.n, self.seg_split), self._ranges(self.n, self.emb_split)
            hs = [self.seg._create(S, max(1, -(-self.n // self.seg_split)), throughput=self.throughput,
                                   recurrence=None if self.throughput else self.recurrence) for _ in sa]
            he = [self.emb._create(S, max(1, -(-self.n // self.emb_split))) for _ in sb]
            got = self._sub[(S, lane)] = (hs, he, sa, sb)
        return got

    def _launch_rows(self, base: int, stride: int, N: int, S: int, keep=None, ring: Optional[AudioRing] = None) -> dict:
        """The GPU half of a step for N <= num_streams rows of S samples at ``base + i * stride``
        floats: segmentation (+ OSP weights) and frame features on this step's lane, pooling behind
        them.  Knows nothing about which stream / file a row belongs to (``launch`` and ``FileBatch``
        decide that)."""
        assert 1 <= N <= self.n
        F, K, D = self.seg.num_frames(S), self.seg.num_speakers, self.emb.dimension
        ln = self._prepare(S, (F, K, D))
        lane = self.lanes[ln]
        hsegs, hembs, _, _ = self._handles(S, ln)
        marks = [("start", _time.perf_counter())] if self.slow_launches is not None else None
        # sub-batch ranges of THIS step's rows (each at most the capacity its handle was built for)
        sa, sb = self._ranges(N, self.seg_split), self._ranges(N, self.emb_split)
        slot = self._take_slot((F, K, D))
        lib, esz = self._lib, 4
        cur = torch.cuda.current_stream(self.device)
        slot["ev_in"].record(cur)                       # inputs produced on the caller's stream
        # InstanceNorm1d(1) statistics of the windows ONCE for both networks (each SincNet would
        # otherwise make its own pass over the same 20 MB).  They go first on the lane's first
        # segmentation stream — the high-priority one: on the caller's (normal-priority) stream this 14 us
        # kernel sat 60 - 130 us in the queue in front of BOTH chains — and every other stream of the
        # step waits for `ev_in` re-recorded behind it.
        stats = slot["stats"] if self.shared_stats else None
        front = lane["f"]                               # None: both halves on the `a` streams
        if stats is not None:
            a0 = (front or lane["a"])[0]
            a0.wait_event(slot["ev_in"])
            _lib.check(lib.dz_wave_stats(self._ctx, base, stride, N, S, stats.data_ptr(), a0.cuda_stream),
                       "dz_wave_stats")
            slot["ev_in"].record(a0)
            if marks is not None:
                marks.append(("wave_stats", _time.perf_counter()))
        pair = self.conv0_pair and stats is not None
        if pair:
            if self._pair is None:
                from .weights import PackedConv0Pair
                self._pair = PackedConv0Pair(self.seg._state, self.emb._state, self.device)
            a0 = lane["a"][0]
            _lib.check(lib.dz_sinc_conv0_pair(hsegs[0], hembs[0], base, stride, N, stats.data_ptr(),
                                              self._pair.planes.data_ptr(), self._pair.bsum.data_ptr(), a0.cuda_stream),
                       "dz_sinc_conv0_pair")
            slot["ev_conv0"].record(a0)
        for j, ((i0, i1), h, a, ev) in enumerate(zip(sa, hsegs, lane["a"], slot["ev_seg"])):
            a.wait_event(slot["ev_in"])
            if i1 == i0:                                 # fewer rows than sub-batches
                ev.record(a)
                continue
            if stats is not None:
                _lib.check(lib.dz_seg_use_wave_stats(h, stats[i0:].data_ptr()), "dz_seg_use_wave_stats")
            if front is not None:
                f = front[j]
                f.wait_event(slot["ev_in"])
                _lib.check(lib.dz_seg_front(h, base + i0 * stride * esz, stride, i1 - i0, f.cuda_stream),
                           "dz_seg_front")
                slot["ev_front"][j].record(f)
                a.wait_event(slot["ev_front"][j])
                _lib.check(lib.dz_seg_back(h, i1 - i0, slot["seg"][i0:i1].data_ptr(), self.gamma, self.beta,
                                           int(self.norm_w), slot["w"][i0:i1].data_ptr(), a.cuda_stream),
                           "dz_seg_back")
                ev.record(a)
                continue
            if self._ablate == "noseg":
                ev.record(a)
                continue
            # segmentation + the OSP weights of its output (one launch sequence, no dz_osp of its own)
            _lib.check(lib.dz_seg_forward_osp(h, base + i0 * stride * esz, stride, i1 - i0,
                                              slot["seg"][i0:i1].data_ptr(), self.gamma, self.beta,
                                              int(self.norm_w), slot["w"][i0:i1].data_ptr(), a.cuda_stream),
                       "dz_seg_forward_osp")
            ev.record(a)
            if marks is not None:
                marks.append(("seg_forward_osp", _time.perf_counter()))
        for (i0, i1), h, b, ev in zip(sb, hembs, lane["b"], slot["ev_frames"]):
            b.wait_event(slot["ev_conv0"] if pair else slot["ev_in"])
            if i1 > i0 and self._ablate != "noemb":
                if stats is not None:
                    _lib.check(lib.dz_emb_use_wave_stats(h, stats[i0:].data_ptr()), "dz_emb_use_wave_stats")
                _lib.check(lib.dz_emb_frames(h, base + i0 * stride * esz, stride, i1 - i0, b.cuda_stream),
                           "dz_emb_frames")
            ev.record(b)
            if marks is not None:
                marks.append(("emb_frames", _time.perf_counter()))
        slot["rows"], slot["slots"] = N, None
        slot["keep"] = keep                              # keep the view alive until the GPU is done
        slot["pool"] = (lane, hembs, sa, sb, N, K, F)     # what _enqueue_pool needs
        slot["ln"] = ln
        if ring is not None:                            # pushes `slack` steps from now wait for these
            ring._read_by(list(lane["a"]) + list(lane["b"]) + list(front or []))
        self._pending.append(slot)
        while len(self._pending) > self.lag:
            self._enqueue_pool(self._pending.pop(0))
        if marks is not None:
            marks.append(("pool", _time.perf_counter()))
            if marks[-1][1] - marks[0][1] > 2e-3:           # a launch that took more than 2 ms: where
                self.slow_launches.append([self._t] + [(b[0], round(1e3 * (b[1] - a[1]), 2)) for a, b in zip(marks, marks[1:])])
        self._t += 1
        return slot

    def _enqueue_pool(self, slot: dict):
        """Statistics pooling + Linear + normalisation of a launched step (they consume the OSP
        weights, i.e. wait for its segmentation), the copy of its results to pinned memory and its
        `done` event, on the embedding stream(s)."""
        lane, hembs, sa, sb, N, K, F = slot["pool"]
        lib = self._lib
        for (i0, i1), h, b in zip(sb, hembs, lane["b"]):
            if i1 == i0:
                continue
            for (j0, j1), ev in zip(sa, slot["ev_seg"]):
                if j0 < i1 and i0 < j1:
                    b.wait_event(ev)
            if self._ablate == "noemb":
                if not slot.get("_filled"):       # something the clustering accepts
                    with torch.cuda.stream(b):
                        slot["emb"].fill_(0.04)
                    slot["_filled"] = True
                continue
            _lib.check(lib.dz_emb_pool(h, slot["w"][i0:i1].data_ptr(), i1 - i0, K, F, 1,
                                       slot["emb"][i0:i1].data_ptr(), b.cuda_stream), "dz_emb_pool")
        tr = self.slow_launches is not None
        m0 = _time.perf_counter() if tr else 0.0
        b0 = lane["b"][0]
        for b, ev in zip(lane["b"][1:], slot["ev_emb"]):
            ev.record(b)
            b0.wait_event(ev)
        # Results -> pinned memory by a kernel of our own.  The two hipMemcpyAsync (tensor.copy_) that stood here
        # blocked the launching thread for a whole step's latency about once per 150 steps (csrc/ring.hip).
        D = slot["emb"].shape[2]
        if self._gallery is not None:
            self._enqueue_match(slot, slot["ln"], N, b0)
        if self.d2h_by_kernel:
            _lib.check(lib.dz_results_to_host(self._ctx, slot["seg"].data_ptr(), slot["seg_h"].data_ptr(), N * F * K,
                                              slot["emb"].data_ptr(), slot["emb_h"].data_ptr(), N * K * D,
                                              b0.cuda_stream), "dz_results_to_host")
        else:
            with torch.cuda.stream(b0):
                slot["seg_h"][:N].copy_(slot["seg"][:N], non_blocking=True)
                slot["emb_h"][:N].copy_(slot["emb"][:N], non_blocking=True)
        m2 = _time.perf_counter() if tr else 0.0
        slot["done"].record(b0)
        if tr and _time.perf_counter() - m0 > 2e-3:
            self.slow_launches.append(["pool tail", ("results to host", round(1e3 * (m2 - m0), 2)),
                                       ("record done", round(1e3 * (_time.perf_counter() - m2), 2))])
        slot["pool"] = None

    # ------------------------------------------------------------------ host half
    def _wait(self, ticket: dict) -> None:
        """Block until the GPU half of the step is done and its results are in pinned host memory."""
        t0 = _time.perf_counter()
        while ticket["pool"] is not None:               # its pooling is still held back: flush in order
            self._enqueue_pool(self._pending.pop(0))
        ticket["done"].synchronize()
        self.host_seconds["wait"] += _time.perf_counter() - t0


class VadBatch(_StepEngine):
    """``VoiceActivityDetection`` of N concurrent streams, one chunk each per step: the segmentation-only form of the
    N-stream engine.  Per stream it produces what that stream's own ``VoiceActivityDetection`` (blocks/vad.py,
    reference ``blocks/vad.py:136-191``) produces: the speech track ``max over speakers`` of the segmentation and the
    ``"speech"`` turns of the region the step finalises (``DelayedAggregation(hamming, loose)`` + ``Binarize``).

    GPU schedule per step, on the step's lane (one HIP stream):

        dz_wave_stats -> dz_seg_forward_vad (the head kernel writes the (N,F) track beside the scores)
                      -> dz_results_to_host (the track only) -> `done`
        host          : aggregation + binarisation of step t-1 (C++ threads, fp64) while the GPU runs step t

    No embedding network and no clustering: the step is the segmentation chain alone.  The engine choices are
    ``StreamBatch``'s (``lanes``, ``recurrence``, ``inflight``, ``wait``, ``warmup``, ``DZ_ENGINE``): with >= 64
    streams in the default precision the matrix-core recurrence on ``THROUGHPUT_LANES`` lanes.  ``host_threads``:
    threads of the output tail.  ``tau_offset``: hysteresis (``dz_tail_set_offset``) — a frame of a stream stays on while
    its aggregated score is > ``tau_offset``; the state is per stream, crosses the steps and is cleared by
    ``reset(slot)``.  None: the single threshold."""

    LABEL = "speech"            # what the turns of `detect` are called (OverlapBatch: "overlap")

    def __init__(self, segmentation: HipSegmentation, num_streams: int, tau_active: float = 0.6,
                 duration: float = 5.0, step: float = 0.5, latency: Optional[float] = None,
                 device: Optional[torch.device] = None, *, lanes: Optional[int] = None,
                 recurrence: Optional[str] = None, inflight: Optional[int] = None, wait: Optional[str] = None,
                 warmup: Optional[int] = None, host_threads: int = 8, serial: bool = False,
                 tau_offset: Optional[float] = None):
        from .blocks.base import check_tau_offset
        self.tau_offset = check_tau_offset(tau_offset, type(self).__name__)      # (before the GPU is touched)
        if serial:
            raise ValueError("VadBatch: serial=True is the measurement engine of StreamBatch (bench.py's roofline "
                             "pass); the VAD engine has no serial form")
        self._timing(duration, step, latency)
        # the engine StreamBatch would pick for these streams: a throughput engine at >= 64 streams in the default
        # precision runs the matrix-core recurrence on THROUGHPUT_LANES lanes
        self._setup(segmentation, None, num_streams, device, lanes=lanes, recurrence=recurrence, inflight=inflight,
                    wait=wait, warmup=warmup, lanes_follow_recurrence=True)
        self.tau_active, self.host_threads = float(tau_active), max(1, int(host_threads))
        # the segmentation chain is the whole step: its streams get the high priority, as in StreamBatch
        pa = int(_lib.exp_env("DZ_PRIO_A", "-1"))
        self.lanes = [torch.cuda.Stream(self.device, priority=pa) for _ in range(self.depth)]

    def set_host_threads(self, n: int) -> int:
        """Host threads of the output tail (aggregation + binarisation) from now on."""
        self.host_threads = max(1, int(n))
        if self.tail is not None:
            self.tail.num_threads = self.host_threads
        return self.host_threads

    def reset(self, slot: Optional[int] = None):
        """Forget the aggregation state of every stream, or of one slot."""
        if self.tail is not None:
            self.tail.reset(slot)
        if slot is None:
            self._steps[:] = 0
        else:
            self._steps[slot] = 0

    # ------------------------------------------------------------------ GPU half
    def _handles(self, S: int, lane: int):
        got = self._sub.get((S, lane))
        if got is None:
            got = self._sub[(S, lane)] = ([self.seg._create(S, self.n, throughput=self.throughput,
                                                            recurrence=None if self.throughput else self.recurrence)], [])
        return got

    def _make_tail(self, F: int) -> BatchedOutputTail:
        return BatchedOutputTail(self.n, F, 1, self.step, self.latency, self.tau_active,
                                 strategy="hamming", cropping_mode="loose", num_threads=self.host_threads,
                                 offset=self.tau_offset)

    def _new_slot(self, shape: tuple) -> dict:
        (F,), n, dev, K = shape, self.n, self.device, self.seg.num_speakers
        return dict(seg=torch.empty((n, F, K), dtype=torch.float32, device=dev),
                    vad=torch.empty((n, F), dtype=torch.float32, device=dev),
                    vad_h=torch.empty((n, F), dtype=torch.float32).pin_memory())

    def _launch_rows(self, base: int, stride: int, N: int, S: int, keep=None, ring: Optional[AudioRing] = None) -> dict:
        assert 1 <= N <= self.n
        F = self.seg.num_frames(S)
        lane = self._prepare(S, (F,))
        a, (h,) = self.lanes[lane], self._handles(S, lane)[0]
        slot = self._take_slot((F,))
        lib = self._lib
        slot["ev_in"].record(torch.cuda.current_stream(self.device))      # inputs produced on the caller's stream
        a.wait_event(slot["ev_in"])
        stats = slot["stats"]
        _lib.check(lib.dz_wave_stats(self._ctx, base, stride, N, S, stats.data_ptr(), a.cuda_stream), "dz_wave_stats")
        _lib.check(lib.dz_seg_use_wave_stats(h, stats.data_ptr()), "dz_seg_use_wave_stats")
        self._forward_track(h, base, stride, N, slot, a)
        _lib.check(lib.dz_results_to_host(self._ctx, slot["vad"].data_ptr(), slot["vad_h"].data_ptr(), N * F,
                                          None, None, 0, a.cuda_stream), "dz_results_to_host")
        slot["done"].record(a)
        if ring is not None:                            # pushes `slack` steps from now wait for this forward
            ring._read_by([a])
        slot["rows"], slot["slots"], slot["keep"] = N, None, keep
        self._t += 1
        return slot

    def _forward_track(self, h, base: int, stride: int, N: int, slot: dict, a) -> None:
        """The step's forward pass on lane stream ``a``: scores -> slot["seg"], the (N,F) track -> slot["vad"]."""
        _lib.check(self._lib.dz_seg_forward_vad(h, base, stride, N, slot["seg"].data_ptr(), slot["vad"].data_ptr(),
                                                a.cuda_stream), "dz_seg_forward_vad")

    # ------------------------------------------------------------------ host half
    def finish(self, ticket: dict) -> np.ndarray:
        """Wait for the step's GPU work and run the N output tails -> the speech track (N,F,1) f32; the step's turns
        are in ``ticket["tail"]`` (``BatchedOutputTail.__call__``'s tuple, indexed by row).  Both are views of
        buffers that a later ``launch`` / ``finish`` reuses."""
        with self._host_half(ticket):
            N, slots = ticket["rows"], ticket["slots"]
            track = ticket["vad_h"].numpy()[:N, :, None]
            ticket["tail"] = self.tail(track, ticket["starts"], self.duration / track.shape[1], slots=slots)
        return track

    def detect(self, waves, starts=None) -> List[Annotation]:
        """One step of every stream, end to end -> N ``Annotation``: the ``"speech"`` turns of the region this step
        finalises (what ``VoiceActivityDetection.__call__`` returns per chunk, without the aggregated audio)."""
        ticket = self.launch(waves, starts)
        self.finish(ticket)
        turns, nturns = ticket["tail"][4], ticket["tail"][5]
        return [BatchedOutputTail.annotation(turns[i], int(nturns[i]), label=self.LABEL) for i in range(self.n)]


class OverlapBatch(VadBatch):
    """``OverlappedSpeechDetection`` of N concurrent streams: ``VadBatch``'s step with the head kernel writing the
    overlap track — per frame the second largest of the speaker scores, NaN ordered above every number
    (``dz_seg_forward_track`` with ``DZ_TRACK_OVERLAP``) — in place of the max, and turns labelled ``"overlap"``.
    Per stream it produces what that stream's own ``OverlappedSpeechDetection`` (blocks/osd.py) produces.  Only the
    (N,F) track travels to the host; ``launch`` / ``finish`` / ``reset`` / ``detect``, the rings, ``slots=`` and the
    lane choices are ``VadBatch``'s.  A model with one speaker has no overlap: ``ValueError``."""

    LABEL = "overlap"

    def __init__(self, segmentation: HipSegmentation, num_streams: int, tau_active: float = 0.5, *args, **kwargs):
        super().__init__(segmentation, num_streams, tau_active, *args, **kwargs)
        if int(self.seg.num_speakers) < 2:       # (known once the weights are on the device; no handle exists yet)
            raise ValueError(f"OverlapBatch: a segmentation model with {self.seg.num_speakers} speaker has no overlap "
                             "track (at least 2 speakers)")

    def _forward_track(self, h, base: int, stride: int, N: int, slot: dict, a) -> None:
        _lib.check(self._lib.dz_seg_forward_track(h, base, stride, N, slot["seg"].data_ptr(), slot["vad"].data_ptr(),
                                                  _lib.TRACK_OVERLAP, a.cuda_stream), "dz_seg_forward_track")


class _TwoChainEngine(_DiarizationEngine):
    """The engine of the embeddings that run as two chains per step, two HIP streams per lane:

        stream A : dz_wave_stats -> dz_seg_forward_osp (scores + OSP weights)            -- ev_seg
        stream B : the model's early launch (reads the windows)   <wait ev_seg>   its late launch (consumes the OSP
                   weights, normalised) -> dz_results_to_host (scores + embeddings) -> `done`
        host     : clustering + output tail of step t-1 (C++ workers, fp64) while the GPU runs step t

    The model says what the two launches are and how many rows its handle holds (``engine_rows``, ``early_launch``,
    ``late_launch``).  Two lanes whatever the recurrence (an embedding handle per lane is gigabytes of arena; 4 HIP
    streams are what the runtime's 4 hardware queues carry), ``inflight`` = lanes + 1; the other engine parameters are
    ``StreamBatch``'s.  No sub-batches and none of the x-vector engine's experiment switches."""

    def __init__(self, segmentation: HipSegmentation, embedding, num_streams: int,
                 tau_active: float = 0.6, rho_update: float = 0.3, delta_new: float = 1.0,
                 gamma: float = 3, beta: float = 10, max_speakers: int = 20,
                 normalize_embedding_weights: bool = False,
                 device: Optional[torch.device] = None, cluster_threads: int = 8,
                 seg_split: Optional[int] = None, emb_split: Optional[int] = None,
                 tail: bool = False, duration: float = 5.0, step: float = 0.5,
                 latency: Optional[float] = None, depth: Optional[int] = None, *, lanes: Optional[int] = None,
                 recurrence: Optional[str] = None, inflight: Optional[int] = None, wait: Optional[str] = None,
                 warmup: Optional[int] = None, serial: bool = False):
        who = type(self).__name__
        for name, split in (("seg_split", seg_split), ("emb_split", emb_split)):
            if split not in (None, 1):
                raise ValueError(f"{who}: {name}={split} (the embedding's forward is one launch sequence over every "
                                 f"stream's rows: {name} must be 1)")
        if depth is not None and lanes is not None and int(depth) != int(lanes):
            raise ValueError(f"{who}: depth={depth} and lanes={lanes} name the same thing")
        # the recurrence StreamBatch would pick for these streams; the lanes stay at 2 (memory, queues)
        self._setup(segmentation, embedding, num_streams, device, lanes=lanes if lanes is not None else depth,
                    recurrence=recurrence, inflight=inflight, wait=wait, warmup=warmup, lanes_follow_recurrence=False)
        self._setup_host(tau_active, rho_update, delta_new, gamma, beta, max_speakers, normalize_embedding_weights,
                         cluster_threads, tail, duration, step, latency)
        if serial and self.depth != 1:
            raise ValueError(f"{who}(serial=True) is one lane with one stream: lanes=1")
        # the step's last kernels wait for the segmentation: its stream keeps StreamBatch's high priority, so that it is
        # never queued behind the embedding networks of both lanes
        self.lanes = [dict(a=torch.cuda.Stream(self.device, priority=-1), b=torch.cuda.Stream(self.device, priority=0))
                      for _ in range(self.depth)]
        if serial:                                      # the measurement form: no two kernels ever overlap
            self.lanes[0]["b"] = self.lanes[0]["a"]
        self.num_hip_streams = 2 * self.depth

    # ------------------------------------------------------------------ GPU half
    def _handles(self, S: int, lane: int):
        got = self._sub.get((S, lane))
        if got is None:
            hs = self.seg._create(S, self.n, throughput=self.throughput,
                                  recurrence=None if self.throughput else self.recurrence)
            try:
                he = self.emb._create(S, self.emb.engine_rows(self.n, self.seg.num_speakers))
            except Exception:
                self.seg._destroy(hs)
                raise
            got = self._sub[(S, lane)] = ([hs], [he])
        return got

    def _new_slot(self, shape: tuple) -> dict:
        (F, K), n, dev, D = shape, self.n, self.device, self.emb.dimension
        return dict(seg=torch.empty((n, F, K), dtype=torch.float32, device=dev),
                    w=torch.empty((n, K, F), dtype=torch.float32, device=dev),
                    emb=torch.empty((n, K, D), dtype=torch.float32, device=dev),
                    seg_h=torch.empty((n, F, K), dtype=torch.float32).pin_memory(),
                    emb_h=torch.empty((n, K, D), dtype=torch.float32).pin_memory(),
                    ev_seg=torch.cuda.Event())

    def _launch_rows(self, base: int, stride: int, N: int, S: int, keep=None, ring: Optional[AudioRing] = None) -> dict:
        """The GPU half of a step for N <= num_streams rows of S samples at ``base + i * stride`` floats; nothing here
        waits for the GPU."""
        assert 1 <= N <= self.n
        F, K, D = self.seg.num_frames(S), self.seg.num_speakers, self.emb.dimension
        ln = self._prepare(S, (F, K))
        a, b = self.lanes[ln]["a"], self.lanes[ln]["b"]
        (hseg,), (hemb,) = self._handles(S, ln)
        slot = self._take_slot((F, K))
        lib = self._lib
        slot["ev_in"].record(torch.cuda.current_stream(self.device))      # inputs produced on the caller's stream
        a.wait_event(slot["ev_in"])
        b.wait_event(slot["ev_in"])
        stats = slot["stats"]
        _lib.check(lib.dz_wave_stats(self._ctx, base, stride, N, S, stats.data_ptr(), a.cuda_stream), "dz_wave_stats")
        _lib.check(lib.dz_seg_use_wave_stats(hseg, stats.data_ptr()), "dz_seg_use_wave_stats")
        _lib.check(lib.dz_seg_forward_osp(hseg, base, stride, N, slot["seg"].data_ptr(), self.gamma, self.beta,
                                          int(self.norm_w), slot["w"].data_ptr(), a.cuda_stream), "dz_seg_forward_osp")
        slot["ev_seg"].record(a)
        # the lane's handle carries one forward at a time: stream B orders this step's early half behind the late half
        # of the lane's previous step
        self.emb.early_launch(hemb, base, stride, N, b.cuda_stream)
        b.wait_event(slot["ev_seg"])
        self.emb.late_launch(hemb, base, stride, slot["w"].data_ptr(), N, K, F, slot["emb"].data_ptr(), b.cuda_stream)
        if self._gallery is not None:
            self._enqueue_match(slot, ln, N, b)
        _lib.check(lib.dz_results_to_host(self._ctx, slot["seg"].data_ptr(), slot["seg_h"].data_ptr(), N * F * K,
                                          slot["emb"].data_ptr(), slot["emb_h"].data_ptr(), N * K * D,
                                          b.cuda_stream), "dz_results_to_host")
        slot["done"].record(b)
        if ring is not None:                            # pushes `slack` steps from now wait for these forward passes
            ring._read_by([a, b])
        slot["rows"], slot["slots"], slot["keep"] = N, None, keep
        self._t += 1
        return slot


class WeSpeakerBatch(_TwoChainEngine):
    """``SpeakerDiarization`` of N concurrent streams with the WeSpeaker ResNet34 embedding
    (pyannote/wespeaker-voxceleb-resnet34-LM, the embedding of pyannote.audio 3.1's pipeline): the sibling of
    ``StreamBatch`` for the one model whose embedding trunk, not the segmentation, is the long chain of a step
    (about 10.7 ms of fbank + ResNet34 per 64 windows against a 0.7 ms segmentation).  Per stream it produces what
    that stream's own ``SpeakerDiarization`` produces; the public surface is ``StreamBatch``'s.

    The two-chain schedule with ``dz_wsp_trunk`` (reads the windows, in place from the ring) as the early launch and
    ``dz_wsp_pool(normalize=1)`` as the late one: the trunk does not depend on the segmentation, so the segmentation
    runs under it and only the pooling waits.  The embeddings are bit for bit those of
    ``HipWeSpeakerEmbedding.forward_multi`` on the same windows and weights (a row's result does not depend on the
    batch it is in).

    ``lanes`` defaults to 2 for every stream count: one ``dz_wsp`` handle of ``num_streams`` rows per lane holds about
    33 MB of activations per row at 5 s (four layer-1 sized buffers of 5.1 MB, the layer outputs, the fbank), i.e.
    about 2.1 GB per lane at 64 streams and 8.4 GB at 256 (``tools/wespeaker_streams.py`` reports the measured
    figure).  No sub-batches and no serial form; a latency outside [step, duration] is refused."""

    def __init__(self, segmentation: HipSegmentation, embedding: HipWeSpeakerEmbedding, num_streams: int,
                 tau_active: float = 0.6, rho_update: float = 0.3, delta_new: float = 1.0,
                 gamma: float = 3, beta: float = 10, max_speakers: int = 20,
                 normalize_embedding_weights: bool = False,
                 device: Optional[torch.device] = None, cluster_threads: int = 8,
                 tail: bool = False, duration: float = 5.0, step: float = 0.5,
                 latency: Optional[float] = None, *, lanes: Optional[int] = None,
                 recurrence: Optional[str] = None, inflight: Optional[int] = None, wait: Optional[str] = None,
                 warmup: Optional[int] = None):
        if not isinstance(embedding, HipWeSpeakerEmbedding):
            raise ValueError(f"WeSpeakerBatch runs the WeSpeaker ResNet34 embedding (HipWeSpeakerEmbedding), not "
                             f"{type(embedding).__name__}: use StreamBatch for HipEmbedding, HipEcapaEmbedding and "
                             "HipSbXvectorEmbedding")
        if not isinstance(segmentation, HipSegmentation):
            raise ValueError(f"WeSpeakerBatch: segmentation must be a HipSegmentation, got {type(segmentation).__name__}")
        if int(num_streams) < 1:
            raise ValueError(f"WeSpeakerBatch: num_streams={num_streams}")
        self._timing(duration, step, latency)
        super().__init__(segmentation, embedding, num_streams, tau_active, rho_update, delta_new, gamma, beta,
                         max_speakers, normalize_embedding_weights, device, cluster_threads, tail=tail,
                         duration=self.duration, step=self.step, latency=self.latency, lanes=lanes,
                         recurrence=recurrence, inflight=inflight, wait=wait, warmup=warmup)


class GroupsBatch(_TwoChainEngine):
    """``SpeakerDiarization`` of N concurrent streams with a groups-form embedding (``HipEcapaEmbedding``: config 3,
    powerset segmentation + ECAPA-TDNN; ``HipSbXvectorEmbedding``; ``HipTitaNetEmbedding``; ``HipSbResNetEmbedding``;
    ``HipEcapaMelEmbedding``): what ``StreamBatch(seg, emb,
    n, ...)`` constructs for them, with ``StreamBatch``'s arguments.  The two-chain schedule with no early launch and
    the model's ``groups_launch`` as the late one: each stream's K speaker rows are embedded with the batch geometry of
    those rows alone (``forward_groups``) and L2-normalised as the embedding block's ``EmbeddingNormalization(1)`` does.

    ``lanes`` (= ``depth``) defaults to 2: one ECAPA handle of 64 streams x 3 speakers = 192 rows x 501 frames (5 s)
    carves about 6.2 GB of device memory per lane, a speechbrain x-vector handle about 1.7 GB, a TitaNet-L handle about
    5.9 GB with "f16x3", a speechbrain ResNet handle about 2.1 GB, a mel-spectrogram ECAPA handle (192 rows x 313
    frames) about 4.3 GB with "f16x3" and 3.0 GB with "f32" (the handle computes its arena from the rows and the
    window).  ``seg_split`` and ``emb_split``
    must be None or 1; ``serial``: the measurement form, one lane (``lanes=1``) whose two chains share one HIP stream.
    The experiments build's ``DZ_PRIO_A``, ``DZ_PRIO_B``, ``DZ_SHARED_STATS``, ``DZ_SEG_SPLIT`` and ``DZ_EMB_SPLIT`` do
    not reach this engine."""


def _is_zero(value) -> bool:
    """Is ``value`` the number 0 (the default of an argument that a form does not take)?"""
    return isinstance(value, (int, float)) and not isinstance(value, bool) and value == 0


class FileBatch:
    """Several FILES of one rank through the hot path at once — the file-parallel evaluation
    (BASELINE.json configs 1 / 4) at the batcher's rate.

    The reference's ``Benchmark`` (``inference.py:392-432``) feeds one file at a time: batches of 32
    consecutive windows go through ``SpeakerDiarization.__call__``, whose per-chunk Python loop
    (``blocks/diarization.py:193-232``) then runs clustering, aggregation and binarisation.  Only
    that loop is sequential, and only within a file.  Here one GPU step carries ``rows`` windows:
    the next ``rows // k`` CONSECUTIVE windows of each of the ``k`` files that are open (file-major
    rows, gathered device to device from the file's resident audio); the host half hands every file
    to a thread that walks its windows in order through that file's own clustering / aggregation
    state (``dz_file_step_batch``; ``dz_file_vad_step_batch`` for the VAD form), ``depth`` GPU steps in
    flight.  A file that ends frees its slot for the next one.  Per file the speech turns — hence the
    RTTM — are those of the one-file-at-a-time path (``tests/test_gpu_der.py``,
    ``tests/test_gpu_file_batch_models.py``).

    The engine under the files follows the models, as ``StreamServer``'s does (``self.kind``):

        HipEmbedding (pyannote/embedding)            "xvector"    StreamBatch
        HipWeSpeakerEmbedding                        "wespeaker"  WeSpeakerBatch
        a groups-form embedding (ECAPA, speechbrain  "groups"     what StreamBatch(seg, emb, ...) constructs: GroupsBatch
          x-vector, TitaNet-L, speechbrain ResNet,                (each chunk's K rows embedded alone: the blocks path at
          mel-spectrogram ECAPA)                                  batch_size = 1, see Benchmark.file_batch)
        None with pipeline="vad"                     "vad"        VadBatch; every turn is labelled "speech"
        None with pipeline="osd"                     "osd"        OverlapBatch; every turn is labelled "overlap"

    Everything ``run`` does with its engine goes through ``_launch_rows`` and the ticket's pinned results
    (``seg_h`` / ``emb_h``, or ``vad_h``).

    ``run(files)``: ``files`` = iterable of ``(uri, padded waveform float32 (samples,), shift)``;
    the waveform already carries ``config.get_padding`` and a zero-filled last block (what
    ``file_blocks`` emits), ``shift`` is the pipeline's ``timestamp_shift``.  Returns
    ``{uri: Annotation}`` (``PredictionAccumulator`` semantics: every chunk's turns, then
    ``support(patch_collar)``)."""

    # Is a step's stage filled by ONE dz_gather_windows launch (True) or by one torch copy per open file?  The kernel takes
    # 6.7 us where the 16 copies take 112 us of GPU time, but the pyannote/embedding form, measured against the parent
    # commit, showed no gain from it (profiles/r24a_file_batch_models.json; README "File batches for every model"): the
    # form that existed keeps the copies it had, the new forms start with the kernel.
    GATHER_DEFAULT = {"xvector": False, "wespeaker": True, "groups": True, "vad": True, "osd": True}

    def __init__(self, segmentation: HipSegmentation, embedding=None, *, rows: int = 64,
                 max_files: int = 16, tau_active: float = 0.6, rho_update: float = 0.3, delta_new: float = 1.0,
                 gamma: float = 3, beta: float = 10, max_speakers: int = 20,
                 normalize_embedding_weights: bool = False, duration: float = 5.0, step: float = 0.5,
                 latency: Optional[float] = None, sample_rate: int = 16000,
                 device: Optional[torch.device] = None, threads: int = 8, patch_collar: float = 0.05,
                 recurrence: Optional[str] = "valu", lanes: Optional[int] = 2, pipeline: str = "diarization",
                 gather: Optional[bool] = None, tau_offset: Optional[float] = None, min_duration_on: float = 0.0,
                 min_duration_off: float = 0.0):
        """``recurrence`` / ``lanes``: the engine under the files.  A file job is short and its files end at different
        times: the latency-form recurrence on two lanes finishes 16 ten-minute files 13 - 40 % sooner than the
        throughput engine a 64-row ``StreamBatch`` would pick for itself (profiles/r06q_file_batch_engine.json:
        25 800 - 26 700 vs 17 900 - 23 600 chunks/s); None = let the engine choose.  The other forms keep the same
        pair for another reason too: the blocks path always runs the "valu" recurrence, a matrix-core recurrence rounds
        the segmentation scores differently, and the RTTM files have to be those of the one-file-at-a-time loop byte for
        byte; two lanes are what the two-chain engines run anyway (gigabytes of arena per lane).

        ``pipeline``: "diarization" | "vad" | "osd" (``embedding`` must be None for the last two).  ``gather``: fill a step's stage with one
        ``dz_gather_windows`` launch instead of one torch copy per open file (None = the form's default).
        ``tau_offset``: the hysteresis of the "vad" and "osd" forms (every file's tail starts with the state off);
        ``pipeline="diarization"`` refuses it.  ``min_duration_on`` / ``min_duration_off`` (seconds): the minimum
        durations of the "vad" and "osd" forms, ``functional.min_duration`` on a file's turns at its end, where
        ``support(patch_collar)`` stitches them — the engine under the files is a live engine, has no look-ahead and never
        sees them; ``pipeline="diarization"`` refuses them by name."""
        self.rows, self.max_files = int(rows), max(1, min(int(max_files), int(rows)))
        if pipeline not in ("diarization", "vad", "osd"):
            raise ValueError(f"FileBatch: pipeline={pipeline!r} (expected diarization | vad | osd)")
        if tau_offset is not None and pipeline == "diarization":
            from .blocks.diarization import refuse_tau_offset
            refuse_tau_offset({"tau_offset": tau_offset}, "FileBatch(pipeline='diarization')")
        from .blocks.base import check_tau_offset
        self.tau_offset = check_tau_offset(tau_offset, "FileBatch")
        if pipeline == "diarization":
            from .blocks.base import refuse_min_duration
            refuse_min_duration({k: v for k, v in (("min_duration_on", min_duration_on),
                                                   ("min_duration_off", min_duration_off)) if not _is_zero(v)},
                                "FileBatch(pipeline='diarization')")
        from .blocks.base import check_min_duration
        self.min_duration_on = check_min_duration(min_duration_on, "min_duration_on", "FileBatch")
        self.min_duration_off = check_min_duration(min_duration_off, "min_duration_off", "FileBatch")
        if pipeline in ("vad", "osd"):
            if embedding is not None:
                raise ValueError(f"FileBatch(pipeline={pipeline!r}) takes no embedding")
            self.kind = pipeline
            engine = VadBatch if pipeline == "vad" else OverlapBatch
            self.engine = engine(segmentation, self.rows, tau_active, duration, step, latency, device, lanes=lanes,
                                 recurrence=recurrence, host_threads=threads)
        else:
            if isinstance(embedding, HipWeSpeakerEmbedding):
                self.kind, engine = "wespeaker", WeSpeakerBatch
            elif isinstance(embedding, _HipGroupsEmbedding):
                self.kind, engine = "groups", StreamBatch          # -> GroupsBatch
            elif isinstance(embedding, HipEmbedding):
                self.kind, engine = "xvector", StreamBatch
            else:
                raise ValueError(f"FileBatch: no engine runs the embedding {type(embedding).__name__}")
            self.engine = engine(segmentation, embedding, self.rows, tau_active, rho_update, delta_new, gamma,
                                 beta, max_speakers, normalize_embedding_weights, device=device,
                                 cluster_threads=threads, tail=False, duration=duration, step=step,
                                 latency=latency, recurrence=recurrence, lanes=lanes)
        self.gather = FileBatch.GATHER_DEFAULT[self.kind] if gather is None else bool(gather)
        self.device = self.engine.device
        self.duration, self.step, self.sr = float(duration), float(step), int(sample_rate)
        self.latency = self.step if latency is None else float(latency)
        self.S, self.hop = int(round(sample_rate * duration)), int(round(sample_rate * step))
        assert self.hop % 4 == 0, "the step must be a multiple of 4 samples (16-byte aligned windows)"
        self.tau, self.rho, self.delta = tau_active, rho_update, delta_new
        self.G = 1 if self.kind in ("vad", "osd") else int(max_speakers)
        self.threads, self.patch_collar = int(threads), patch_collar
        self._lib = _lib.load()
        self._ctx = _lib.context(self.device.index)
        self._runs = (_lib.WindowRun * self.max_files)()
        self._clu: List = []          # per file slot: dz_clu handle (none for the VAD form)
        self._tails: Optional[BatchedOutputTail] = None
        self._stage: List[torch.Tensor] = []
        self._pool, self._lent = FileBatch._PinnedPool(), {}
        self.chunks_done = 0

    # ------------------------------------------------------------------ per-slot state
    def _ensure_state(self, F: int) -> None:
        if self._tails is not None:
            return
        for _ in range(0 if self.kind in ("vad", "osd") else self.max_files):
            h = _lib.vp()
            _lib.check(self._lib.dz_clu_create(self.tau, self.rho, self.delta, self.G, C.byref(h)), "dz_clu_create")
            self._clu.append(h)
        # DelayedAggregation(hamming, loose) + Binarize: what both pipelines build (the VAD form: one "speaker")
        self._tails = BatchedOutputTail(self.max_files, F, self.G, self.step, self.latency, self.tau,
                                        num_threads=self.threads, offset=self.tau_offset)
        self._F = F
        self._max_turns = self._tails.max_turns
        n = self.engine.max_inflight + 1
        self._stage = [torch.empty((self.rows, self.S), dtype=torch.float32, device=self.device) for _ in range(n)]
        self._turns = [np.empty((self.rows, self._max_turns, 3), dtype=np.float64) for _ in range(2)]
        self._nturns = [np.empty(self.rows, dtype=np.int32) for _ in range(2)]

    def __del__(self):
        try:
            for h in self._clu:
                self._lib.dz_clu_destroy(h)
        except Exception:
            pass

    # ------------------------------------------------------------------ the run
    class _PinnedPool:
        """Pinned host buffers for the files in flight, reused (allocating pinned memory costs
        milliseconds per file; the loader thread acquires, the run loop releases)."""

        def __init__(self):
            import threading
            self._free: List[torch.Tensor] = []
            self._lock = threading.Lock()

        def acquire(self, n: int) -> torch.Tensor:
            with self._lock:
                for i, t in enumerate(self._free):
                    if t.numel() >= n:
                        return self._free.pop(i)
            return torch.empty(max(1, int(n * 1.1)), dtype=torch.float32).pin_memory()

        def release(self, t: torch.Tensor) -> None:
            with self._lock:
                self._free.append(t)

    def host_buffer(self, n: int) -> np.ndarray:
        """A pinned float32 array of n samples from the pool, for a feeder that wants to decode a file
        straight into upload-ready memory (``Benchmark.run_batched``); hand it to ``run`` as the
        waveform and the loader skips its own copy."""
        t = self._pool.acquire(n)
        a = t.numpy()[:n]
        self._lent[a.__array_interface__["data"][0]] = t
        return a

    class _Loader:
        """Reads / pads the next files on a background thread while the GPU works (reading a WAV and
        converting it to float32 takes ~10 ms per 5 minutes of audio: done serially in front of the
        first launch it cost more than the GPU time of the whole file).  ``get(block)`` ->
        (uri, pinned float32 tensor, samples, shift) in the order of ``files``, None when nothing is
        ready yet (``block=False``), ``StopIteration`` at the end."""

        def __init__(self, files, owner: "FileBatch", depth: int = 4):
            import queue
            import threading
            self.q: "queue.Queue" = queue.Queue(maxsize=depth)
            self.done = False
            self.stop = False               # set by close(): the thread stops producing and hands its buffer back
            self._END = object()
            self._owner = owner

            def put(item) -> bool:          # q.put that gives up when the consumer has gone away
                while not self.stop:
                    try:
                        self.q.put(item, timeout=0.05)
                        return True
                    except queue.Full:
                        continue
                return False

            def work():
                try:
                    for uri, wav, shift in files:
                        lent = None
                        if isinstance(wav, np.ndarray) and wav.dtype == np.float32 and wav.ndim == 1:
                            lent = owner._lent.pop(wav.__array_interface__["data"][0], None)
                        if lent is not None:            # decoded straight into a pool buffer
                            t = lent
                        else:
                            wav = np.ascontiguousarray(wav, dtype=np.float32).reshape(-1)
                            t = owner._pool.acquire(len(wav))
                            t[:len(wav)].copy_(torch.from_numpy(wav))
                        if not put((uri, t, len(wav), shift)):
                            owner._pool.release(t)
                            return
                    put(self._END)
                except BaseException as exc:       # surfaces in the consumer
                    put(exc)

            threading.Thread(target=work, name="dz-file-loader", daemon=True).start()

        def close(self) -> None:
            """Stop the loader thread and give the pinned buffers of files that were read but never admitted
            back to the pool (the consumer is leaving early: an exception in a step)."""
            import queue
            self.stop = True
            while True:
                try:
                    item = self.q.get(timeout=0.1)
                except queue.Empty:
                    break
                if isinstance(item, tuple):
                    self._owner._pool.release(item[1])
            self.done = True

        def get(self, block: bool):
            import queue
            if self.done:
                raise StopIteration
            try:
                item = self.q.get(block=block)
            except queue.Empty:
                return None
            if item is self._END:
                self.done = True
                raise StopIteration
            if isinstance(item, BaseException):
                self.done = True
                raise item
            return item

    def run(self, files) -> dict:
        files = FileBatch._Loader(files, self)
        F = self.engine.seg.to(self.device).num_frames(self.S)
        self._ensure_state(F)
        vad = self.kind in ("vad", "osd")         # the one-track forms: no clustering, one label for every turn
        res = self.duration / F
        open_files: List[Optional[dict]] = [None] * self.max_files
        done: dict = {}
        exhausted = False
        inflight: List[tuple] = []
        step_no = 0

        def admit():
            """Fill free slots with files that are READY; wait for one only when nothing is open."""
            nonlocal exhausted
            for slot in range(self.max_files):
                if exhausted:
                    return
                if open_files[slot] is None:
                    try:
                        item = files.get(block=not any(f is not None for f in open_files))
                    except StopIteration:
                        exhausted = True
                        return
                    if item is None:
                        return
                    uri, pinned, nsamp, shift = item
                    if uri in done or any(f is not None and f["uri"] == uri for f in open_files):
                        self._pool.release(pinned)
                        raise ValueError(f"FileBatch.run: two files share the uri {uri!r}; the results are keyed by it")
                    nwin = (nsamp - self.S) // self.hop + 1 if nsamp >= self.S else 0
                    if not vad:
                        _lib.check(self._lib.dz_clu_reset(self._clu[slot]), "dz_clu_reset")
                    self._tails.reset(slot)
                    if nwin <= 0:
                        done[uri] = []
                        self._pool.release(pinned)      # shorter than one window: nothing to upload
                        return admit()
                    open_files[slot] = dict(uri=uri, shift=float(shift), nwin=nwin, sent=0, got=0, turns=[], start=0,
                                            audio=pinned[:nsamp].to(self.device, non_blocking=True), host=pinned)

        def launch_step():
            nonlocal step_no
            active = [(slot, f) for slot, f in enumerate(open_files) if f is not None and f["sent"] < f["nwin"]]
            if not active:
                return False
            per = max(1, self.rows // len(active))
            stage = self._stage[step_no % len(self._stage)]
            plan, r = [], 0
            for slot, f in active:
                c = min(per, f["nwin"] - f["sent"], self.rows - r)
                if c <= 0:
                    break
                w0 = f["sent"]
                # c consecutive windows of this file, `hop` apart in its resident audio -> dense rows
                if self.gather:
                    run = self._runs[len(plan)]
                    run.src, run.row0, run.count = f["audio"].data_ptr() + 4 * w0 * self.hop, r, c
                else:
                    view = f["audio"][w0 * self.hop: w0 * self.hop + (c - 1) * self.hop + self.S].unfold(0, self.S, self.hop)
                    stage[r:r + c].copy_(view, non_blocking=True)
                # window start times by repeated addition, exactly as rearrange_audio_stream counts them
                # (`start += step`, operators.py:82-84): bit-identical for steps that are not dyadic
                starts = np.empty(c, dtype=np.float64)
                for j in range(c):
                    starts[j] = f["start"]
                    f["start"] += self.step
                plan.append((slot, f, r, c, starts))
                f["sent"] += c
                r += c
            if self.gather:
                # one launch for every open file, on the stream the files' uploads were queued on
                _lib.check(self._lib.dz_gather_windows(
                    self._ctx, self._runs, len(plan), self.S, self.hop, stage.data_ptr(), stage.stride(0), self.rows,
                    torch.cuda.current_stream(self.device).cuda_stream), "dz_gather_windows")
            ticket = self.engine._launch_rows(stage.data_ptr(), stage.stride(0), r, self.S, keep=stage)
            inflight.append((ticket, plan, r))
            step_no += 1
            return True

        def finish_step():
            ticket, plan, r = inflight.pop(0)
            with self.engine._host_half(ticket):
                k = len(plan)
                tails = (_lib.vp * k)(*[self._tails._hs[slot] for slot, *_ in plan])
                row0 = np.array([p[2] for p in plan], dtype=np.int32)
                count = np.array([p[3] for p in plan], dtype=np.int32)
                starts = np.concatenate([p[4] for p in plan]).astype(np.float64)
                turns, nturns = self._turns[0], self._nturns[0]
                if vad:
                    track = ticket["vad_h"].numpy()[:r]
                    _lib.check(self._lib.dz_file_vad_step_batch(
                        tails, k, row0.ctypes.data, count.ctypes.data, track.ctypes.data, track.shape[1],
                        starts.ctypes.data, float(res), turns.ctypes.data, self._max_turns, nturns.ctypes.data,
                        self.threads), "dz_file_vad_step_batch")
                else:
                    seg = ticket["seg_h"].numpy()[:r]
                    emb = ticket["emb_h"].numpy()[:r]
                    clus = (_lib.vp * k)(*[self._clu[slot] for slot, *_ in plan])
                    _lib.check(self._lib.dz_file_step_batch(
                        clus, tails, k, row0.ctypes.data, count.ctypes.data, seg.ctypes.data, seg.shape[1], seg.shape[2],
                        emb.ctypes.data, emb.shape[2], self.G, starts.ctypes.data, float(res), turns.ctypes.data,
                        self._max_turns, nturns.ctypes.data, None, self.threads), "dz_file_step_batch")
            for slot, f, r0, c, _ in plan:
                for j in range(r0, r0 + c):
                    if nturns[j]:
                        f["turns"].append(turns[j, :nturns[j]].copy())
                f["got"] += c
                self.chunks_done += c
                if f["got"] == f["nwin"]:
                    done[f["uri"]] = (f["turns"], f["shift"])
                    open_files[slot] = None
                    self._pool.release(f["host"])     # its upload finished long ago (results depend on it)

        try:
            admit()
            while True:
                while len(inflight) < self.engine.max_inflight and launch_step():
                    pass
                if not inflight:
                    admit()
                    if not any(f is not None for f in open_files):
                        break
                    continue
                finish_step()
                admit()
        except BaseException:
            # leave nothing behind: tickets still on the GPU are waited for and handed back (a busy
            # ticket makes every later launch allocate pinned memory under running kernels), the open files'
            # and the loader's pinned buffers return to the pool, the loader thread stops
            for ticket, _, _ in inflight:
                try:
                    self.engine._wait(ticket)
                finally:
                    self.engine._release(ticket)
            # the open files' pinned buffers may still be the source of a non_blocking upload: only a finished
            # copy makes them safe to hand to the next run's loader thread
            try:
                torch.cuda.synchronize(self.engine.device)
            except Exception:      # noqa: BLE001 — the original exception is the one to report
                pass
            for f in open_files:
                if f is not None:
                    self._pool.release(f["host"])
            files.close()
            raise
        out = {}
        for uri, rec in done.items():
            ann = Annotation(uri=uri, modality="speech")
            if rec:
                chunks, shift = rec
                for arr in chunks:
                    for n, (s, e, g) in enumerate(arr):
                        if vad:                 # one track per turn of a chunk, like Timeline.to_annotation
                            ann[Segment(s + shift, e + shift), n] = self.engine.LABEL
                        else:
                            ann[Segment(s + shift, e + shift), int(g)] = f"speaker{int(g)}"
            if self.min_duration_on == 0.0 and self.min_duration_off == 0.0:
                out[uri] = ann.support(self.patch_collar)
            else:
                from .functional import min_duration
                out[uri] = min_duration(ann, self.min_duration_on, self.min_duration_off, self.patch_collar)
        return out
