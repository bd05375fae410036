"""Many live streams on one GPU: a cross-stream batcher on top of ``StreamBatch``
(SURVEY.md §8f rank 4).

The reference serves ONE stream per process (``diart.serve`` / ``diart.stream``:
``console/serve.py:105-127``, ``sources.py:204-271`` feed a single ``StreamingInference``); its
per-stream chain is ``source blocks -> rearrange_audio_stream -> pipeline([chunk])``
(``inference.py:101-147``).  ``StreamServer`` keeps that chain per stream — arbitrary-length audio
blocks in, a new 5 s window every 500 ms of audio (``operators.py:44-100``) — but runs the windows
that are ready *across streams* as one GPU batch: every ``step()`` takes at most one pending
window from each open stream, stacks them, runs segmentation / embedding once and steps each
stream's own clustering and aggregation state.  Streams join and leave at any time and advance at
their own pace; per stream the output is what a dedicated ``SpeakerDiarization`` pipeline with the
same configuration produces.  The model pair may be config 2's (x-vector) or config 3's (powerset segmentation +
``HipEcapaEmbedding``, with ``normalize_embedding_weights=True``), or the same with the speechbrain x-vector
(``HipSbXvectorEmbedding``), the speechbrain ResNet (``HipSbResNetEmbedding``) or the mel-spectrogram ECAPA
(``HipEcapaMelEmbedding``) on a ``GroupsBatch``; with a ``HipWeSpeakerEmbedding`` (pyannote.audio 3.1's embedding)
the engine is a ``WeSpeakerBatch``.  ``pipeline="vad"`` (no embedding) serves
``VoiceActivityDetection`` instead (``diart.serve --pipeline VoiceActivityDetection``, reference
``console/serve.py:19-22,99-102``) on a ``VadBatch``: every stream's turns are labelled ``"speech"``, and
only the prediction is served, not the aggregated audio.  ``pipeline="osd"`` (no embedding either) serves
``OverlappedSpeechDetection`` the same way on an ``OverlapBatch``: the turns are the regions where two or more people
talk at once, labelled ``"overlap"``.

Audio reaches the GPU through per-stream device rings (``AudioRing.push_rows`` / ``gather``): a step
uploads only the NEW 500 ms block of each stream that has one (32 KB instead of the 320 KB window the
reference moves per chunk, ``blocks/segmentation.py:47``) and assembles the batch of windows on the
device.  ``device_rings=False`` (and any custom ``engine``) keeps the windows on the host instead.

Clients may send what they have: ``input_format`` ``"s16"`` (16-bit PCM), ``"u8"``, ``"s32"``, ``"ulaw"`` or ``"alaw"``
(G.711, one byte per sample: telephone audio, usually with ``input_sample_rate=8000``; the definitions are in
``diart_amd.pcm``) and ``input_channels`` (interleaved frames, averaged like the reference's loader,
``audio.py:32-34``).  In ring mode the raw blocks are uploaded as they came
and the push kernel converts and averages them (``dz_ring_push_rows_pcm``); the host modes do the same arithmetic
in numpy (``pcm_to_mono``), so every mode hands the models identical float32 windows.  ``device_rings="all"``
also uses rings where a block is not a multiple of 4 samples (44.1 kHz, 22.05 kHz).

Clients differ in level by tens of dB.  ``volume_in_db`` (default ``None``: off, no kernel, today's windows) brings
every window of every stream to that volume on its own before the models see it — the reference's per-window
``blocks.AdjustVolume``: gain to the target, then division by the scaled peak where it exceeds 1.  With the default
engines it runs in place on the staged device rows, behind the resampler and on its stream; a custom ``engine`` gets
windows adjusted by the same kernel, so every mode sees identical bits.  As in the reference a digitally silent
window (all zeros) becomes a NaN window, and its scores are NaN rows.

Transport (websocket, microphone) is out of scope: ``push`` is the seam a network front-end calls
(thread-safe), ``step`` / ``serve_forever`` is the worker loop."""
from __future__ import annotations

import threading
import time
from typing import Callable, Dict, Hashable, List, Optional

import numpy as np
import torch

from .blocks.aggregation import BatchedOutputTail
from .features import Annotation
from .functional import _target_db, adjust_volume, adjust_volume_rows, resampler
from .models import HipWeSpeakerEmbedding
from .pcm import INPUT_FORMATS, pcm_to_mono  # noqa: F401  (INPUT_FORMATS: name -> dtype of the values clients push)
from .pipeline import AudioRing, OverlapBatch, StreamBatch, VadBatch, WeSpeakerBatch

PIPELINES = ("diarization", "vad", "osd")
# the segmentation-only pipelines: (what it is, its engine, the label of every turn)
_ONE_TRACK = {"vad": ("VoiceActivityDetection", VadBatch, "speech"),
              "osd": ("OverlappedSpeechDetection", OverlapBatch, "overlap")}
MAX_INPUT_CHANNELS = 8


class _Stream:
    __slots__ = ("slot", "buffer", "blocks", "consumed", "chunk", "start", "emitted", "prediction")

    def __init__(self, slot: int, dtype=np.float32):
        self.slot = slot
        self.buffer = np.zeros(0, dtype=dtype)        # values (input format, interleaved) not yet a whole step block
        self.blocks: List[np.ndarray] = []            # whole step blocks the worker has not taken yet
        self.consumed = 0                             # step blocks taken by the worker so far
        self.chunk: Optional[np.ndarray] = None       # host-window mode: the current (<= duration) window
        self.start = 0.0                              # host-window mode: start time of `chunk`
        self.emitted = 0
        self.prediction: Optional[Annotation] = None


class StreamServer:
    def __init__(self, segmentation, embedding, max_streams: int = 64, *, duration: float = 5.0,
                 step: float = 0.5, latency: Optional[float] = None, sample_rate: int = 16000,
                 tau_active: float = 0.6, rho_update: float = 0.3, delta_new: float = 1.0,
                 gamma: float = 3, beta: float = 10, max_speakers: int = 20,
                 device: Optional[torch.device] = None, patch_collar: float = 0.05,
                 engine: Optional[Callable] = None, device_rings=True,
                 normalize_embedding_weights: bool = False, input_sample_rate: Optional[int] = None,
                 pipeline: str = "diarization", input_format: str = "f32", input_channels: int = 1,
                 volume_in_db: Optional[float] = None, tau_offset: Optional[float] = None):
        if pipeline not in PIPELINES:
            raise ValueError(f"StreamServer: pipeline={pipeline!r} (expected one of {PIPELINES})")
        # hysteresis of the one-track pipelines (VadBatch / OverlapBatch keep the state per slot; a stream that joins
        # gets a reset slot, so it starts with the state off); refused before anything touches the GPU
        if tau_offset is not None and pipeline not in _ONE_TRACK:
            from .blocks.diarization import refuse_tau_offset
            refuse_tau_offset({"tau_offset": tau_offset}, "StreamServer(pipeline='diarization')")
        from .blocks.base import check_tau_offset
        self.tau_offset = check_tau_offset(tau_offset, "StreamServer")
        if self.tau_offset is not None and engine is not None:
            raise ValueError("StreamServer: tau_offset is the default engine's (VadBatch / OverlapBatch); a custom "
                             "engine= binarises on its own")
        if pipeline in _ONE_TRACK and embedding is not None:
            raise ValueError(f"StreamServer: pipeline={pipeline!r} ({_ONE_TRACK[pipeline][0]}) runs the segmentation "
                             "only; pass embedding=None")
        if input_format not in INPUT_FORMATS:
            raise ValueError(f"StreamServer: input_format={input_format!r} (expected one of {tuple(INPUT_FORMATS)})")
        if not (isinstance(input_channels, (int, np.integer)) and 1 <= input_channels <= MAX_INPUT_CHANNELS):
            raise ValueError(f"StreamServer: input_channels={input_channels!r} (expected 1 .. {MAX_INPUT_CHANNELS})")
        if device_rings not in (True, False, "all"):
            raise ValueError(f"StreamServer: device_rings={device_rings!r} (expected True, False or 'all')")
        # per-window volume adjustment (None: off); a non-finite or non-numeric target is refused here
        self.volume_in_db = None if volume_in_db is None else _target_db(volume_in_db)
        # what clients push: interleaved frames of `input_channels` values of `input_format`
        self.input_format, self.input_channels = input_format, int(input_channels)
        self._in_dtype = INPUT_FORMATS[input_format]
        self.pipeline = pipeline
        self._label = _ONE_TRACK[pipeline][2] if pipeline in _ONE_TRACK else None   # turn labels: speaker{g} | speech | overlap
        self.duration, self.step_seconds, self.sample_rate = float(duration), float(step), int(sample_rate)
        self.latency = self.step_seconds if latency is None else float(latency)
        # the rate clients push at.  Blocks and windows are cut at this rate; a window at another rate than the
        # pipeline's is resampled on its own on the device before the models see it (the reference's per-window
        # blocks.Resample, inference.py:101-122)
        self.input_sample_rate = self.sample_rate if input_sample_rate is None else int(input_sample_rate)
        self.model_chunk_samples = int(round(sample_rate * duration))
        self.chunk_samples = int(round(self.input_sample_rate * duration))
        self.step_samples = int(round(self.input_sample_rate * step))
        self._block_values = self.step_samples * self.input_channels      # values of one step block as pushed
        self.resampler = None
        self.max_streams, self.patch_collar = int(max_streams), patch_collar
        self.blocks_per_window = -(-self.chunk_samples // self.step_samples)
        self._lock = threading.Lock()          # stream table, buffers, slot lists
        self._step_lock = threading.Lock()     # serialises step(): one engine
        self._streams: Dict[Hashable, _Stream] = {}
        self._free = list(range(self.max_streams - 1, -1, -1))
        self._inflight: set = set()            # slots whose window the worker is processing now
        self._deferred: List[int] = []         # slots closed while in flight: freed after the step
        self._stop = False
        self._step_names = None                # per row of the step's batch: {g: name} (a gallery is attached), else None
        import collections
        self.step_errors = collections.deque(maxlen=64)   # (time, repr) of failed steps, newest last
        # `engine(windows (k, S) float32, starts (k,), slots [k]) -> list of k (turns (m, 3) array)`;
        # the default engine is a StreamBatch with the C++ output tail (a VadBatch for pipeline="vad", an OverlapBatch
        # for pipeline="osd")
        if engine is None and pipeline in _ONE_TRACK:
            batch_cls = _ONE_TRACK[pipeline][1]
            self.batch = batch_cls(segmentation, self.max_streams, tau_active, duration=duration, step=step,
                                   latency=self.latency, device=device, tau_offset=self.tau_offset)
        elif engine is None:
            # the WeSpeaker ResNet34 embedding has an engine of its own (its trunk is the long chain of a step)
            batch_cls = WeSpeakerBatch if isinstance(embedding, HipWeSpeakerEmbedding) else StreamBatch
            self.batch = batch_cls(segmentation, embedding, self.max_streams, tau_active, rho_update,
                                   delta_new, gamma, beta, max_speakers,
                                   normalize_embedding_weights=normalize_embedding_weights, device=device, tail=True,
                                   duration=duration, step=step, latency=self.latency)
        if engine is None:
            self._dev = torch.empty((self.max_streams, self.model_chunk_samples), dtype=torch.float32,
                                    device=self.batch.device)
            # resampling: windows at the input rate land in _raw, their resampled rows in _dev
            if self.input_sample_rate != self.sample_rate:
                self.resampler = resampler(self.input_sample_rate, self.sample_rate, self.batch.device)
                if self.resampler.out_len(self.chunk_samples) != self.model_chunk_samples:
                    raise ValueError(f"a {duration} s window at {self.input_sample_rate} Hz resamples to "
                                     f"{self.resampler.out_len(self.chunk_samples)} samples, not {self.model_chunk_samples}")
                self._raw = torch.empty((self.max_streams, self.chunk_samples), dtype=torch.float32,
                                        device=self.batch.device)
            self._engine, self._reset_slot = self._gpu_engine, self.batch.reset
            # per-stream device rings need whole blocks per window, and 16-byte aligned rows unless
            # device_rings="all" (44.1 kHz: 22 050 samples per block; the ring then moves 4-byte pieces where it must)
            self.rings: Optional[AudioRing] = None
            if device_rings and self.chunk_samples % self.step_samples == 0 and \
                    (self.step_samples % 4 == 0 or device_rings == "all"):
                self.rings = AudioRing(self.max_streams, self.chunk_samples, self.step_samples, slack_blocks=0,
                                       device=self.batch.device)
                # a stream takes at most blocks_per_window blocks in one step (its warm-up); round r of
                # a step stages its blocks in plane r, so no plane is rewritten while the GPU reads it.  The planes
                # hold the blocks as the clients sent them (the push kernel converts), rows 16 bytes apart or a
                # multiple: the kernel then loads 16 bytes per lane
                per16 = 16 // self._in_dtype.itemsize
                self._stage = torch.empty((self.blocks_per_window, self.max_streams, -(-self._block_values // per16) * per16),
                                          dtype=torch.from_numpy(np.zeros(0, self._in_dtype)).dtype).pin_memory()
            else:
                self._pinned = torch.empty((self.max_streams, self.chunk_samples), dtype=torch.float32).pin_memory()
        else:
            self.batch, self.rings = None, None
            self._engine, self._reset_slot = engine, getattr(engine, "reset", lambda slot: None)
            if self.volume_in_db is not None:
                # a custom engine gets its windows adjusted, each on its own (GPU), behind the resampler
                self._engine = self._adjusting_engine(engine, device)
            if self.input_sample_rate != self.sample_rate:
                # a custom engine gets its windows at the pipeline's rate, each resampled on its own (GPU)
                self.resampler = resampler(self.input_sample_rate, self.sample_rate, device)
                self._engine = self._resampling_engine(self._engine)

    # ------------------------------------------------------------------ speaker gallery
    def set_gallery(self, gallery, delta_id=None) -> None:
        """Name the speakers of every stream against ``gallery`` (``gallery.SpeakerGallery``; ``None`` removes it):
        the engine's ``set_gallery``, between two steps.  From the next ``step()`` on the Annotations carry the names
        where a voiceprint is within ``delta_id`` (no default; a gallery with a cohort is matched by the normalised
        distance and takes a signed threshold), and so does everything derived from them: ``close()``
        and the websocket messages.  A stream that joins later starts with no names (``open`` resets its slot).  The
        diarization pipeline only: ``"vad"`` and ``"osd"`` have no speakers to name."""
        if self.pipeline in _ONE_TRACK:
            raise ValueError(f"StreamServer.set_gallery: pipeline={self.pipeline!r} ({_ONE_TRACK[self.pipeline][0]}) has "
                             "no speakers to name; a gallery needs pipeline='diarization'")
        if self.batch is None:
            raise ValueError("StreamServer.set_gallery: a custom engine runs its own embedding; the gallery needs the "
                             "default engine")
        with self._step_lock:
            self.batch.set_gallery(gallery, delta_id)

    # ------------------------------------------------------------------ stream life cycle
    def open(self, stream_id: Hashable) -> None:
        with self._lock:
            if stream_id in self._streams:
                raise ValueError(f"stream {stream_id!r} is already open")
            if not self._free:
                raise RuntimeError(f"all {self.max_streams} stream slots are in use")
            # a free slot is never in flight (close() defers the release of a slot the worker is
            # still stepping), so resetting its clustering / aggregation state here is safe
            slot = self._free.pop()
            self._reset_slot(slot)
            if self.rings is not None:
                self.rings.reset_row(slot)
            self._streams[stream_id] = _Stream(slot, self._in_dtype)

    def close(self, stream_id: Hashable) -> Annotation:
        """Drop the stream (windows still pending are discarded: call ``drain`` first to flush them)
        and return everything it said so far, stitched like ``PredictionAccumulator``
        (``sinks.py:59-88``)."""
        with self._lock:
            st = self._streams.pop(stream_id)
            if st.slot in self._inflight:
                # the worker is inside step() with a window of this stream: its clustering / tail
                # state is being read on host threads right now.  The slot is handed back (and may
                # then be reset by the next open()) only when that step has finished; the step's
                # result for this stream is discarded.
                self._deferred.append(st.slot)
            else:
                self._free.append(st.slot)
        pred = st.prediction if st.prediction is not None else Annotation(str(stream_id), "speech")
        pred.uri = str(stream_id)
        return pred.support(self.patch_collar)

    @property
    def open_streams(self) -> List[Hashable]:
        with self._lock:
            return list(self._streams)

    # ------------------------------------------------------------------ audio in
    def push(self, stream_id: Hashable, samples) -> int:
        """Append audio (any length) to a stream; returns the number of windows now pending for it.  ``samples``:
        values of the server's ``input_format`` — mono, or for ``input_channels > 1`` interleaved frames as a 1-D
        array (a call may end in the middle of a frame) or an ``(n, channels)`` array.  The windowing is
        ``rearrange_audio_stream`` (``operators.py:44-100``): whole ``step`` blocks, a window once ``duration``
        seconds have arrived, then one per block."""
        x = self._as_values(samples)
        with self._lock:
            st = self._streams[stream_id]
            st.buffer = np.concatenate([st.buffer, x]) if st.buffer.size else x.copy()
            while st.buffer.size >= self._block_values:
                st.blocks.append(st.buffer[:self._block_values].copy())
                st.buffer = st.buffer[self._block_values:]
            return self._pending(st)

    def _as_values(self, samples) -> np.ndarray:
        """``samples`` as a 1-D array of the input dtype; another kind of number is refused, not cast."""
        x = np.asarray(samples)
        if self.input_format == "f32":
            if x.dtype.kind != "f":
                raise ValueError(f"push: {x.dtype} samples to a server with input_format='f32' (expected float32)")
        elif x.dtype != self._in_dtype:
            raise ValueError(f"push: {x.dtype} samples to a server with input_format={self.input_format!r} "
                             f"(expected {self._in_dtype.name})")
        if self.input_channels > 1 and not (x.ndim == 1 or (x.ndim == 2 and x.shape[1] == self.input_channels)):
            raise ValueError(f"push: samples of shape {x.shape} (expected interleaved 1-D or (n, {self.input_channels}))")
        return np.ascontiguousarray(x, dtype=self._in_dtype).reshape(-1)

    def pending(self, stream_id: Hashable) -> int:
        """Windows of the stream still waiting for the worker (0 for an unknown / closed stream)."""
        with self._lock:
            st = self._streams.get(stream_id)
            return 0 if st is None else self._pending(st)

    def _pending(self, st: _Stream) -> int:
        # block number c (1-based) completes a window iff c >= blocks_per_window
        last = st.consumed + len(st.blocks)
        return max(0, last - max(st.consumed, self.blocks_per_window - 1))

    def _take_host_window(self, st: _Stream):
        """Host-window mode: consume blocks until one completes a window -> (window copy, start)."""
        while st.blocks:
            new = pcm_to_mono(st.blocks.pop(0), self.input_format, self.input_channels)
            st.consumed += 1
            st.chunk = new if st.chunk is None else np.concatenate([st.chunk, new])
            if st.chunk.size > self.chunk_samples:
                st.chunk = st.chunk[-self.chunk_samples:]
                st.start += self.step_seconds
            if st.chunk.size == self.chunk_samples:
                return st.chunk.copy(), st.start
        return None

    def _take_ring_blocks(self, st: _Stream):
        """Ring mode: the blocks to upload this step (until one completes a window) -> (blocks,
        start time of the completed window | None)."""
        taken = []
        while st.blocks:
            taken.append(st.blocks.pop(0))
            st.consumed += 1
            if st.consumed >= self.blocks_per_window:
                return taken, (st.consumed - self.blocks_per_window) * self.step_seconds
        return taken, None

    # ------------------------------------------------------------------ the worker
    def step(self) -> Dict[Hashable, Annotation]:
        """Process at most one pending window of every open stream, as ONE batch.  Returns the
        speech turns each of those streams gained (the per-chunk ``Annotation`` of the reference's
        pipeline); the running total is kept per stream until ``close``."""
        with self._step_lock:                       # one engine, one step at a time
            uploads = []                            # ring mode: (slot, [blocks]) of this step
            undo = []                               # (stream, blocks, consumed, chunk, start) before the take
            pushed: Dict[int, int] = {}             # ring mode: blocks of a slot that reached its ring
            with self._lock:
                work = []                           # (stream id, stream, host window | None, start)
                for sid, st in self._streams.items():
                    if not st.blocks:
                        continue
                    undo.append((st, list(st.blocks), st.consumed, st.chunk, st.start))
                    if self.rings is None:
                        got = self._take_host_window(st)
                        if got is not None:
                            work.append((sid, st, got[0], got[1]))
                    else:
                        taken, start = self._take_ring_blocks(st)
                        uploads.append((st.slot, taken))
                        if start is not None:
                            work.append((sid, st, None, start))
                # slots whose ring row / clustering state the worker touches until the step is over
                self._inflight = {st.slot for _, st, _, _ in work} | {slot for slot, _ in uploads}
            try:
                if uploads:
                    self._upload(uploads, pushed)
                if not work:
                    if uploads:     # warm-up blocks only: the staging planes are free once the GPU has read them
                        self._sync_uploads()
                    return {}
                starts = np.array([t for _, _, _, t in work], dtype=np.float64)
                slots = [st.slot for _, st, _, _ in work]
                self._step_names = None
                if self.rings is None:
                    turns = self._engine(np.stack([w for _, _, w, _ in work]), starts, slots)
                else:
                    turns = self._gpu_engine(self.rings.gather(slots, self._window_buffer()), starts, slots)
            except BaseException as exc:
                self._roll_back(undo, pushed, exc)
                raise
            finally:
                with self._lock:
                    self._inflight = set()
                    self._free.extend(self._deferred)     # slots closed while they were in flight
                    self._deferred = []
            out = {}
            names = self._step_names if self._step_names is not None else [None] * len(work)
            with self._lock:
                for (sid, st, _, _), tr, nm in zip(work, turns, names):
                    if self._streams.get(sid) is not st:      # closed (or re-opened) mid-step: drop
                        continue
                    ann = BatchedOutputTail.annotation(np.asarray(tr, dtype=np.float64).reshape(-1, 3),
                                                       len(tr), uri=str(sid), label=self._label, names=nm)
                    st.emitted += 1
                    if st.prediction is None:
                        st.prediction = ann
                    else:
                        st.prediction.update(ann)
                    out[sid] = ann
            return out

    def _roll_back(self, undo, pushed: Dict[int, int], exc: BaseException) -> None:
        """A step failed (upload, gather or the engine raised).  The blocks it took must not vanish
        and the host-side block count of a stream must keep matching what its device ring holds:
        otherwise every later step of that stream computes wrong start times or fails in
        ``dz_ring_gather`` — which rejects the whole batch, i.e. one desynchronised stream would fail
        every step of every stream.  Host-window mode: the taken blocks go back to the
        front of the queue and the window state is restored; the step can simply be retried.  Ring
        mode: blocks that already reached the ring stay consumed (``consumed`` = count before + pushed,
        the ring's own per-row counter), the others go back; a window whose blocks were all pushed
        but whose engine run failed is lost for that stream (recorded in ``step_errors``)."""
        with self._lock:
            for st, blocks, consumed, chunk, start in undo:
                # blocks this step popped: both take functions count every pop in `consumed`.  (NOT len(blocks)
                # - len(st.blocks): a push() that lands while the engine runs — the lock is released then —
                # makes that short, and taken blocks would be dropped)  st.blocks now holds the
                # untaken blocks followed by whatever was pushed meanwhile.
                taken = st.consumed - consumed
                keep = pushed.get(st.slot, 0) if self.rings is not None else 0
                keep = min(keep, taken)
                st.blocks = blocks[keep:taken] + st.blocks
                st.consumed = consumed + keep
                if self.rings is None:
                    st.chunk, st.start = chunk, start
            self.step_errors.append((time.time(), repr(exc)))

    def _sync_uploads(self) -> None:
        if self._dev.is_cuda:
            torch.cuda.current_stream(self._dev.device).synchronize()

    def _upload(self, uploads, pushed: Optional[Dict[int, int]] = None) -> None:
        """New blocks -> the streams' device rings: round r carries the r-th new block of every stream
        that has one (a running stream has exactly one; a joining stream up to a whole window).
        ``pushed[slot]`` counts the blocks of a slot whose ring push was enqueued (for ``_roll_back``)."""
        import contextlib
        with (torch.cuda.device(self._dev.device) if self._dev.is_cuda else contextlib.nullcontext()):
            for r in range(max(len(b) for _, b in uploads)):
                rows = [slot for slot, b in uploads if len(b) > r]
                plane = self._stage[r]
                if plane.shape[1] != self._block_values:        # rows padded to a multiple of 16 bytes
                    plane = plane[:, :self._block_values]
                for j, (slot, b) in enumerate((u for u in uploads if len(u[1]) > r)):
                    plane[j].copy_(torch.from_numpy(b[r]))
                if self.input_channels == 1 and self.input_format == "f32":
                    self.rings.push_rows(plane[:len(rows)], rows)
                else:
                    self.rings.push_rows(plane[:len(rows)], rows, channels=self.input_channels, format=self.input_format)
                if pushed is not None:
                    for slot in rows:
                        pushed[slot] = pushed.get(slot, 0) + 1

    def drain(self) -> int:
        """``step`` until no block is waiting; returns the number of steps."""
        n = 0
        while True:
            with self._lock:
                if not any(st.blocks for st in self._streams.values()):
                    return n
            self.step()
            n += 1

    def serve_forever(self, idle_sleep: float = 0.002) -> None:
        while not self._stop:
            with self._lock:
                idle = not any(st.blocks for st in self._streams.values())
            if idle:
                time.sleep(idle_sleep)
            else:
                self.step()

    def shutdown(self) -> None:
        self._stop = True

    def _window_buffer(self) -> torch.Tensor:
        """Device rows the windows are assembled in, at the input rate."""
        return self._dev if self.resampler is None else self._raw

    def _resampling_engine(self, engine: Callable) -> Callable:
        def run(windows, starts, slots):
            x = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.float32))
            return engine(self.resampler(x).numpy(), starts, slots)
        return run

    def _adjusting_engine(self, engine: Callable, device) -> Callable:
        def run(windows, starts, slots):
            x = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.float32))
            return engine(adjust_volume(x, self.volume_in_db, device).numpy(), starts, slots)
        return run

    # ------------------------------------------------------------------ GPU engine
    def _gpu_engine(self, windows, starts: np.ndarray, slots: List[int]):
        """``windows``: (k, S) on the host (uploaded whole, like the reference) or already a device
        batch gathered from the rings."""
        k = windows.shape[0]
        if not torch.is_tensor(windows):
            self._pinned[:k].copy_(torch.from_numpy(windows))
            self._window_buffer()[:k].copy_(self._pinned[:k], non_blocking=True)
        if self.resampler is not None:
            with torch.cuda.device(self._dev.device):
                self.resampler.rows(self._raw[:k], self._dev[:k])
        if self.volume_in_db is not None:
            rows = self._dev[:k]
            adjust_volume_rows(rows, self.volume_in_db, out=rows)       # in place, on the current stream
        ticket = self.batch.launch(self._dev[:k], starts, slots=slots)
        if isinstance(self.batch, VadBatch):
            self.batch.finish(ticket)
        else:
            self.batch.finish(ticket, want_scores=False)
        _, _, _, _, turns, nturns = ticket["tail"]
        if getattr(self.batch, "_gallery", None) is not None:
            self._step_names = ticket["names"]
        return [turns[i, :int(nturns[i])].copy() for i in range(k)]
