"""File-parallel evaluation of a pipeline — BASELINE.json configs 1 and 4.

The drivers on either side of the hot path, restated without ``rx`` / ``torchaudio``:

* ``file_blocks``       ``FileAudioSource.read``       reference ``sources.py:85-135``
* ``rolling_windows``   ``rearrange_audio_stream``     reference ``operators.py:44-100``
* ``StreamingInference`` (file sources, batched)       reference ``inference.py:22-253``
* ``PredictionAccumulator``                            reference ``sinks.py:59-88``
* ``Benchmark``                                        reference ``inference.py:255-432``
* ``DistributedBenchmark`` — what ``Parallelize`` (``inference.py:435-559``) does with a pool of
  spawned workers that each copy the models, done the MI355X way: one process per GPU
  (``torchrun``), whole files assigned to ranks by longest-processing-time (no file is split,
  no data-path collective), the weights broadcast once (``distributed.broadcast_state``) and the
  per-file error components gathered at the end.

Any ``blocks.Pipeline`` subclass drops in (``SpeakerDiarization``, ``VoiceActivityDetection``);
nothing here touches the GPU itself.
"""
from __future__ import annotations

import wave
from pathlib import Path
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import distributed as D
from .features import Annotation, SlidingWindow, SlidingWindowFeature, load_rttm

FilePath = Union[str, Path]


# ------------------------------------------------------------------------------------- audio
_WAVE_TAGS = {1: "integer PCM", 3: "IEEE float", 6: "A-law", 7: "mu-law"}


def _riff(path: FilePath, with_data: bool = True) -> dict:
    """The ``fmt `` and ``data`` chunks of a RIFF/WAVE file: format tag (the sub-format's of an extensible header),
    channels, rate, bits per value, the number of whole frames and, ``with_data``, their bytes.  Unknown chunks are
    skipped, an odd-sized chunk is followed by its pad byte.  ``ValueError`` names the file and what is wrong with it;
    the file is only ever read as data."""
    import struct
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        end = f.seek(0, 2)
        pos, fmt = 12, None
        while pos + 8 <= end:
            f.seek(pos)
            cid, size = struct.unpack("<4sI", f.read(8))
            if cid == b"fmt ":
                body = f.read(min(size, 40))
                if len(body) < 16:
                    raise ValueError(f"{path}: fmt chunk of {len(body)} bytes")
                tag, nch, sr, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == 0xFFFE:                      # extensible: the tag is the first two bytes of the sub-format
                    if len(body) < 26:
                        raise ValueError(f"{path}: extensible fmt chunk of {len(body)} bytes")
                    tag, = struct.unpack("<H", body[24:26])
                fmt = (tag, nch, sr, bits)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: data chunk before the fmt chunk")
                tag, nch, sr, bits = fmt
                if tag not in _WAVE_TAGS:
                    raise ValueError(f"{path}: unsupported WAVE format tag {tag} (0x{tag:04x}); supported: "
                                     + ", ".join(f"{t} ({n})" for t, n in _WAVE_TAGS.items()))
                if bits not in {1: (8, 16, 24, 32), 3: (32, 64), 6: (8,), 7: (8,)}[tag]:
                    raise ValueError(f"{path}: {bits}-bit {_WAVE_TAGS[tag]} (format tag {tag}) is not supported")
                if nch < 1 or sr < 1:
                    raise ValueError(f"{path}: {nch} channels at {sr} Hz")
                frame = nch * (bits // 8)
                n = min(size, end - pos - 8) // frame          # (a streamed file's size field may exceed the file)
                info = {"tag": tag, "channels": nch, "rate": sr, "width": bits // 8, "frames": n}
                if with_data:
                    info["data"] = f.read(n * frame)
                return info
            pos += 8 + size + (size & 1)
    raise ValueError(f"{path}: no data chunk")


def _decode_wav(path: FilePath, info: dict) -> np.ndarray:
    """The samples of ``_riff(path)`` as mono float32."""
    raw, nch, width, tag = info["data"], info["channels"], info["width"], info["tag"]
    if tag == 3:
        x = np.frombuffer(raw, dtype="<f4" if width == 4 else "<f8").astype(np.float32)
    elif tag in (6, 7):
        from .pcm import pcm_to_float
        x = pcm_to_float(np.frombuffer(raw, dtype=np.uint8), "alaw" if tag == 6 else "ulaw")
    elif width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 3:
        # 24-bit little-endian PCM: the 3 bytes as the top of an int32 (what a 32-bit file of the same samples holds),
        # so the decode is the 32-bit one (value / 2^31, exact)
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3)
        w = np.zeros((b.shape[0], 4), dtype=np.uint8)
        w[:, 1:] = b
        x = w.view("<i4")[:, 0].astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"{path}: unsupported sample width {width}")
    x = x.reshape(-1, nch)
    return (x.mean(axis=1) if nch > 1 else x[:, 0]).astype(np.float32)


def read_wav_into(path: FilePath, alloc, padding_of, block_duration: float = 0.5):
    """``padded_file(read_wav(path))`` in ONE pass: decode the samples straight into
    ``alloc(n_total)`` (e.g. a pinned upload buffer) at their padded position.  ``padding_of(duration
    seconds) -> (left, right)`` seconds.  -> (array, sample rate, (left, right)); same samples as the
    two-step form (the 2^-15 / 2^-31 / 2^-7 scalings are exact in float32)."""
    info = _riff(path)
    sr, nch, width, n = info["rate"], info["channels"], info["width"], info["frames"]
    padding = padding_of(n / sr)
    left, right = (int(np.rint(p * sr)) for p in padding)
    size = int(np.rint(block_duration * sr))
    total = left + n + right
    out = alloc(-(-total // size) * size)
    out[:left] = 0.0
    out[left + n:] = 0.0
    dst = out[left:left + n]
    if nch == 1 and width == 2 and info["tag"] == 1:
        np.multiply(np.frombuffer(info["data"], dtype="<i2"), np.float32(1.0 / 32768.0), out=dst, dtype=np.float32,
                    casting="unsafe")
    else:
        dst[:] = _decode_wav(path, info)
    return out, sr, padding


def read_wav(path: FilePath) -> Tuple[np.ndarray, int]:
    """WAV -> (mono float32, sample rate): integer PCM (8/16/24/32-bit, in [-1, 1)), IEEE float (32-bit; 64-bit cast to
    float32), G.711 A-law and mu-law (``diart_amd.pcm``), plain or in an extensible header; another format tag is a
    ``ValueError`` that names it.  Channels are averaged like ``AudioLoader(mono=True)`` (reference
    ``audio.py:36-40``).  A RIFF reader of the project's own (``_riff``): the standard library's ``wave`` refuses
    everything but integer PCM."""
    info = _riff(path)
    return _decode_wav(path, info), info["rate"]


def resample_file(waveform: np.ndarray, orig_freq: int, new_freq: int, device=None) -> np.ndarray:
    """A whole mono signal at ``new_freq`` (float32 on the host), resampled on the GPU ``device`` (None: the current
    one) by ``functional.resample``."""
    from .functional import resample
    return resample(np.asarray(waveform, dtype=np.float32).reshape(-1), orig_freq, new_freq, device)


def read_wav_resampled_into(path: FilePath, alloc, padding_of, block_duration: float, sample_rate: int,
                            device=None):
    """``read_wav_into`` at the pipeline's rate: a file at another rate is decoded, resampled as a whole on the GPU,
    then padded (``padding_of`` gets the file's own duration, as the reference's ``get_file_padding`` does) and
    blocked at ``sample_rate`` into ``alloc``.  A file at ``sample_rate`` takes ``read_wav_into`` itself."""
    sr = _riff(path, with_data=False)["rate"]
    if sr == sample_rate:
        return read_wav_into(path, alloc, padding_of, block_duration)
    x, sr = read_wav(path)
    padding = padding_of(len(x) / sr)
    y = resample_file(x, sr, sample_rate, device)
    left, right = (int(np.rint(p * sample_rate)) for p in padding)
    size = int(np.rint(block_duration * sample_rate))
    total = left + len(y) + right
    out = alloc(-(-total // size) * size)
    out[:] = 0.0
    out[left:left + len(y)] = y
    return out, sample_rate, padding


def write_wav(path: FilePath, samples: np.ndarray, sample_rate: int = 16000) -> None:
    """Mono float waveform -> 16-bit PCM WAV."""
    pcm = np.clip(np.rint(np.asarray(samples, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sample_rate)
        f.writeframes(pcm.tobytes())


def wav_duration(path: FilePath) -> float:
    info = _riff(path, with_data=False)
    return info["frames"] / float(info["rate"])


def file_blocks(waveform: np.ndarray, sample_rate: int, padding: Tuple[float, float] = (0, 0),
                block_duration: float = 0.5) -> Iterator[np.ndarray]:
    """Blocks ``(1, block_size)`` of a mono file as ``FileAudioSource.read`` emits them: zero
    padding left / right in seconds, a trailing incomplete block zero-filled (and up-cast to
    float64 by the concatenation with ``np.zeros``, as in the reference ``sources.py:117-121``)."""
    wav = np.asarray(waveform, dtype=np.float32).reshape(-1)
    left, right = (int(np.rint(p * sample_rate)) for p in padding)
    if left > 0:
        wav = np.concatenate([np.zeros(left, dtype=np.float32), wav])
    if right > 0:
        wav = np.concatenate([wav, np.zeros(right, dtype=np.float32)])
    size = int(np.rint(block_duration * sample_rate))
    full = wav.shape[0] // size
    for i in range(full):
        yield wav[None, i * size:(i + 1) * size]
    if wav.shape[0] % size != 0:
        last = wav[full * size:]
        yield np.concatenate([last[None, :], np.zeros((1, size - last.shape[0]))], axis=-1)


def padded_file(waveform: np.ndarray, sample_rate: int, padding: Tuple[float, float] = (0, 0),
                block_duration: float = 0.5) -> np.ndarray:
    """The concatenation of everything ``file_blocks`` emits, as one float32 array: zero padding
    left / right, the trailing incomplete block zero-filled.  (``file_blocks`` up-casts that last
    block to float64 like the reference; every consumer casts back with ``.float()``,
    ``features.py:124``, so float32 zeros are the same samples.)"""
    wav = np.asarray(waveform, dtype=np.float32).reshape(-1)
    left, right = (int(np.rint(p * sample_rate)) for p in padding)
    size = int(np.rint(block_duration * sample_rate))
    total = left + wav.shape[0] + right
    out = np.zeros(-(-total // size) * size, dtype=np.float32)
    out[left:left + wav.shape[0]] = wav
    return out


def rolling_windows(blocks: Iterable[np.ndarray], duration: float = 5.0, step: float = 0.5,
                    sample_rate: int = 16000) -> Iterator[SlidingWindowFeature]:
    """``rearrange_audio_stream``: buffer blocks until ``step`` seconds are available, append them
    to the current chunk, keep its last ``duration`` seconds (the start time advances by ``step``
    whenever samples are dropped) and emit every changed chunk that is exactly ``duration`` long,
    as a ``(samples, 1)`` feature whose frame grid starts at the chunk's start time."""
    chunk_samples, step_samples = int(round(sample_rate * duration)), int(round(sample_rate * step))
    chunk, buffer, start = None, None, 0
    for value in blocks:
        if value.ndim != 2 or value.shape[0] != 1:
            raise ValueError(f"Waveform must have shape (1, samples) but {value.shape} was found")
        buffer = value if buffer is None else np.concatenate([buffer, value], axis=1)
        if buffer.shape[1] < step_samples:
            continue
        new, buffer = (buffer, None) if buffer.shape[1] == step_samples else \
            (buffer[:, :step_samples], buffer[:, step_samples:])
        chunk = new if chunk is None else np.concatenate([chunk, new], axis=1)
        if chunk.shape[1] > chunk_samples:
            chunk = chunk[:, -chunk_samples:]
            start += step
        if chunk.shape[1] == chunk_samples:
            yield SlidingWindowFeature(chunk.T, SlidingWindow(start=start, duration=1.0 / sample_rate,
                                                              step=1.0 / sample_rate))


# -------------------------------------------------------------------------------- inference
class PredictionAccumulator:
    """Joins the per-chunk annotations of one stream; same-speaker turns closer than
    ``patch_collar`` are stitched (``Annotation.support``).  ``min_duration_on`` / ``min_duration_off`` (the track
    pipelines' configuration; seconds): ``functional.min_duration`` in ``get_prediction``, where the whole stream is
    known — gaps shorter than ``min_duration_off`` filled, then turns shorter than ``min_duration_on`` dropped.  Both 0:
    the stitching alone."""

    def __init__(self, uri: Optional[str] = None, patch_collar: float = 0.05, min_duration_on: float = 0.0,
                 min_duration_off: float = 0.0):
        from .blocks.base import check_min_duration
        self.uri, self.patch_collar = uri, patch_collar
        self.min_duration_on = check_min_duration(min_duration_on, "min_duration_on", "PredictionAccumulator")
        self.min_duration_off = check_min_duration(min_duration_off, "min_duration_off", "PredictionAccumulator")
        self._prediction: Optional[Annotation] = None

    def on_next(self, value):
        prediction = value[0] if isinstance(value, tuple) else value
        prediction.uri = self.uri
        if self._prediction is None:
            self._prediction = prediction
        else:
            self._prediction.update(prediction)

    def get_prediction(self) -> Optional[Annotation]:
        if self._prediction is None:
            return None
        self._prediction = self._prediction.support(self.patch_collar)
        if self.min_duration_on == 0.0 and self.min_duration_off == 0.0:
            return self._prediction
        # the accumulated turns stay as they are (a later on_next may still bridge a gap); the durations act on a copy
        from .functional import min_duration
        return min_duration(self._prediction, self.min_duration_on, self.min_duration_off, self.patch_collar)


class StreamingInference:
    """One file through one pipeline: blocks -> rolling windows -> batches of ``batch_size``
    consecutive windows -> ``pipeline(batch)`` -> accumulated ``Annotation``."""

    def __init__(self, pipeline, waveform: np.ndarray, sample_rate: int, uri: str = "stream",
                 padding: Tuple[float, float] = (0, 0), batch_size: int = 1, hooks: Sequence = ()):
        cfg = pipeline.config
        if sample_rate != cfg.sample_rate:
            # the whole file at the pipeline's rate, as FileAudioSource loads it (reference audio.py:31-37), on the
            # pipeline's GPU; the padding (seconds) is applied after.  A pipeline without a GPU device has nowhere
            # to resample.
            if getattr(getattr(cfg, "device", None), "type", None) != "cuda":
                raise ValueError(f"audio source has sample rate {sample_rate}, the pipeline's is {cfg.sample_rate} "
                                 "and the pipeline has no GPU device to resample on; resample the file first")
            waveform = resample_file(waveform, sample_rate, cfg.sample_rate, cfg.device)
            sample_rate = cfg.sample_rate
        self.pipeline, self.batch_size, self.hooks = pipeline, max(1, int(batch_size)), list(hooks)
        # the track pipelines' minimum durations act on the accumulated prediction, never on a step's output
        self.accumulator = PredictionAccumulator(uri, min_duration_on=getattr(cfg, "min_duration_on", 0.0),
                                                 min_duration_off=getattr(cfg, "min_duration_off", 0.0))
        self._windows = rolling_windows(file_blocks(waveform, sample_rate, padding, cfg.step),
                                        cfg.duration, cfg.step, sample_rate)
        total = padding[0] + len(waveform) / sample_rate + padding[1]
        self.num_chunks = int(np.ceil((total - cfg.duration + cfg.step) / cfg.step))
        self.chunks_done = 0

    def __call__(self) -> Optional[Annotation]:
        batch: List[SlidingWindowFeature] = []

        def flush():
            for out in self.pipeline(batch):
                self.accumulator.on_next(out)
                for hook in self.hooks:
                    hook(out)
            self.chunks_done += len(batch)
            batch.clear()

        for window in self._windows:
            batch.append(window)
            if len(batch) == self.batch_size:
                flush()
        if batch:
            flush()
        return self.accumulator.get_prediction()


# Which forms of the file batch `Benchmark` takes WITHOUT being asked (``concurrent_files=None``): a form whose file batch
# measured slower than its loop stays on the loop unless ``concurrent_files`` is given (profiles/r24a_file_batch_models.json,
# README "File batches for every model").
FILE_BATCH_BY_DEFAULT = {"xvector": True, "wespeaker": True, "groups": True, "vad": True, "osd": True}


def file_batch_kind(pipeline_class: type, segmentation_type: type, embedding_type: Optional[type], batch_size: int,
                    concurrent_files: int = 16, device_type: str = "cuda", explicit: bool = True) -> Optional[str]:
    """Which ``FileBatch`` form runs (pipeline class, model classes, batch size), or None for the one-file-at-a-time
    loop.  No device is touched: the arguments are classes, numbers and a device TYPE.

        SpeakerDiarization   HipSegmentation + HipEmbedding (pyannote/embedding)            "xvector"
        SpeakerDiarization   HipSegmentation + HipWeSpeakerEmbedding                        "wespeaker"
        SpeakerDiarization   HipSegmentation + a groups-form embedding, batch_size == 1     "groups"
        VoiceActivityDetection   HipSegmentation                                            "vad"
        OverlappedSpeechDetection   HipSegmentation                                         "osd"

    A groups-form model (ECAPA, speechbrain x-vector, TitaNet-L, speechbrain ResNet, mel-spectrogram ECAPA) pads and
    normalises a row by the geometry of the rows it is batched with: at ``batch_size=32`` the loop's embeddings depend on
    the batch, as the reference's do, while ``GroupsBatch`` embeds each chunk's K rows alone — the loop at
    ``batch_size=1``.  Only there do the two agree, so only there is the file batch taken; any other batch size keeps the
    numbers it gives today.

    None as well for ``concurrent_files <= 0``, a device that is not "cuda", a SUBCLASS of any of the pipelines (it may
    override any stage), models that are not exactly these classes, and — when ``concurrent_files`` was not given
    (``explicit=False``) — a form that ``FILE_BATCH_BY_DEFAULT`` leaves on the loop."""
    from .blocks.diarization import SpeakerDiarization
    from .blocks.osd import OverlappedSpeechDetection
    from .blocks.vad import VoiceActivityDetection
    from .models import HipEmbedding, HipSegmentation, HipWeSpeakerEmbedding, _HipGroupsEmbedding
    if int(concurrent_files) <= 0 or device_type != "cuda" or segmentation_type is not HipSegmentation:
        return None
    kind = None
    if pipeline_class is VoiceActivityDetection:
        kind = "vad"
    elif pipeline_class is OverlappedSpeechDetection:
        kind = "osd"
    elif pipeline_class is SpeakerDiarization and isinstance(embedding_type, type):
        if embedding_type is HipEmbedding:
            kind = "xvector"
        elif embedding_type is HipWeSpeakerEmbedding:
            kind = "wespeaker"
        elif issubclass(embedding_type, _HipGroupsEmbedding) and int(batch_size) == 1:
            kind = "groups"
    if kind is not None and not explicit and not FILE_BATCH_BY_DEFAULT[kind]:
        return None
    return kind


class Benchmark:
    """Run a pipeline class on every WAV of ``speech_path``; write ``<uri>.rttm`` files to
    ``output_path`` and / or score against ``reference_path/<uri>.rttm``.  Same constructor and call
    as the reference's; the report is the metric object (``abs(metric)`` = aggregate rate,
    ``metric.report()`` = the per-file table) instead of a pandas frame of pyannote.metrics.

    ``concurrent_files`` files of this process share one GPU batch (``FileBatch``) where ``file_batch_kind`` names a
    form for the pipeline and its models: ``SpeakerDiarization`` with pyannote/embedding, with the WeSpeaker ResNet34, or
    (at ``batch_size=1`` only) with a groups-form embedding, ``VoiceActivityDetection`` and ``OverlappedSpeechDetection``.  Everything else — and
    everything at ``concurrent_files=0`` — runs the reference's loop, one file at a time in batches of ``batch_size``
    windows.  The RTTM files are the same either way; ``last_path`` says which path ran."""

    def __init__(self, speech_path: FilePath, reference_path: Optional[FilePath] = None,
                 output_path: Optional[FilePath] = None, show_progress: bool = False,
                 show_report: bool = True, batch_size: int = 32, concurrent_files: Optional[int] = None):
        self.speech_path = Path(speech_path).expanduser()
        assert self.speech_path.is_dir(), "Speech path must be a directory"
        assert reference_path is not None or output_path is not None, \
            "Benchmark expected reference path, output path or both"
        self.reference_path = None
        if reference_path is not None:
            self.reference_path = Path(reference_path).expanduser()
            assert self.reference_path.is_dir(), "Reference path must be a directory"
        self.output_path = None
        if output_path is not None:
            self.output_path = Path(output_path).expanduser()
            self.output_path.mkdir(parents=True, exist_ok=True)
        self.show_progress, self.show_report, self.batch_size = show_progress, show_report, batch_size
        # files of this process that share one GPU batch (``FileBatch``); None = 16, 0 = the reference's
        # one-file-at-a-time loop.  `file_batch_kind` says which pipelines and models have the batched path; anything
        # else falls back to the loop.
        from .config import overrides, setting
        self.concurrent_files = int(setting("concurrent_files", concurrent_files, 16, int))
        self._files_given = concurrent_files is not None or overrides().get("concurrent_files") is not None
        # windows per GPU step of the file batch (at least `batch_size`).  An attribute, not an argument: the engine under
        # the files allocates by it (a 64-row ECAPA engine holds about 6 GB per lane), so a small job may lower it
        self.file_batch_rows = 64
        self.last_path = None      # "file_batch" | "one_file_at_a_time": which path the last call took

    def get_file_paths(self) -> List[Path]:
        return sorted(p for p in self.speech_path.iterdir() if p.suffix.lower() == ".wav")

    def run_single(self, pipeline, filepath: Path) -> Annotation:
        """Does NOT reset the pipeline (like the reference's ``run_single``)."""
        waveform, sr = read_wav(filepath)
        padding = pipeline.config.get_padding(len(waveform) / sr)
        pipeline.set_timestamp_shift(-padding[0])
        pred = StreamingInference(pipeline, waveform, sr, filepath.stem, padding, self.batch_size)()
        if pred is None:
            pred = Annotation(filepath.stem)
        pred.uri = filepath.stem
        if self.output_path is not None:
            with open(self.output_path / f"{filepath.stem}.rttm", "w") as out_file:
                pred.write_rttm(out_file)
        if self.show_progress:
            print(f"[benchmark] {filepath.stem}: {len(pred)} turns", flush=True)
        return pred

    def file_batch(self, pipeline_class: type, config):
        """A ``FileBatch`` for (pipeline_class, config), or None when this combination has to go through the
        one-file-at-a-time loop: the rule is ``file_batch_kind`` (custom pipeline classes, non-HIP models, CPU devices,
        groups-form embeddings at a batch size other than 1, ``concurrent_files=0``)."""
        from .blocks.diarization import SpeakerDiarization
        from .blocks.osd import OverlappedSpeechDetection
        from .blocks.vad import VoiceActivityDetection
        if self.concurrent_files <= 0 or pipeline_class not in (SpeakerDiarization, VoiceActivityDetection,
                                                                OverlappedSpeechDetection):
            return None                 # (a custom pipeline's config may have neither models nor a device)
        if getattr(getattr(config, "device", None), "type", "cpu") != "cuda":
            return None
        seg, emb = config.segmentation, getattr(config, "embedding", None)
        seg.load()
        if emb is not None:
            emb.load()
        kind = file_batch_kind(pipeline_class, type(seg.model), None if emb is None else type(emb.model),
                               self.batch_size, self.concurrent_files, config.device.type, self._files_given)
        if kind is None:
            return None
        from .pipeline import FileBatch
        # one engine per (form, models, hyper-parameters): its scratch arenas (1 - 12 GB) and pinned slots are
        # allocated once, not per call
        one_track = kind in ("vad", "osd")
        hyper = () if one_track else (config.rho_update, config.delta_new, config.gamma, config.beta,
                                          config.max_speakers, config.normalize_embedding_weights)
        key = (kind, id(seg.model), None if one_track else id(emb.model), config.tau_active,
               getattr(config, "tau_offset", None) if one_track else None,
               (getattr(config, "min_duration_on", 0.0), getattr(config, "min_duration_off", 0.0)) if one_track else None,
               hyper, config.duration,
               config.step, config.latency, config.sample_rate, str(config.device), self.batch_size,
               self.concurrent_files, self.file_batch_rows)
        cached = getattr(self, "_fb_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        fb = self._new_file_batch(FileBatch, seg, None if one_track else emb, config, kind)
        self._fb_cache = (key, fb)
        return fb

    def _new_file_batch(self, FileBatch, seg, emb, config, kind: Optional[str] = None):
        common = dict(rows=max(int(self.file_batch_rows), self.batch_size), max_files=self.concurrent_files, tau_active=config.tau_active,
                      duration=config.duration, step=config.step, latency=config.latency,
                      sample_rate=config.sample_rate, device=config.device)
        if emb is None:
            return FileBatch(seg.model, None, pipeline="osd" if kind == "osd" else "vad",
                             tau_offset=getattr(config, "tau_offset", None),
                             min_duration_on=getattr(config, "min_duration_on", 0.0),
                             min_duration_off=getattr(config, "min_duration_off", 0.0), **common)
        return FileBatch(seg.model, emb.model, rho_update=config.rho_update, delta_new=config.delta_new,
                         gamma=config.gamma, beta=config.beta, max_speakers=config.max_speakers,
                         normalize_embedding_weights=config.normalize_embedding_weights, **common)

    def run_batched(self, fb, config, paths: Sequence[Path]) -> List[Annotation]:
        """``paths`` through one ``FileBatch``: same padding, timestamp shift, RTTM files and
        progress lines as ``run_single``, files read lazily as slots free up."""
        def feed():      # runs on the FileBatch's loader thread: decode straight into pinned memory
            for fp in paths:
                padded, _, padding = read_wav_resampled_into(fp, fb.host_buffer, config.get_padding, config.step,
                                                             config.sample_rate, config.device)
                yield fp.stem, padded, -padding[0]

        got = fb.run(feed())
        preds = []
        for fp in paths:
            pred = got[fp.stem]
            pred.uri = fp.stem
            if self.output_path is not None:
                with open(self.output_path / f"{fp.stem}.rttm", "w") as out_file:
                    pred.write_rttm(out_file)
            if self.show_progress:
                print(f"[benchmark] {fp.stem}: {len(pred)} turns", flush=True)
            preds.append(pred)
        return preds

    def evaluate(self, predictions: List[Annotation], metric):
        if self.reference_path is None:
            return predictions
        for hyp in predictions:
            ref = load_rttm(self.reference_path / f"{hyp.uri}.rttm").popitem()[1]
            metric(ref, hyp)
        if self.show_report:
            print(metric.report(), flush=True)
        return metric

    def __call__(self, pipeline_class: type, config, metric=None):
        pipeline = pipeline_class(config)
        fb = self.file_batch(pipeline_class, config)
        self.last_path = "file_batch" if fb is not None else "one_file_at_a_time"
        if fb is not None:
            predictions = self.run_batched(fb, config, self.get_file_paths())
        else:
            predictions = []
            for filepath in self.get_file_paths():
                pipeline.reset()
                predictions.append(self.run_single(pipeline, filepath))
        metric = pipeline.suggest_metric() if metric is None else metric
        return self.evaluate(predictions, metric)


class DistributedBenchmark:
    """``Benchmark`` over the ranks of a ``torchrun`` job (one process per GPU): rank r runs the
    files ``shard_files_lpt`` gives it, every rank writes its own RTTMs, and rank 0 receives the
    per-file error components of all ranks (``all_gather_object``: a few doubles per file — the
    only communication besides the one-time weight broadcast).  With WORLD_SIZE = 1 it is
    ``Benchmark``."""

    def __init__(self, benchmark: Benchmark):
        self.benchmark = benchmark

    def __call__(self, pipeline_class: type, config, metric=None):
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        b = self.benchmark
        files = b.get_file_paths()
        mine = D.shard_files_lpt([wav_duration(p) for p in files], world)[rank]
        pipeline = pipeline_class(config)
        metric = pipeline.suggest_metric() if metric is None else metric
        local: Dict[str, Optional[dict]] = {}
        fb = b.file_batch(pipeline_class, config)
        b.last_path = "file_batch" if fb is not None else "one_file_at_a_time"
        # longest first: the short files fill the slots the long ones leave at the end
        batched = {h.uri: h for h in b.run_batched(fb, config, [files[i] for i in mine])} if fb is not None else None
        for i in sorted(mine):
            if batched is not None:
                hyp = batched[files[i].stem]
            else:
                pipeline.reset()
                hyp = b.run_single(pipeline, files[i])
            comp = None
            if b.reference_path is not None:
                ref = load_rttm(b.reference_path / f"{hyp.uri}.rttm").popitem()[1]
                comp = metric.components(ref, hyp)
            local[hyp.uri] = comp
        gathered = [local]
        if world > 1:
            gathered = [None] * world
            dist.all_gather_object(gathered, local)
        merged: Dict[str, Optional[dict]] = {}
        for part in gathered:
            merged.update(part)
        if b.reference_path is None:
            return sorted(merged)
        metric.reset()
        for uri in sorted(merged):
            for c, v in merged[uri].items():
                metric.accumulated[c] += v
            metric.results.append((uri, merged[uri]))
        if b.show_report and rank == 0:
            print(metric.report(), flush=True)
        return metric
