"""``VoiceActivityDetection`` pipeline (reference: ``/root/reference/src/diart/blocks/vad.py``;
config :26-73, pipeline :76-191): segmentation -> max over speakers -> aggregation -> binarise.
The hot-path lines are :136-148 (segmentation + ``torch.max(..., dim=-1, keepdim=True)``)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import models as m
from ..features import Annotation, Segment, SlidingWindow, SlidingWindowFeature, Timeline
from . import base
from .aggregation import DelayedAggregation
from .diarization import _latency
from .segmentation import SpeakerSegmentation
from .utils import Binarize, windows_batch


def _repeat_label(label):
    while True:
        yield label


class VoiceActivityDetectionConfig(base.PipelineConfig):
    def __init__(self, segmentation: Optional[m.SegmentationModel] = None, duration: float = 5,
                 step: float = 0.5, latency: Union[float, str, None] = None, tau_active: float = 0.6,
                 device: Optional[torch.device] = None, sample_rate: int = 16000, tau_offset: Optional[float] = None,
                 min_duration_on: float = 0.0, min_duration_off: float = 0.0, **kwargs):
        self.segmentation = segmentation or m.SegmentationModel.from_pyannote("pyannote/segmentation")
        self._duration, self._step, self._sample_rate = duration, step, sample_rate
        self._latency = _latency(latency, step, duration)
        self.tau_active = tau_active
        # hysteresis: a frame stays on while its score is > tau_offset; None = tau_active, the single threshold
        self.tau_offset = base.check_tau_offset(tau_offset, f"{type(self).__name__}")
        # minimum durations, in seconds: gaps shorter than min_duration_off are filled, then turns shorter than
        # min_duration_on are dropped.  They act where a whole file is known (the accumulated prediction of
        # StreamingInference and Benchmark, the file batch, the tuner); a live step has no look-ahead, so the pipeline's
        # per-chunk __call__ and the N-stream engines neither take nor apply them
        self.min_duration_on = base.check_min_duration(min_duration_on, "min_duration_on", f"{type(self).__name__}")
        self.min_duration_off = base.check_min_duration(min_duration_off, "min_duration_off", f"{type(self).__name__}")
        self.device = device or torch.device("cuda" if torch.cuda.is_available() else "cpu")

    @property
    def duration(self) -> float:
        return self._duration

    @property
    def step(self) -> float:
        return self._step

    @property
    def latency(self) -> float:
        return self._latency

    @property
    def sample_rate(self) -> int:
        return self._sample_rate


class _TrackDetection(base.Pipeline):
    """What the pipelines that binarise ONE track of the segmentation share (``VoiceActivityDetection``: the max over
    speakers; ``OverlappedSpeechDetection``, blocks/osd.py: the second largest): the blocks, the buffers and the host
    half behind the track (reference vad.py:150-191).  A private base, not a pipeline: the two are siblings."""

    LABEL: str                  # what every turn is called
    CONFIG: type                # the pipeline's configuration class

    def __init__(self, config=None):
        self._config = self.CONFIG() if config is None else config
        c = self._config
        msg = f"Latency should be in the range [{c.step}, {c.duration}]"
        assert c.step <= c.latency <= c.duration, msg
        self.segmentation = SpeakerSegmentation(c.segmentation, c.device)
        self.pred_aggregation = DelayedAggregation(c.step, c.latency, strategy="hamming", cropping_mode="loose")
        self.audio_aggregation = DelayedAggregation(c.step, c.latency, strategy="first", cropping_mode="center")
        self.binarize = Binarize(c.tau_active, offset=getattr(c, "tau_offset", None))
        self.timestamp_shift = 0
        self.chunk_buffer, self.pred_buffer = [], []

    @staticmethod
    def hyper_parameters() -> Sequence[base.HyperParameter]:
        return [base.TauActive]

    @property
    def config(self):
        return self._config

    def reset(self):
        self.set_timestamp_shift(0)
        self.chunk_buffer, self.pred_buffer = [], []
        self.binarize.reset()

    def set_timestamp_shift(self, shift: float):
        self.timestamp_shift = shift

    def _windows(self, waveforms: Sequence[SlidingWindowFeature]) -> torch.Tensor:
        """``__call__``'s checks of its chunks, then their batch on the device."""
        assert len(waveforms) >= 1, "Pipeline expected at least 1 input"
        expected = int(np.rint(self.config.duration * self.config.sample_rate))
        got = waveforms[0].data.shape[0]
        assert all(w.data.shape[0] == got for w in waveforms), "chunks of different lengths in one batch"
        assert got == expected, f"Expected {expected} samples per chunk, but got {got}"
        return windows_batch(waveforms, self.config.device)

    def _finalise_track(self, waveforms: Sequence[SlidingWindowFeature], track: torch.Tensor):
        """Aggregation, binarisation and labelling of the chunks' track ``(batch, frames, 1)``."""
        seg_resolution = waveforms[0].extent.duration / track.shape[1]
        outputs = []
        for wav, row in zip(waveforms, track):
            sw = SlidingWindow(start=wav.extent.start, duration=seg_resolution, step=seg_resolution)
            row = SlidingWindowFeature(row.cpu().numpy(), sw)
            self.chunk_buffer.append(wav)
            self.pred_buffer.append(row)
            agg_waveform = self.audio_aggregation(self.chunk_buffer)
            timeline = self.binarize(self.pred_aggregation(self.pred_buffer)).get_timeline(copy=False)
            if self.timestamp_shift != 0:
                shifted = Timeline(uri=timeline.uri)
                for segment in timeline:
                    shifted.add(Segment(segment.start + self.timestamp_shift, segment.end + self.timestamp_shift))
                timeline = shifted
            outputs.append((timeline.to_annotation(_repeat_label(self.LABEL)), agg_waveform))
            if len(self.chunk_buffer) == self.pred_aggregation.num_overlapping_windows:
                self.chunk_buffer = self.chunk_buffer[1:]
                self.pred_buffer = self.pred_buffer[1:]
        return outputs


class VoiceActivityDetection(_TrackDetection):
    LABEL = "speech"
    CONFIG = VoiceActivityDetectionConfig

    @staticmethod
    def get_config_class() -> type:
        return VoiceActivityDetectionConfig

    @staticmethod
    def suggest_metric():
        from ..metrics import DetectionErrorRate
        return DetectionErrorRate(collar=0, skip_overlap=False)

    @property
    def config(self) -> VoiceActivityDetectionConfig:
        return self._config

    def __call__(self, waveforms: Sequence[SlidingWindowFeature]) -> Sequence[Tuple[Annotation, SlidingWindowFeature]]:
        return self.finalise(waveforms, self.segmentation(self._windows(waveforms)))

    def model_outputs(self, waveforms: Sequence[SlidingWindowFeature]) -> torch.Tensor:
        """The model half of ``__call__``: what ``finalise`` computes as ``voice_detection``, ``(batch, frames, 1)``
        float32 on the host.  Nothing here depends on ``tau_active``: ``optim.VadTuneCache`` keeps these tracks and
        replays the aggregation and the binarisation per trial."""
        batch = windows_batch(waveforms, self.config.device)
        return torch.max(self.segmentation(batch), dim=-1, keepdim=True)[0].float().cpu()

    def finalise(self, waveforms: Sequence[SlidingWindowFeature], segmentations: torch.Tensor):
        """The host half of ``__call__`` (reference vad.py:146-191) for given segmentation scores."""
        return self._finalise_track(waveforms, torch.max(segmentations, dim=-1, keepdim=True)[0])   # (batch, frames, 1)
