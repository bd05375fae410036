"""``OverlappedSpeechDetection`` pipeline: segmentation -> second largest over speakers -> aggregation -> binarise.

The third published use of the segmentation model beside speaker diarization and voice activity detection
(pyannote's ``OverlappedSpeechDetection``): where do two or more people talk at once.  The overlap track of a frame is
the second largest of its per-speaker scores counted with multiplicity, NaN ordered above every number
(``functional.overlap_track``; DESIGN.md "Overlapped speech detection").  Everything behind the track is
``VoiceActivityDetection``'s: ``DelayedAggregation(hamming, loose)`` + ``Binarize(tau_active)``, turns labelled
``"overlap"``.

A sibling of ``VoiceActivityDetection``, not a subclass: ``inference.file_batch_kind`` and the tuner treat subclasses
of the existing pipelines as custom code and keep them off the engines.  What the two share (the blocks, the buffers,
the host half behind the track) is the private base ``vad._TrackDetection``."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from .. import models as m
from ..features import Annotation, SlidingWindowFeature
from ..functional import overlap_track
from .segmentation import _range_check
from .vad import VoiceActivityDetectionConfig, _TrackDetection


class OverlappedSpeechDetectionConfig(VoiceActivityDetectionConfig):
    """``VoiceActivityDetectionConfig``'s fields; ``tau_active`` defaults to 0.5, pyannote's onset for this task.
    ``min_duration_on`` / ``min_duration_off`` (through ``**kwargs``) are the base class's too: they act where a whole
    file is known, never in a live step."""

    def __init__(self, segmentation: Optional[m.SegmentationModel] = None, duration: float = 5,
                 step: float = 0.5, latency: Union[float, str, None] = None, tau_active: float = 0.5,
                 device: Optional[torch.device] = None, sample_rate: int = 16000, tau_offset: Optional[float] = None,
                 **kwargs):
        super().__init__(segmentation, duration, step, latency, tau_active, device, sample_rate, tau_offset=tau_offset,
                         **kwargs)


class OverlappedSpeechDetection(_TrackDetection):
    LABEL = "overlap"
    CONFIG = OverlappedSpeechDetectionConfig

    def __init__(self, config: Optional[OverlappedSpeechDetectionConfig] = None):
        super().__init__(config)
        speakers = getattr(self._config.segmentation.model, "num_speakers", None)    # (on the device by now)
        if speakers is not None and int(speakers) < 2:
            raise ValueError(f"OverlappedSpeechDetection: a segmentation model with {speakers} speaker has no "
                             "overlap track (at least 2 speakers)")

    @staticmethod
    def get_config_class() -> type:
        return OverlappedSpeechDetectionConfig

    @staticmethod
    def suggest_metric():
        from ..metrics import OverlapDetectionErrorRate
        return OverlapDetectionErrorRate(collar=0, skip_overlap=False)

    @property
    def config(self) -> OverlappedSpeechDetectionConfig:
        return self._config

    def __call__(self, waveforms: Sequence[SlidingWindowFeature]) -> Sequence[Tuple[Annotation, SlidingWindowFeature]]:
        # the scores stay on the model's device: finalise reduces them there and copies the (batch, frames, 1) track
        outputs = self.finalise(waveforms, self.segmentation.forward_device(self._windows(waveforms)))
        _range_check(self.config.device)
        return outputs

    def model_outputs(self, waveforms: Sequence[SlidingWindowFeature]) -> torch.Tensor:
        """The model half of ``__call__``: what ``finalise`` computes as the overlap track, ``(batch, frames, 1)``
        float32 on the host.  Nothing here depends on ``tau_active``."""
        track = overlap_track(self.segmentation.forward_device(self._windows(waveforms))).float().cpu()
        _range_check(self.config.device)
        return track

    def finalise(self, waveforms: Sequence[SlidingWindowFeature], segmentations: torch.Tensor):
        """The host half of ``__call__`` for given segmentation scores ``(batch, frames, speakers)``: scores on the GPU
        are reduced there (``overlap_track_kernel``), scores on the host by the defining torch statement."""
        if segmentations.shape[-1] < 2:
            raise ValueError(f"OverlappedSpeechDetection: scores of {segmentations.shape[-1]} speaker have no overlap "
                             "track (at least 2 speakers)")
        return self._finalise_track(waveforms, overlap_track(segmentations).cpu())       # (batch, frames, 1)
