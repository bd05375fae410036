"""Pipeline / PipelineConfig interfaces and tunable hyper-parameters (reference:
``/root/reference/src/diart/blocks/base.py:12-137``) — what ``StreamingInference``,
``Benchmark`` and ``Optimizer`` rely on."""
from __future__ import annotations

from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Any, Sequence, Tuple

from ..features import SlidingWindowFeature


@dataclass
class HyperParameter:
    name: str
    low: float
    high: float

    @staticmethod
    def from_name(name: str) -> "HyperParameter":
        for hp in (TauActive, RhoUpdate, DeltaNew, DeltaId, TauOffset, MinDurationOn, MinDurationOff):
            if hp.name == name:
                return hp
        raise ValueError(f"Hyper-parameter '{name}' not recognized")


TauActive = HyperParameter("tau_active", low=0, high=1)
RhoUpdate = HyperParameter("rho_update", low=0, high=1)
DeltaNew = HyperParameter("delta_new", low=0, high=2)
# the identification distance of a speaker gallery (optim.IdentTuneCache): the cosine distance's range, as delta_new
DeltaId = HyperParameter("delta_id", low=0, high=2)
# the offset threshold of the track pipelines' hysteresis (VoiceActivityDetection, OverlappedSpeechDetection)
TauOffset = HyperParameter("tau_offset", 0, 1)
# the minimum durations of the track pipelines, where a whole file is known (file batches, the accumulated prediction, the
# tuner): gaps shorter than min_duration_off are filled, then turns shorter than min_duration_on are dropped.  The range
# is pyannote's Uniform(0, 1) for both, in seconds
MinDurationOn = HyperParameter("min_duration_on", 0, 1)
MinDurationOff = HyperParameter("min_duration_off", 0, 1)


def check_tau_offset(value, who: str):
    """``None`` (no hysteresis: the offset is ``tau_active``) or the finite float of ``value``; anything else is a
    ``ValueError`` that names ``who``."""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: tau_offset must be a finite number or None, got {value!r}") from None
    if isinstance(value, bool) or v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: tau_offset must be a finite number or None, got {value!r}")
    return v


def check_min_duration(value, name: str, who: str) -> float:
    """The finite float >= 0 of ``value`` (``name``: min_duration_on | min_duration_off, in seconds); anything else is a
    ``ValueError`` that names ``who``."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {value!r}") from None
    if isinstance(value, bool) or not (0.0 <= v < float("inf")):
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {value!r}")
    return v


def refuse_min_duration(kwargs: dict, who: str) -> None:
    """``SpeakerDiarization`` and everything that serves it take no minimum duration (they would be per speaker): a
    ``ValueError`` if ``kwargs`` names one."""
    for name in ("min_duration_on", "min_duration_off"):
        if name in kwargs:
            raise ValueError(f"{who}: {name} is not a parameter of SpeakerDiarization; the minimum durations are "
                             "VoiceActivityDetection's and OverlappedSpeechDetection's, where a whole file is known")


class PipelineConfig(ABC):
    @property
    @abstractmethod
    def duration(self) -> float: ...

    @property
    @abstractmethod
    def step(self) -> float: ...

    @property
    @abstractmethod
    def latency(self) -> float: ...

    @property
    @abstractmethod
    def sample_rate(self) -> int: ...

    def get_padding(self, stream_duration: float) -> Tuple[float, float]:
        """(left, right) zero padding in seconds for a stream of this length — the arithmetic of
        ``get_file_padding`` (base.py:81-85, utils.py:69-88) without the audio-file probe."""
        right = self.latency - self.step
        total = stream_duration + right
        left = self.duration - total if total < self.duration else 0
        return left, right

    def get_file_padding(self, filepath) -> Tuple[float, float]:
        """The reference's entry point (``blocks/base.py:81-85`` -> ``utils.get_padding_left/right``):
        padding for an audio FILE; the duration comes from the WAV header."""
        from ..inference import wav_duration
        return self.get_padding(wav_duration(filepath))


class Pipeline(ABC):
    @staticmethod
    @abstractmethod
    def get_config_class() -> type: ...

    @staticmethod
    @abstractmethod
    def suggest_metric(): ...

    @staticmethod
    @abstractmethod
    def hyper_parameters() -> Sequence[HyperParameter]: ...

    @property
    @abstractmethod
    def config(self) -> PipelineConfig: ...

    @abstractmethod
    def reset(self): ...

    @abstractmethod
    def set_timestamp_shift(self, shift: float): ...

    @abstractmethod
    def __call__(self, waveforms: Sequence[SlidingWindowFeature]) -> Sequence[Tuple[Any, SlidingWindowFeature]]: ...
