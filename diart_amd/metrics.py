"""Diarization / detection error rates (``pyannote.metrics`` is not installable here).

``DiarizationErrorRate(collar=0, skip_overlap=False)`` is what the reference's pipelines suggest
(``/root/reference/src/diart/blocks/diarization.py:131-133``; ``vad.py:108-110`` for
``DetectionErrorRate``) and what ``Benchmark`` reports (``inference.py:380-389``).  Definition
(NIST md-eval, as pyannote.metrics implements it): with the one-to-one speaker mapping that
maximises the total overlap (Hungarian), over every elementary region with ``Nref`` reference and
``Nhyp`` hypothesis speakers of which ``Ncor`` are correctly mapped,

    miss = max(0, Nref - Nhyp), false alarm = max(0, Nhyp - Nref),
    confusion = min(Nref, Nhyp) - Ncor,   DER = sum(miss + fa + conf) / sum(Nref)   (durations)

No collar, overlapped speech included.  Components accumulate over files like BaseMetric.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from .features import Annotation

COMPONENTS = ("total", "correct", "false alarm", "missed detection", "confusion")


def _turns(ann: Annotation) -> List[Tuple[float, float, object]]:
    return [(seg.start, seg.end, label) for seg, _, label in ann.support().itertracks(yield_label=True)]


def _regions(ref_turns, hyp_turns):
    """Elementary regions between consecutive boundaries -> (duration, ref labels, hyp labels)."""
    bounds = sorted({t for s, e, _ in ref_turns + hyp_turns for t in (s, e)})
    events = []  # (time, +1/-1, side, label)
    for side, turns in ((0, ref_turns), (1, hyp_turns)):
        for s, e, label in turns:
            events.append((s, 1, side, label))
            events.append((e, -1, side, label))
    events.sort(key=lambda ev: (ev[0], ev[1]))
    active = ({}, {})
    k = 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        while k < len(events) and events[k][0] <= lo:
            _, d, side, label = events[k]
            active[side][label] = active[side].get(label, 0) + d
            k += 1
        r = [lab for lab, c in active[0].items() if c > 0]
        h = [lab for lab, c in active[1].items() if c > 0]
        if r or h:
            yield hi - lo, r, h


def optimal_mapping(reference: Annotation, hypothesis: Annotation) -> Dict[object, object]:
    """hypothesis label -> reference label maximising the co-occurrence duration."""
    from ._lsap import linear_sum_assignment
    rl, hl = reference.labels(), hypothesis.labels()
    if not rl or not hl:
        return {}
    cooc = np.zeros((len(hl), len(rl)))
    ri, hi = {l: i for i, l in enumerate(rl)}, {l: i for i, l in enumerate(hl)}
    for dur, r, h in _regions(_turns(reference), _turns(hypothesis)):
        for a in h:
            for b in r:
                cooc[hi[a], ri[b]] += dur
    rows, cols = linear_sum_assignment(-cooc)
    return {hl[i]: rl[j] for i, j in zip(rows, cols) if cooc[i, j] > 0}


class _Accumulating:
    def __init__(self):
        self.accumulated = {c: 0.0 for c in COMPONENTS}
        self.results: List[Tuple[object, Dict[str, float]]] = []

    def _rate(self, comp: Dict[str, float]) -> float:
        err = comp["false alarm"] + comp["missed detection"] + comp["confusion"]
        return err / comp["total"] if comp["total"] > 0 else (0.0 if err == 0 else 1.0)

    def __call__(self, reference: Annotation, hypothesis: Annotation, detailed: bool = False):
        comp = self.components(reference, hypothesis)
        for c in COMPONENTS:
            self.accumulated[c] += comp[c]
        self.results.append((reference.uri, comp))
        rate = self._rate(comp)
        return dict(comp, **{self.name: rate}) if detailed else rate

    def __abs__(self) -> float:
        return self._rate(self.accumulated)

    def reset(self):
        self.__init__()

    def report(self) -> str:
        head = f"{'item':24s} {self.name + ' %':>8s} " + " ".join(f"{c:>17s}" for c in COMPONENTS)
        lines = [head]
        for uri, comp in self.results + [("TOTAL", self.accumulated)]:
            lines.append(f"{str(uri):24s} {100 * self._rate(comp):8.2f} " +
                         " ".join(f"{comp[c]:17.2f}" for c in COMPONENTS))
        return "\n".join(lines)


class DiarizationErrorRate(_Accumulating):
    name = "diarization error rate"

    def __init__(self, collar: float = 0.0, skip_overlap: bool = False):
        if collar != 0.0 or skip_overlap:
            raise NotImplementedError("only collar=0, skip_overlap=False (what diart suggests) is built")
        super().__init__()

    def components(self, reference: Annotation, hypothesis: Annotation) -> Dict[str, float]:
        mapping = optimal_mapping(reference, hypothesis)
        comp = {c: 0.0 for c in COMPONENTS}
        for dur, r, h in _regions(_turns(reference), _turns(hypothesis)):
            nref, nhyp = len(r), len(h)
            ncor = len(set(r) & {mapping.get(a) for a in h})
            comp["total"] += dur * nref
            comp["correct"] += dur * ncor
            comp["missed detection"] += dur * max(0, nref - nhyp)
            comp["false alarm"] += dur * max(0, nhyp - nref)
            comp["confusion"] += dur * (min(nref, nhyp) - ncor)
        return comp


class DetectionErrorRate(_Accumulating):
    name = "detection error rate"

    def __init__(self, collar: float = 0.0, skip_overlap: bool = False):
        if collar != 0.0 or skip_overlap:
            raise NotImplementedError("only collar=0, skip_overlap=False is built")
        super().__init__()

    def components(self, reference: Annotation, hypothesis: Annotation) -> Dict[str, float]:
        comp = {c: 0.0 for c in COMPONENTS}
        for dur, r, h in _regions(_turns(reference), _turns(hypothesis)):
            comp["total"] += dur * bool(r)
            comp["correct"] += dur * (bool(r) and bool(h))
            comp["missed detection"] += dur * (bool(r) and not h)
            comp["false alarm"] += dur * (bool(h) and not r)
        return comp


def overlap_reference(annotation: Annotation) -> Annotation:
    """The overlapped-speech regions of ``annotation`` as an annotation of ``"overlap"`` turns: the support of the
    places where at least two turns with DIFFERENT labels are active.  Two overlapping turns of one label are one
    speaker and no overlap; touching regions are merged; three speakers at once are one region."""
    from .features import Segment
    regions: List[Tuple[float, float]] = []
    for lo, hi, labels in _bounded_regions(_turns(annotation)):
        if len(labels) < 2:
            continue
        if regions and regions[-1][1] == lo:
            regions[-1] = (regions[-1][0], hi)
        else:
            regions.append((lo, hi))
    out = Annotation(uri=annotation.uri)
    for i, (lo, hi) in enumerate(regions):
        out[Segment(lo, hi), i] = "overlap"
    return out


def _bounded_regions(turns):
    """Elementary regions of one annotation's turns -> (start, end, distinct active labels)."""
    bounds = sorted({t for s, e, _ in turns for t in (s, e)})
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        labels = {label for s, e, label in turns if s <= lo and e >= hi}
        if labels:
            yield lo, hi, labels


class OverlapDetectionErrorRate(DetectionErrorRate):
    """``DetectionErrorRate(collar=0, skip_overlap=False)`` of an ``OverlappedSpeechDetection`` hypothesis against the
    reference's OVERLAP regions (``overlap_reference``): the reference is an ordinary speaker annotation, the
    hypothesis holds ``"overlap"`` turns.  ``total`` is the duration of overlapped speech in the reference."""
    name = "overlap detection error rate"

    def components(self, reference: Annotation, hypothesis: Annotation) -> Dict[str, float]:
        return super().components(overlap_reference(reference), hypothesis)


def detection_prf(components) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(precision, recall, F)`` of detection components ``(..., 5)`` in ``COMPONENTS`` order (a dict of them is one
    row), vectorised over the leading axes.  (R) — read from pyannote.metrics' published detection precision, recall
    and F-measure (beta = 1), not run against the package:

        retrieved = correct + false alarm,  relevant = total,
        precision = 1 if retrieved == 0 else correct / retrieved,
        recall    = 1 if relevant == 0 else correct / relevant,
        F         = 0 if precision + recall == 0 else 2 precision recall / (precision + recall).

    Over several files the components are summed first (pyannote accumulates the components, not the rates)."""
    if isinstance(components, dict):
        components = [components[c] for c in COMPONENTS]
    comp = np.asarray(components, dtype=np.float64)
    if comp.shape[-1] != len(COMPONENTS):
        raise ValueError(f"detection_prf: components (..., {len(COMPONENTS)}) expected, got {comp.shape}")
    relevant, correct = comp[..., 0], comp[..., 1]
    retrieved = correct + comp[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = np.where(retrieved == 0, 1.0, correct / retrieved)
        recall = np.where(relevant == 0, 1.0, correct / relevant)
        f = np.where(precision + recall == 0, 0.0, 2.0 * precision * recall / (precision + recall))
    return precision, recall, f


class OverlapDetectionFMeasure(_Accumulating):
    """The detection F-measure of an ``OverlappedSpeechDetection`` hypothesis against the reference's overlap regions
    (``detection_prf`` of ``OverlapDetectionErrorRate``'s components), what pyannote tunes this task on: overlap is
    rare, and a hypothesis without a turn has an error rate of exactly 100 %.  Accumulates the components like
    ``OverlapDetectionErrorRate``; ``abs()`` and ``report()`` give F of the sums — larger is better."""
    name = "overlap detection f-measure"

    def __init__(self, collar: float = 0.0, skip_overlap: bool = False):
        self._rater = OverlapDetectionErrorRate(collar, skip_overlap)
        super().__init__()

    def components(self, reference: Annotation, hypothesis: Annotation) -> Dict[str, float]:
        return self._rater.components(reference, hypothesis)

    def _rate(self, comp: Dict[str, float]) -> float:
        return float(detection_prf(comp)[2])


class IdentificationErrorRate(_Accumulating):
    """The identification error rate: hypothesis labels are NAMES and are compared with the reference labels as they
    are — there is no mapping.  (R) — read from pyannote.metrics' published ``IdentificationErrorRate`` with unit
    weights (confusion, miss and false alarm each count 1), not run against the package, which is not installable
    here.  Over every elementary region with reference labels R and hypothesis labels H:

        total += dur |R|,  correct += dur |R & H|,
        missed detection += dur max(0, |R| - |H|),  false alarm += dur max(0, |H| - |R|),
        confusion += dur (min(|R|, |H|) - |R & H|),   IER = sum(miss + fa + conf) / sum(|R|)

    A reference speaker nobody names can only be missed or confused; a hypothesis label no reference has (an unnamed
    ``speaker3``, say) can only be a false alarm or a confusion.  No collar, overlapped speech included."""
    name = "identification error rate"

    def __init__(self, collar: float = 0.0, skip_overlap: bool = False):
        if collar != 0.0 or skip_overlap:
            raise NotImplementedError("only collar=0, skip_overlap=False is built")
        super().__init__()

    def components(self, reference: Annotation, hypothesis: Annotation) -> Dict[str, float]:
        comp = {c: 0.0 for c in COMPONENTS}
        for dur, r, h in _regions(_turns(reference), _turns(hypothesis)):
            nref, nhyp, both = len(r), len(h), len(set(r) & set(h))
            comp["total"] += dur * nref
            comp["correct"] += dur * both
            comp["missed detection"] += dur * max(0, nref - nhyp)
            comp["false alarm"] += dur * max(0, nhyp - nref)
            comp["confusion"] += dur * (min(nref, nhyp) - both)
        return comp
