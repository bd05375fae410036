"""Cases of the minimum-duration tests (tests/test_min_duration_host.py, tests/test_gpu_min_duration.py): the rule as
a Python loop — the yardstick of every test — and the tuner's files and trials, on tests/hysteresis_cases.py (F = 32,
latency 2.5, files of 9 / 60 / 300 / 520 chunks: at 256 lanes one, one, two and three steps per lane, empty lanes behind)
plus a fifth file of one chunk.  The trials are chosen from the data.  No checkpoint, no model."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hysteresis_cases as hc  # noqa: E402
import tune_vad_cases as vc  # noqa: E402

PATCH_COLLAR = 0.05
TIE_BAR = 1e-9          # no duration or gap lies this close to a trial's value without being equal to it


# ---------------------------------------------------------------------------------------------------- the rule
def support(turns, collar):
    """Annotation.support of one label on (start, end) pairs: a gap is merged when gap <= 1e-6 or gap < collar."""
    out = []
    for s, e in sorted(turns):
        if out:
            gap = s - out[-1][1]
            if gap <= 1e-6 or gap < collar:
                out[-1][1] = max(out[-1][1], e)
                continue
        out.append([s, e])
    return [(s, e) for s, e in out]


def min_duration(turns, on, off, patch_collar=PATCH_COLLAR):
    merged = support(turns, max(patch_collar, off))          # fill the short gaps first ...
    return [(s, e) for s, e in merged if not (e - s < on)]   # ... then drop the short turns (strict <)


def turns_of(annotation):
    return sorted((seg.start, seg.end) for seg, _ in annotation.itertracks())


def annotation_of(turns, uri, label):
    from diart_amd.features import Annotation, Segment
    ann = Annotation(uri=uri)
    for n, (s, e) in enumerate(turns):
        ann[Segment(s, e), n] = label
    return ann


# ---------------------------------------------------------------------------------------------------- files
def one_chunk(kind: str) -> np.ndarray:
    """One chunk: two rises, the second of one frame, a gap of two frames between them."""
    t = np.full((1, hc.F), hc.LOW, dtype=np.float32)
    t[0, 5:19] = hc.HIGH
    t[0, 21] = hc.HIGH
    return t


def files(kind: str):
    return hc.files(kind) + [vc.file_of(one_chunk(kind), shift=-0.5, uri=f"{kind}4")]


def cache(kind: str):
    from diart_amd.optim import OsdTuneCache, VadTuneCache
    return (VadTuneCache if kind == "vad" else OsdTuneCache).from_arrays(files(kind), vc.config_of(hc.LATENCY, hc.ON))


# ---------------------------------------------------------------------------------------------------- trials
def raw_turns(cache_, bits_row, n):
    """File n's turns before any merging, from one trial's masks: per step [middle(onset), middle(first off row))."""
    out = []
    p, m = int(cache_.file_row_off[n]), int(cache_.file_row_off[n] + cache_.chunk_off[n])
    for c in range(int(cache_.chunk_off[n]), int(cache_.chunk_off[n + 1])):
        rows = int(cache_.step_rows[c])
        on = np.concatenate([[False], bits_row[p:p + rows] > 0, [False]])
        edges = np.flatnonzero(on[1:] != on[:-1])
        out += [(float(cache_.mids[m + s]), float(cache_.mids[m + e])) for s, e in zip(edges[::2], edges[1::2])
                if cache_.mids[m + e] - cache_.mids[m + s] > 1e-6]
        p, m = p + rows, m + rows + 1
    return out


def gaps_of(turns):
    """Every gap a merge decision reads: a turn's start minus the running maximum of the ends before it."""
    out, end = [], -np.inf
    for s, e in sorted(turns):
        if np.isfinite(end):
            out.append(s - end)
        end = max(end, e)
    return out


def trials(cache_) -> np.ndarray:
    """(T, 4) = (tau_active, tau_offset, min_duration_on, min_duration_off), from the base pair's own spans and gaps in
    file 2 (300 chunks, two steps per lane): see NAMES."""
    bits = cache_.replay(np.array([[hc.ON, hc.OFF]]), backend="host")[1][0]
    spans = support(raw_turns(cache_, bits, 2), PATCH_COLLAR)
    durations = sorted(e - s for s, e in spans)
    gaps = sorted(g for g in gaps_of(raw_turns(cache_, bits, 2)) if g >= PATCH_COLLAR)
    on_tie, off_tie = durations[len(durations) // 2], gaps[len(gaps) // 2]
    assert on_tie > 0.1 and off_tie > PATCH_COLLAR
    base = [hc.ON, hc.OFF]
    return np.array([base + [0.0, 0.0],
                     base + [on_tie, 0.0],
                     base + [0.0, off_tie],
                     base + [2.0, 0.0],
                     base + [0.0, 1.3],
                     base + [1000.0, 0.0],
                     base + [0.0, 1000.0],
                     [hc.ON, hc.ON, 0.31, 0.27],
                     base + [0.53, 0.41],
                     base + [on_tie, off_tie]])


NAMES = ("base", "min_on = a span's duration (kept)", "min_off = a gap (not merged)", "min_on 2 s", "min_off 1.3 s",
         "min_on above every span", "min_off above the file", "tau_offset == tau_active", "both", "both ties")
ON_TIE, OFF_TIE, NOTHING, ONE_SPAN = 1, 2, 5, 6


def check_trials(cache_, quads, bits):
    """What the trials must be for the tests to show anything, and for independent texts not to disagree by right: no
    span duration and no gap lies within TIE_BAR of a trial's value unless it EQUALS it (equal doubles compare the same
    way in every text); the tie trials have their tie; spans that min_on = 2 s drops and gaps that min_off = 1.3 s
    fills cross lane boundaries (at 256 lanes a lane of files 2 and 3 holds 2 and 3 steps of 0.5 s)."""
    ties = np.zeros((len(quads), 2), dtype=int)
    for t, (_, _, on, off) in enumerate(quads):
        for n in range(cache_.N):
            turns = raw_turns(cache_, bits[t], n)
            for g in gaps_of(turns):
                assert g == off or abs(g - off) > TIE_BAR, (t, n, g)
                ties[t, 1] += g == off
            for s, e in support(turns, max(PATCH_COLLAR, off)):
                assert (e - s) == on or abs((e - s) - on) > TIE_BAR, (t, n, s, e)
                ties[t, 0] += (e - s) == on
    assert ties[ON_TIE, 0] >= 1 and ties[OFF_TIE, 1] >= 1, ties
    for n, per in ((2, 2), (3, 3)):
        c0, c1 = int(cache_.chunk_off[n]), int(cache_.chunk_off[n + 1])
        assert -(-(c1 - c0) // 256) == per
        first = cache_.mids[cache_.row_off[c0:c1] + np.arange(c0, c1)]              # every step's first frame middle
        lane_of = lambda x: (int(np.searchsorted(first, x, side="right")) - 1) // per
        turns = raw_turns(cache_, bits[3], n)
        dropped = [(s, e) for s, e in support(turns, PATCH_COLLAR) if e - s < 2.0]
        assert sum(lane_of(s) != lane_of(e - 1e-3) for s, e in dropped) >= 2, n
        merged = support(turns, 1.3)
        assert len(merged) < len(support(turns, PATCH_COLLAR)), n
        assert any(lane_of(e - 1e-3) - lane_of(s) > 3 for s, e in merged), n
    for n in range(cache_.N):
        assert not min_duration(raw_turns(cache_, bits[NOTHING], n), quads[NOTHING][2], quads[NOTHING][3])
        assert len(min_duration(raw_turns(cache_, bits[ONE_SPAN], n), quads[ONE_SPAN][2], quads[ONE_SPAN][3])) <= 1
