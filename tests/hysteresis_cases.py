"""Cases of the hysteresis tests (tests/test_hysteresis_host.py, tests/test_gpu_hysteresis.py): the rule as a Python
loop — the yardstick of every test — and hand-made tracks for the tuner, on the helpers of tests/tune_vad_cases.py and
tests/tune_cases.py.  No checkpoint, no model."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_osd_cases as oc  # noqa: E402
import tune_vad_cases as vc  # noqa: E402

F = 32
LATENCY = 2.5
ON, OFF = 0.6, 0.4                 # the base pair
HIGH, BAND, LOW = 0.9, 0.5, 0.1    # above tau_active, inside the band, below tau_offset
CHUNKS = (9, 60, 300, 520)         # at 256 lanes: one, one, two and three steps per lane, empty lanes behind the last


def hysteresis(rows, tau_active, tau_offset, active=False):
    """The rule: ``rows`` are the aggregated scores of one step of one track, in order."""
    on = np.empty(len(rows), bool)
    for r, y in enumerate(rows):                       # float64, plain compares
        active = bool(y > (tau_offset if active else tau_active))
        on[r] = active
    return on, active        # `active` enters the same stream's NEXT step


def turns_of(on, t0, res, speaker=0):
    """Binarize's turns of one step from its rows' ``on``: [middle(first on row), middle(first off row after it)), the
    row after the last closing an open turn; the middles as csrc/tail.cpp and SlidingWindow form them."""
    def middle(i):
        s = t0 + i * res
        return 0.5 * (s + (s + res))
    out, onset = [], -1
    for r in range(len(on) + 1):
        active = r < len(on) and bool(on[r])
        if active and onset < 0:
            onset = r
        if not active and onset >= 0:
            out.append((middle(onset), middle(r), float(speaker)))
            onset = -1
    return out


def tracks(kind: str):
    """The four files' tracks (chunks, F) float32.  ``kind``: "vad" | "osd" — which helper draws the random parts."""
    draw = vc.track_of if kind == "vad" else oc.track_of
    a = draw(11, CHUNKS[0], F)
    # begins inside the band and stays off; ordinary activity behind it
    b = draw(12, CHUNKS[1], F)
    b[:30] = BAND
    # a held turn with a NaN step inside it: on at chunks 10..14, band up to chunk 139 — the NaN of chunk 70 switches
    # the track off, and the band behind it leaves it off — then low, then ordinary activity
    c = draw(13, CHUNKS[2], F)
    c[:10], c[10:15], c[15:140], c[140:160] = LOW, HIGH, BAND, LOW
    c[70] = np.nan
    # one rise above tau_active (five chunks: the buffers of a step), 290 steps inside the band (some hundred lanes of three steps), then low
    d = draw(14, CHUNKS[3], F)
    d[100:110], d[110:115], d[115:405], d[405:415] = LOW, HIGH, BAND, LOW
    return [np.ascontiguousarray(t, dtype=np.float32) for t in (a, b, c, d)]


def files(kind: str):
    shifts = (0.0, -1.75, 0.0, -0.25)
    return [vc.file_of(t, shift=s, uri=f"{kind}{n}") for n, (t, s) in enumerate(zip(tracks(kind), shifts))]


def cache(kind: str):
    from diart_amd.optim import OsdTuneCache, VadTuneCache
    return (VadTuneCache if kind == "vad" else OsdTuneCache).from_arrays(files(kind), vc.config_of(LATENCY, ON))


def trials(agg) -> np.ndarray:
    """(T, 2): the base pair; a pair of thresholds that both equal an aggregated score that occurs (`>` meets it); offset
    == onset; offset > onset; an offset far below every score.  The first two are the band trials."""
    finite = agg[np.isfinite(agg)]
    tie_on = float(np.sort(finite[(finite > 0.55) & (finite < 0.8)])[3])
    tie_off = float(np.sort(finite[(finite > 0.2) & (finite < 0.45)])[3])
    return np.array([[ON, OFF], [tie_on, tie_off], [ON, ON], [OFF, ON], [ON, -5.0]])


BAND_TRIALS = (0, 1)


def loop_bits(cache_, agg, pair) -> np.ndarray:
    """The masks of one trial by the rule, file by file (the state off at every file's first row)."""
    out = np.zeros(cache_.total_rows, dtype=np.uint32)
    for n in range(cache_.N):
        a, b = int(cache_.file_row_off[n]), int(cache_.file_row_off[n + 1])
        out[a:b] = hysteresis(agg[a:b], pair[0], pair[1])[0]
    return out
