"""Synthetic caches for the VoiceActivityDetection tuner's tests (tests/test_tune_vad_host.py,
tests/test_gpu_tune_vad.py): tracks drawn by tests/tune_cases.py (the max over its local speakers) or made by hand,
window starts and references as that module makes them.  No checkpoint, no model."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402


def track_of(seed: int, chunks: int, F: int) -> np.ndarray:
    return np.ascontiguousarray(tc.random_outputs(seed, chunks, F, 3, 2)[0].max(axis=2))


def file_of(track, shift: float = 0.0, uri: str = "file", reference=None) -> dict:
    C, F = track.shape
    return dict(uri=uri, track=track, starts=tc.starts_for(C), res=tc.DURATION / F, shift=shift,
                reference=tc.reference_for(C, shift) if reference is None else reference)


def config_of(latency: float, tau: float = 0.6) -> dict:
    return dict(step=tc.STEP, latency=latency, tau_active=tau)


def taus_of(count: int, seed: int = 0) -> np.ndarray:
    """Uniform draws of tau in [0, 1] plus tau = 0.0 and tau = 1.0 (one trial: one draw)."""
    rng = np.random.default_rng(seed)
    if count < 3:
        return rng.uniform(0.0, 1.0, size=count)
    return np.concatenate([rng.uniform(0.0, 1.0, size=count - 2), [0.0, 1.0]])


def cache_of(files, latency):
    from diart_amd.optim import VadTuneCache
    return VadTuneCache.from_arrays(files, config_of(latency))


# name -> (F, latency, trials): a file of one chunk beside one of 61 with shift -1.25.  F = 16 at latency = step (one
# buffer per step: only the first chunk's prepend and the plain rows), 2.5 and 5.0; one frame per chunk; one trial, 67.
EDGES = {
    "lat_step": (16, 0.5, 33),
    "lat_mid": (16, 2.5, 33),
    "lat_max": (16, 5.0, 33),
    "F1": (1, 2.5, 33),
    "T1": (16, 5.0, 1),
    "T67": (16, 2.5, 67),
}


# (F1's seed: the first of 0..7 whose 61-chunk file has false alarm and missed detection in at least half of the trials
# — with one frame per chunk most draws of tau leave a file all speech or all silence)
EDGE_SEEDS = {"lat_step": 5, "lat_mid": 4, "lat_max": 3, "F1": 7, "T1": 1, "T67": 2}


def edge_cache(name):
    F, latency, T = EDGES[name]
    seed = EDGE_SEEDS[name]
    files = [file_of(track_of(100 + seed, 1, F), uri="one"),
             file_of(track_of(200 + seed, 61, F), shift=-1.25, uri="sixty-one")]
    return cache_of(files, latency), taus_of(T, seed)


COLLAR_LEVELS = (0.9, 0.1)          # speech / no speech of the hand-made track; the collar trials include tau = 0.5


def collar_runs(cache):
    """(first packed row, frames) of the inactive runs of the hand-made track: 1, 2, 3 and 4 frames inside a step
    (in the first step, whose rows are 5 / 293 s: 2 frames are 0.034 s, 3 are 0.051 s; behind it 3 frames are 0.05 s up
    to the last bits), 2, 3 and 4 frames that straddle a step's end, 2 and 3 frames that end exactly at a step's last
    row."""
    ro = cache.row_off
    return ((20, 2), (40, 1), (70, 4), (100, 3), (int(ro[4]) + 10, 3), (int(ro[3]) - 1, 3), (int(ro[5]) - 2, 3), (int(ro[6]) - 1, 2),
            (int(ro[7]) - 3, 4), (int(ro[8]) - 2, 2), (int(ro[9]) - 3, 3), (int(ro[10]) + 3, 1))


def collar_cache():
    """12 chunks of 293 frames at latency = step: 30 output rows of 1 / 60 s per step, each the score of one frame of
    its step's chunk (one buffer), so the track is set row by row: speech from packed row 5 to the end of chunk 10's
    step, with collar_runs() cut out.  2 frames of silence (0.033 s) are patched, 4 (0.067 s) are not, 3 sit on
    0.05 s up to the last bits.  Returns (cache, the rows that are speech at tau = 0.5)."""
    chunks, F = 12, 293
    blank = cache_of([file_of(np.zeros((chunks, F), dtype=np.float32), shift=-0.3, uri="collar")], 0.5)
    assert (blank.step_rows[1:] == 30).all() and (blank.plan[:, 3] == 1).all()
    on = np.zeros(blank.total_rows, dtype=bool)
    on[5:int(blank.row_off[11])] = True
    for start, frames in collar_runs(blank):
        on[start:start + frames] = False
    track = np.full((chunks, F), COLLAR_LEVELS[1], dtype=np.float32)
    for p in range(blank.total_rows):
        c = int(blank.row_chunk[p])
        r, plan = p - int(blank.row_off[c]), blank.plan[c]
        frame = min(max(plan[2] + r if r < plan[1] else plan[4] + (r - plan[1]), 0), F - 1)      # (cropped rows are clipped)
        if on[p]:
            track[c, frame] = COLLAR_LEVELS[0]
    return cache_of([file_of(track, shift=-0.3, uri="collar")], 0.5), on


def carry_cache():
    """300 chunks at F = 16 whose chunks 40 to 250 are all zero (at 256 lanes a lane owns two steps: the end of the
    last turn before the silence is carried across a hundred lanes that have no turn), beside a file of 3 chunks,
    fewer than the 10 buffers of latency 5.0."""
    track = track_of(300, 300, 16)
    track[40:251] = 0
    return cache_of([file_of(track, uri="three-hundred"), file_of(track_of(301, 3, 16), shift=-0.75, uri="three")], 5.0)


def degenerate_cache():
    """A file whose track is all zero, a file with an empty reference, a file with a chunk of NaN."""
    nan = track_of(402, 20, 16)
    nan[7] = np.nan
    return cache_of([file_of(np.zeros((20, 16), dtype=np.float32), uri="silent"),
                     file_of(track_of(401, 20, 16), shift=-1.25, uri="no-reference", reference=[]),
                     file_of(nan, uri="nan")], 2.5)
