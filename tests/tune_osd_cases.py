"""Synthetic caches for the OverlappedSpeechDetection tuner's tests (tests/test_tune_osd_host.py,
tests/test_gpu_tune_osd.py): the shapes of tests/tune_vad_cases.py behind the other track (the second largest over the
local speakers of tests/tune_cases.py's draws) and speaker references, whose overlap regions are what is scored.  No
checkpoint, no model."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_vad_cases as vc  # noqa: E402

EDGES = vc.EDGES
taus_of = vc.taus_of
config_of = vc.config_of


def track_of(seed: int, chunks: int, F: int) -> np.ndarray:
    return np.ascontiguousarray(np.sort(tc.random_outputs(seed, chunks, F, 3, 2)[0], axis=2)[:, :, -2])


def file_of(track, shift: float = 0.0, uri: str = "file", reference=None) -> dict:
    """tc.reference_for's three speakers overlap by construction (a turn of speaker s starts 0.37 s behind one of
    speaker s - 1 at the start of the file, and the periods differ)."""
    return vc.file_of(track, shift, uri, reference)


def cache_of(files, latency):
    from diart_amd.optim import OsdTuneCache
    return OsdTuneCache.from_arrays(files, config_of(latency, 0.5))


# per case a seed of 0..7, no two cases the same, whose 61-chunk file has false alarm and missed detection in at least
# half of the trials and a positive overlap total (the tests assert both; seed 4 fails that at latency 5.0, and with one
# frame per chunk so do seeds 1 and 7)
EDGE_SEEDS = {"lat_step": 0, "lat_mid": 2, "lat_max": 3, "F1": 6, "T1": 1, "T67": 5}


def edge_files(name, seed=None):
    F, latency, T = EDGES[name]
    seed = EDGE_SEEDS[name] if seed is None else seed
    files = [file_of(track_of(100 + seed, 1, F), uri="one"),
             file_of(track_of(200 + seed, 61, F), shift=-1.25, uri="sixty-one")]
    return files, latency, taus_of(T, seed)


def edge_cache(name, seed=None):
    files, latency, taus = edge_files(name, seed)
    return cache_of(files, latency), taus


CARRY_TAUS = (33, 8)


def carry_cache():
    """vc.carry_cache's shape: 300 chunks at F = 16 whose chunks 40 to 250 are all zero (211 silent chunks: the end of
    the last turn before them is carried across a hundred lanes without a turn), beside a file of 3 chunks."""
    track = track_of(300, 300, 16)
    track[40:251] = 0
    return cache_of([file_of(track, uri="three-hundred"), file_of(track_of(301, 3, 16), shift=-0.75, uri="three")], 5.0)


NO_OVERLAP = [(0.4, 3.1, "a"), (3.1, 6.0, "b"), (7.2, 9.9, "a"), (8.0, 9.0, "a")]


def degenerate_cache():
    """A file whose track is all zero, a file whose reference has speech and no overlap (total = 0), a file with a chunk
    of NaN."""
    nan = track_of(402, 20, 16)
    nan[7] = np.nan
    return cache_of([file_of(np.zeros((20, 16), dtype=np.float32), uri="silent"),
                     file_of(track_of(401, 20, 16), shift=-1.25, uri="no-overlap", reference=NO_OVERLAP),
                     file_of(nan, uri="nan")], 2.5)


# crafted references over a file of 20 chunks (14.5 s), times off the frame grid
CRAFTED = {
    "two_partly": [(1.03, 5.21, "a"), (3.17, 8.4, "b")],
    "one_label_twice": [(1.03, 5.21, "a"), (3.17, 8.4, "a")],                      # one speaker: no overlap
    "three_at_once": [(1.03, 6.3, "a"), (2.11, 7.7, "b"), (3.17, 5.05, "c"), (9.0, 11.0, "a")],
    "regions_touch": [(1.03, 4.0, "a"), (2.11, 3.0, "b"), (3.0, 4.0, "c")],         # (a, b) up to 3.0, (a, c) from 3.0
    "no_overlap": [(1.03, 2.0, "a"), (3.17, 4.0, "b"), (4.0, 5.5, "a")],
    "empty": [],
}
# the overlap regions the docstring of metrics.overlap_reference promises for them
CRAFTED_REGIONS = {
    "two_partly": [(3.17, 5.21)],
    "one_label_twice": [],
    "three_at_once": [(2.11, 6.3)],
    "regions_touch": [(2.11, 4.0)],
    "no_overlap": [],
    "empty": [],
}
