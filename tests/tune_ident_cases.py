"""Caches, galleries and trials for the delta_id tuner's tests (tests/test_tune_ident_host.py without a GPU,
tests/test_gpu_tune_ident.py on one).  The model outputs are tests/tune_cases.py's generators at D = 64 (the gallery's
smallest dimension); the yardstick of the names is gallery.SpeakerNames in Python, of the score
metrics.IdentificationErrorRate on IdentTuneCache.hypothesis."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402

F, K, D, G, LATENCY, CHUNKS = 16, 3, 64, 5, 2.5, 40
SEEDS = (11, 12, 13)                      # one per file
SHIFTS = (0.0, -1.25, -0.5)
OWN = (0.5, 0.3, 1.0)
NAMES = ("ref0", "ref1", "ref7", "dave", "zed", "far")


def outputs(seed: int):
    return tc.random_outputs(seed, CHUNKS, F, K, D)


def pool(seed: int) -> np.ndarray:
    """The generator's pool of voices: the first draw of the same seed."""
    return np.random.default_rng(seed).standard_normal((6, D))


def busiest(seed: int) -> np.ndarray:
    """The pool's voices by how many embedding rows of the seed's file are nearest to them, busiest first."""
    emb = outputs(seed)[1].reshape(-1, D)
    emb = emb[~np.isnan(emb).any(axis=1)]
    v = pool(seed)
    near = np.argmax(emb @ (v / np.linalg.norm(v, axis=1, keepdims=True)).T, axis=1)
    return v[np.argsort(-np.bincount(near, minlength=6), kind="stable")]


def gallery_rows() -> np.ndarray:
    """Six voiceprints.  Four near pool voices: "ref0" and "ref1" near-duplicates of file 0's busiest voice, "ref7" (a
    label no reference has) near file 1's, "dave" near file 2's.  "zed" lies half way between two voices of file 0,
    "far" is the negative of the mean of all voices."""
    rng = np.random.default_rng(1000)
    v0, v1, v2 = (busiest(s) for s in SEEDS)
    rows = [v0[0] + 0.05 * rng.standard_normal(D), v0[0] + 0.05 * rng.standard_normal(D),
            v1[0] + 0.1 * rng.standard_normal(D), v2[0] + 0.1 * rng.standard_normal(D),
            v0[1] + v0[2], -np.concatenate([v0, v1, v2]).mean(axis=0)]
    return np.stack(rows).astype(np.float32)


def gallery():
    from diart_amd.gallery import SpeakerGallery
    return SpeakerGallery(list(NAMES), gallery_rows())


def base_cache():
    """Three files of 40 chunks, tune_cases.random_outputs(seed, 40, F, K=3, D=64), shifts as tests/tune_cases.py's."""
    from diart_amd.optim import TuneCache
    files = [tc.file_of(*outputs(seed), shift=shift, uri=f"file{i}") for i, (seed, shift) in enumerate(zip(SEEDS, SHIFTS))]
    return TuneCache.from_arrays(files, tc.config_of(*OWN, G, LATENCY))


def trials() -> np.ndarray:
    """(16, 4): tune_cases.neighbours' eight and eight of random_trials' draws for the clustering, delta_id over
    {0, 0.2, 0.5, 1.0, 2.0} and six uniform draws from its range."""
    hp3 = np.concatenate([tc.neighbours(*OWN), tc.random_trials(OWN, 9, seed=4)[1:]])
    rng = np.random.default_rng(77)
    delta = np.concatenate([[0.0, 0.2, 0.5, 1.0, 2.0, 0.2, 0.5, 1.0, 0.0, 0.5], rng.uniform(0.0, 2.0, size=6)])
    return np.ascontiguousarray(np.concatenate([hp3, delta[:, None]], axis=1))


def stop_cache():
    """(TuneCache, gallery, hparams (4, 4)): one chunk beside tune_cases.failing_step_inputs padded with zeros to
    D = 64 (zeros change no dot product), whose chain stops at its chunk 3 under the first trial."""
    from diart_amd.gallery import SpeakerGallery
    from diart_amd.optim import TuneCache
    k, g, seg, emb = tc.failing_step_inputs(tc.RAISES_SEED)
    wide = np.zeros(emb.shape[:2] + (D,), dtype=np.float32)
    wide[:, :, :emb.shape[2]] = emb
    seg1, emb1 = tc.random_outputs(301, 1, seg.shape[1], k, D)
    files = [tc.file_of(seg1, emb1, shift=0.0, uri="one"), tc.file_of(seg, wide, shift=-1.25, uri="six")]
    cache = TuneCache.from_arrays(files, tc.config_of(*tc.RAISES_OWN, g, 2.5))
    rows = np.stack([wide[0, 0], wide[2, 1] + 0.1 * wide[0, 1], emb1[0, 0]]).astype(np.float32)
    gal = SpeakerGallery(["ref0", "ref1", "erin"], rows)
    hp3 = tc.random_trials(tc.RAISES_OWN, 4, seed=5)
    hp = np.concatenate([hp3, np.array([[0.5], [1.0], [0.3], [2.0]])], axis=1)
    return cache, gal, np.ascontiguousarray(hp)


def python_hold(cache, assign_t: np.ndarray, delta_id: float) -> np.ndarray:
    """(chunks, G) int32: gallery.SpeakerNames(1, G, delta_id) over every file's chunks in order (definition 1)."""
    from diart_amd.gallery import SpeakerNames
    hold = np.empty((int(cache.chunk_off[-1]), cache.G), dtype=np.int32)
    for n in range(cache.N):
        rule = SpeakerNames(1, cache.G, delta_id)
        for c in range(int(cache.chunk_off[n]), int(cache.chunk_off[n + 1])):
            rule.update(assign_t[c][None], cache.match_index[c][None], cache.match_distance[c][None])
            hold[c] = rule.holders()[0]
    return hold


def reference_of(cache, n: int):
    from diart_amd.features import Annotation, Segment
    ref = Annotation(uri=cache.files[n]["uri"])
    for i, (s, e, label) in enumerate(cache.files[n]["turns"]):
        ref[Segment(s, e), i] = label
    return ref


def metric_components(cache, bits, hold) -> np.ndarray:
    """(T, N, 5): metrics.IdentificationErrorRate on (reference, cache.hypothesis(...)) (definitions 2 and 3)."""
    from diart_amd.metrics import COMPONENTS, IdentificationErrorRate
    out = np.zeros((bits.shape[0], cache.N, 5))
    for n in range(cache.N):
        ref = reference_of(cache, n)
        for t in range(bits.shape[0]):
            comp = IdentificationErrorRate().components(ref, cache.hypothesis(bits[t], hold[t], n))
            out[t, n] = [comp[c] for c in COMPONENTS]
    return out


def bars(per_file: np.ndarray) -> np.ndarray:
    """1e-9 x the pair's total, per component: the tolerance the tuners use between their backends (the sides differ in
    the order in which the durations are summed)."""
    return 1e-9 * per_file[..., :1]
