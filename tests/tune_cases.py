"""Synthetic caches for the hyper-parameter tuner's tests (tests/test_tune_host.py, tests/test_gpu_tune.py): model
outputs from tests/golden/scenarios.py or drawn here, window starts as the file loop counts them (repeated addition of
the step), a made-up reference.  No checkpoint, no model."""
import sys
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLD))
import scenarios  # noqa: E402

STEP, DURATION = 0.5, 5.0
RANGES = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 2.0]])      # tau_active, rho_update, delta_new (blocks/base.py)


def starts_for(chunks: int, first: float = 0.0) -> np.ndarray:
    out, t = [], first
    for _ in range(chunks):
        out.append(t)
        t += STEP
    return np.array(out, dtype=np.float64)


def reference_for(chunks: int, shift: float = 0.0, speakers: int = 3):
    """Overlapping turns of `speakers` reference speakers over the file's time span (times off the frame grid)."""
    end = DURATION + STEP * (chunks - 1) + shift
    turns = []
    for s in range(speakers):
        t = 0.37 * s
        while t < end:
            turns.append((t, min(end, t + 2.9 + 0.61 * s), f"ref{s}"))
            t += 4.3 + 0.83 * s
    return turns


def file_of(seg, emb, shift: float = 0.0, uri: str = "file", ref_speakers: int = 3) -> dict:
    C, F = seg.shape[0], seg.shape[1]
    return dict(uri=uri, seg=seg, emb=emb, starts=starts_for(C), res=DURATION / F, shift=shift,
                reference=reference_for(C, shift, ref_speakers))


def config_of(tau, rho, delta, G, latency) -> dict:
    return dict(step=STEP, latency=latency, tau_active=tau, rho_update=rho, delta_new=delta, max_speakers=int(G))


def random_outputs(seed: int, chunks: int, F: int, K: int, D: int, pool: int = 6):
    """Activity that persists over a few chunks (so the aggregation has something to average), voices from a small
    pool, with NaN embeddings, duplicated rows and silent chunks mixed in."""
    rng = np.random.default_rng(seed)
    voices = rng.standard_normal((pool, D))
    seg = np.zeros((chunks, F, K), dtype=np.float32)
    emb = np.zeros((chunks, K, D), dtype=np.float32)
    who = rng.choice(pool, size=K, replace=pool < K)
    level = rng.random(K)
    for c in range(chunks):
        if rng.random() < 0.3:
            k = rng.integers(K)
            who[k], level[k] = rng.integers(pool), rng.random()
        seg[c] = np.clip(level * (rng.random((F, K)) < 0.3 + 0.7 * level) + 0.05 * rng.random((F, K)), 0, 1)
        e = voices[who] + 0.3 * rng.standard_normal((K, D))
        emb[c] = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-3)
        r = rng.random()
        if r < 0.06:
            emb[c, rng.integers(K)] = np.nan
        elif r < 0.12 and K > 1:
            emb[c, 1] = emb[c, 0]
        elif r < 0.16:
            seg[c] = 0
    return seg, emb


def neighbours(tau, rho, delta) -> np.ndarray:
    """A trial's own parameters and seven neighbours."""
    base = np.array([tau, rho, delta], dtype=np.float64)
    out = [base]
    for i in range(3):
        for sign in (-1.0, 1.0):
            p = base.copy()
            p[i] = np.clip(p[i] + sign * 0.05, RANGES[i, 0], RANGES[i, 1])
            out.append(p)
    out.append(np.clip(base + [0.03, -0.04, 0.06], RANGES[:, 0], RANGES[:, 1]))
    return np.array(out)


def random_trials(own, count: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    draws = rng.uniform(RANGES[:, 0], RANGES[:, 1], size=(count - 1, 3))
    return np.concatenate([np.array([own], dtype=np.float64), draws])


def long_random(seed, K, D, G, steps: int = 300):
    seg, emb = [], []
    for t, (s, e) in enumerate(scenarios.clustering_long_random_inputs(seed, K, D, G)):
        if t == steps:
            break
        seg.append(s)
        emb.append(e)
    return np.stack(seg), np.stack(emb)


def failing_step_inputs(seed: int):
    """Six steps of a short stream with more local than global speakers (K 5..8, G 3..4; D 8, 12 frames), two of them
    at most active in the first: (K, G, seg, emb).  Under tau 0.55, rho 0.25 and a delta_new that unmaps nobody (1e11)
    most seeds reach a step at which the reference raises "Cannot update unknown centers", many of them after that
    step has updated a centroid (tests/test_clustering.py test_state_after_a_failing_step_is_the_oracles)."""
    rng = np.random.default_rng(1000 + seed)
    K, G, D, F = int(rng.integers(5, 9)), int(rng.integers(3, 5)), 8, 12
    seg = np.zeros((6, F, K), dtype=np.float32)
    emb = np.zeros((6, K, D), dtype=np.float32)
    for t in range(6):
        seg[t] = rng.random((F, K)) * (rng.random(K) < 0.5) * rng.choice([0.3, 0.8, 1.0], K)
        emb[t] = rng.standard_normal((K, D))
        if t == 0:
            seg[t, :, 0] = 0.9
            seg[t, :, 2:] = 0
    return K, G, seg, emb


# name -> (F, K, D, G, latency, trials): D = 1 and 15 (dot2's odd tail), one local / one global speaker, one frame,
# one trial and 67, fewer centroids than local speakers with more than one of them (1 < G < K: the transposed
# assignment problem whose pairs have to be sorted by row, and `valid` enumerating a column list shorter than K; K = 8
# is the capacity of the fixed arrays); every case is a file of one chunk beside one of 61.  "raises": beside the one
# chunk, failing_step_inputs(RAISES_SEED), whose chunk 3 makes dz_clu_step return non-zero ("Cannot update unknown
# centers") under the first trial, after it has decided a centroid update; the other trials are uniform draws
EDGES = {
    "D1": (16, 3, 1, 4, 2.5, 67),
    "D15": (16, 3, 15, 4, 0.5, 67),
    "K1": (16, 1, 8, 4, 5.0, 67),
    "G1": (16, 3, 8, 1, 2.5, 67),
    "F1": (1, 3, 8, 4, 2.5, 67),
    "T1": (16, 3, 8, 4, 5.0, 1),
    "K4G3": (16, 4, 8, 3, 2.5, 33),
    "K8G5": (16, 8, 12, 5, 2.5, 33),
    "lat_step": (32, 4, 24, 20, 0.5, 9),
    "lat_mid": (32, 4, 24, 20, 2.5, 9),
    "lat_max": (32, 4, 24, 20, 5.0, 9),
    "raises": (12, 8, 8, 4, 2.5, 9),
}
RAISES_SEED, RAISES_OWN = 17, (0.55, 0.25, 1e11)

EDGE_SEEDS = sorted(n for n in EDGES if n not in ("K4G3", "K8G5", "raises")) + ["K4G3", "K8G5", "raises"]


def edge_cache(name):
    from diart_amd.optim import TuneCache
    F, K, D, G, latency, T = EDGES[name]
    seed = EDGE_SEEDS.index(name)
    own = RAISES_OWN if name == "raises" else (0.5, 0.3, 1.0)
    if name == "raises":
        assert failing_step_inputs(RAISES_SEED)[:2] == (K, G)
        second = file_of(*failing_step_inputs(RAISES_SEED)[2:], shift=-1.25, uri="six")
    else:
        second = file_of(*random_outputs(200 + seed, 61, F, K, D), shift=-1.25, uri="sixty-one")
    files = [file_of(*random_outputs(100 + seed, 1, F, K, D), shift=0.0, uri="one"), second]
    cache = TuneCache.from_arrays(files, config_of(*own, G, latency))
    return cache, random_trials(own, T, seed=seed) if T > 1 else np.array([own])
