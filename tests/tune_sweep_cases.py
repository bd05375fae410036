"""The cases of the sweep's tests (tests/test_tune_sweep_host.py without a GPU, tests/test_gpu_tune_sweep.py on one):
tests/tune_ident_cases.py's caches, gallery and clustering trials, plus a cohort of 12 impostors, two planes
(top_n = 6 and 12) and five signed thresholds: ten (plane, threshold) points per clustering trial.  top_n = 3 of 12 is
avoided: its standard deviations hit the 1e-3 floor (dn down to -302)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_ident_cases as ic  # noqa: E402

TOP_NS = (6, 12)
THRESHOLDS = (-12.0, -6.0, -3.0, -1.0, 0.5)
POINTS = len(TOP_NS) * len(THRESHOLDS)
# the stop cache (a one-chunk file and a chain that stops): three impostors.  With so few, dn is large (the plane of
# top_n = 2 reaches the 1e-3 floor: -588 .. 16; top_n = 3 spans -33 .. 0.7), and a speaker keeps its LOWEST match, so the
# thresholds that change a name lie far down: nobody is named at -600, more and more at -50, -10 and 0.
STOP_TOP_NS = (2, 3)
STOP_THRESHOLDS = (-600.0, -50.0, -10.0, 0.0)


def cohort() -> np.ndarray:
    return np.random.default_rng(2000).standard_normal((12, ic.D)).astype(np.float32)


def stop_cohort() -> np.ndarray:
    return np.random.default_rng(2001).standard_normal((3, ic.D)).astype(np.float32)


def gallery():
    """tune_ident_cases.gallery() with the cohort (its own top_n is the second plane's)."""
    return ic.gallery().with_cohort(cohort(), TOP_NS[1])


def hp3() -> np.ndarray:
    """(16, 3): the clustering rows of tune_ident_cases.trials()."""
    return np.ascontiguousarray(ic.trials()[:, :3])


def normalised_cache(device=None):
    return ic.base_cache().with_gallery(gallery(), device=device, normalised=True, top_n=TOP_NS)


def stop_case():
    """(normalised IdentTuneCache over tune_ident_cases.stop_cache(), its gallery with the cohort, hparams (4, 3))."""
    cache, gal, hp = ic.stop_cache()
    gal = gal.with_cohort(stop_cohort(), STOP_TOP_NS[1])
    return cache.with_gallery(gal, normalised=True, top_n=STOP_TOP_NS), gal, np.ascontiguousarray(hp[:, :3])


def expansion(hp: np.ndarray, thresholds) -> np.ndarray:
    """(T * Q, 4): every clustering row beside every threshold, trial-major."""
    thresholds = np.asarray(thresholds, dtype=np.float64)
    rows = np.repeat(hp, thresholds.shape[0], axis=0)
    return np.ascontiguousarray(np.concatenate([rows, np.tile(thresholds, hp.shape[0])[:, None]], axis=1))


def point_by_point(cache, hp: np.ndarray, thresholds, top_ns, backend: str, **kw):
    """The sweep's definition: (rate (T, P, Q), components (T, P, Q, 5), per_file (T, P, Q, N, 5)) from
    evaluate(hparams (T * Q, 4), top_n=) of every plane."""
    T, Q = hp.shape[0], len(thresholds)
    rate, comp, per_file = [], [], []
    for tn in (top_ns or (None,)):
        r = cache.evaluate(expansion(hp, thresholds), backend=backend, top_n=tn, **kw)
        rate.append(r.rate.reshape(T, Q))
        comp.append(r.components.reshape(T, Q, 5))
        per_file.append(r.per_file.reshape(T, Q, cache.N, 5))
    return np.stack(rate, axis=1), np.stack(comp, axis=1), np.stack(per_file, axis=1)


def python_hold(cache, assign_t: np.ndarray, delta_id: float, plane: int, signed: bool = True) -> np.ndarray:
    """(chunks, G) int32: gallery.SpeakerNames(1, G, delta_id, signed) over every file's chunks in order, on one plane
    of the stored match."""
    from diart_amd.gallery import SpeakerNames
    index, distance = cache.plane_index[plane], cache.plane_distance[plane]
    hold = np.empty((int(cache.chunk_off[-1]), cache.G), dtype=np.int32)
    for n in range(cache.N):
        rule = SpeakerNames(1, cache.G, delta_id, signed=signed)
        for c in range(int(cache.chunk_off[n]), int(cache.chunk_off[n + 1])):
            rule.update(assign_t[c][None], index[c][None], distance[c][None])
            hold[c] = rule.holders()[0]
    return hold


def python_holds(cache, assign: np.ndarray, thresholds, planes) -> np.ndarray:
    """(T, P, Q, chunks, G): python_hold at every (trial, plane, threshold)."""
    return np.stack([np.stack([np.stack([python_hold(cache, assign[t], d, p) for d in thresholds]) for p in planes])
                     for t in range(assign.shape[0])])


def same_sweep(a, b) -> bool:
    """Two SweepResults with the same bits everywhere."""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
