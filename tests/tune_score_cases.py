"""Hand-made masks for the tuner's device scoring (tests/test_tune_score_core.py without a GPU,
tests/test_gpu_tune_score.py on one): caches of silent model outputs whose only purpose is their output grid (293 frames
per chunk: 30 output rows per 0.5 s step, as tests/test_tune_host.py's _masks_cache), a made-up reference, and packed
masks written row by row.  Every case is `(cache, bits (T, rows) uint32)`; the yardstick is dz_tune_score on the same
masks (`cache.score(bits)`) and, for the small ones, metrics.DiarizationErrorRate on `cache.hypothesis`."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
from test_tune_host import GAPS, _masks_cache  # noqa: E402

FRAMES = 293
LANES = 256                  # TuneCache.SCORE_LANES


def masks_file(chunks, reference, shift=0.0, uri="masks"):
    seg = np.zeros((chunks, FRAMES, 1), dtype=np.float32)
    emb = np.ones((chunks, 1, 2), dtype=np.float32)
    return dict(uri=uri, seg=seg, emb=emb, starts=tc.starts_for(chunks), res=tc.DURATION / FRAMES, shift=shift,
                reference=reference)


def cache_of(files, max_speakers):
    from diart_amd.optim import TuneCache
    return TuneCache.from_arrays(files, tc.config_of(0.5, 0.3, 1.0, max_speakers, 0.5))


def runs(rows, seed, speakers, on=(3, 90), off=(1, 40)):
    """One uint32 mask per row: every speaker of `speakers` alternates active runs of on[0]..on[1] rows and silences of
    off[0]..off[1] rows (so gaps of 1 to 5 frames, on either side of the patch collar, occur many times)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(rows, dtype=np.uint32)
    for g in speakers:
        p = int(rng.integers(0, off[1]))
        while p < rows:
            n = int(rng.integers(on[0], on[1] + 1))
            out[p:p + n] |= np.uint32(1 << g)
            p += n + int(rng.integers(off[0], off[1] + 1) if rng.random() < 0.6 else rng.integers(1, 6))
    return out


def gap_masks():
    """tests/test_tune_host.py test_score_is_the_diarization_error_rate's four trials: one speaker with gaps of 2, 3 and 4
    frames inside a step and across a step's end, an empty hypothesis, two hypothesis speakers against four in the
    reference, three hypothesis speakers at once."""
    cache, f = _masks_cache()
    rows = cache.total_rows
    bits = np.zeros((4, rows), dtype=np.uint32)
    on = np.zeros(rows, dtype=bool)
    on[5:600] = True
    for start, gap in GAPS(cache):
        on[start:start + gap] = False
    bits[0] = on.astype(np.uint32)
    bits[2] = bits[0] | (np.roll(on, 37).astype(np.uint32) << 2)
    bits[3, 100:130] = 0b1011
    return cache, bits


def lanes_case():
    """One file of 300 chunks: more steps than lanes, two steps per lane (lane i walks steps 2i and 2i + 1).  Speaker 0:
    one turn through 65 lanes.  Speaker 1: active inside lane 5, silent over lanes 6 to 8, back in lane 9 (the end it
    carries crosses three empty lanes).  Speaker 2: gaps of 2 frames that start exactly on a lane boundary (step 40),
    that straddle one (step 60), that straddle a step boundary inside a lane (step 81), and 4-frame gaps at the same
    three kinds of place (steps 100, 120, 141).  Speaker 3: random runs.  A second trial has random runs of all four."""
    chunks = 300
    end = tc.DURATION + tc.STEP * (chunks - 1)
    reference = tc.reference_for(chunks, -0.3, speakers=4) + [(end - 30.0, end - 29.95, "ref1")]
    cache = cache_of([masks_file(chunks, reference, shift=-0.3, uri="lanes")], 4)
    ro, rows = cache.row_off, cache.total_rows
    assert (cache.step_rows[1:] == 30).all() and -(-chunks // LANES) == 2
    bits = np.zeros((2, rows), dtype=np.uint32)
    bits[0, 100:int(ro[2 * 67]) + 11] |= 1
    bits[0, int(ro[10]) + 4:int(ro[11]) + 20] |= 2
    bits[0, int(ro[18]) + 7:int(ro[19]) + 3] |= 2
    two = np.zeros(rows, dtype=bool)
    two[int(ro[30]):int(ro[160])] = True
    for step, before, frames in ((40, 0, 2), (60, 1, 2), (81, 1, 2), (100, 0, 4), (120, 2, 4), (141, 2, 4)):
        two[int(ro[step]) - before:int(ro[step]) - before + frames] = False
    bits[0] |= two.astype(np.uint32) << 2
    bits[0] |= runs(rows, 11, [3])
    bits[1] = runs(rows, 12, [0, 1, 2, 3])
    return cache, bits


def _small(reference, max_speakers, chunks=12, shift=-0.3):
    return cache_of([masks_file(chunks, reference, shift=shift)], max_speakers)


def label_cases():
    """name -> (cache, bits): `str_order` (max_speakers 12, hypothesis speakers 2, 10 and 11: "10" < "11" < "2"),
    `ref34` (34 reference speakers: bits above 31 of the reference mask are live; 3 hypothesis speakers), `hyp5_ref2`
    (more hypothesis than reference labels: the assignment problem's other orientation), `no_overlap` (a hypothesis
    speaker active only where no reference speaker is: its co-occurrence row is zero)."""
    out = {}
    ref4 = [(0.2, 3.1, "a"), (1.0, 2.0, "b"), (1.5, 4.4, "c"), (1.8, 1.9, "d"), (3.0, 3.05, "a"), (4.4, 5.7, "b")]
    cache = _small(ref4, 12)
    bits = np.stack([runs(cache.total_rows, 21, [2, 10, 11]), runs(cache.total_rows, 22, [2, 10, 11], on=(20, 120))])
    out["str_order"] = (cache, bits)
    ref34 = [(0.11 * i, 0.11 * i + 1.3 + 0.07 * (i % 5), f"r{i:02d}") for i in range(34)]
    ref34 += [(6.0, 8.2, "r33"), (6.5, 9.0, "r32"), (7.0, 9.5, "r05")]
    cache = _small(ref34, 4)
    bits = np.stack([runs(cache.total_rows, 23, [0, 1, 3], on=(20, 120)), runs(cache.total_rows, 24, [0, 1, 3])])
    out["ref34"] = (cache, bits)
    cache = _small([(0.2, 3.1, "a"), (1.0, 5.0, "b"), (5.5, 9.0, "a")], 8)
    bits = np.stack([runs(cache.total_rows, 25, [0, 2, 3, 5, 7], on=(20, 120)), runs(cache.total_rows, 26, [0, 2, 3, 5, 7])])
    out["hyp5_ref2"] = (cache, bits)
    cache = _small([(0.2, 3.1, "a"), (1.0, 4.0, "b")], 4)
    late = int(np.searchsorted(cache.mids, 4.5)) + 40          # rows well behind the last reference turn
    bits = np.stack([runs(cache.total_rows, 27, [0, 1]), runs(cache.total_rows, 28, [0, 1], on=(20, 120))])
    bits[:, late:] &= ~np.uint32(0b11)
    bits[:, late + 5:late + 90] |= 1 << 2
    out["no_overlap"] = (cache, bits)
    return out


def pairs_case():
    """Three files of 5, 12 and 300 chunks with different shifts, four trials of which the second is empty: scored by
    two workgroups, every scratch slice is reused five times and an empty hypothesis follows a busy one on both."""
    files = [masks_file(5, tc.reference_for(5, 0.0, 2), shift=0.0, uri="five"),
             masks_file(12, tc.reference_for(12, -1.25, 3), shift=-1.25, uri="twelve"),
             masks_file(300, tc.reference_for(300, -0.3, 4), shift=-0.3, uri="threehundred")]
    cache = cache_of(files, 6)
    bits = np.stack([runs(cache.total_rows, 31, [0, 1, 2, 4]), np.zeros(cache.total_rows, dtype=np.uint32),
                     runs(cache.total_rows, 32, [1, 3, 5], on=(20, 200)), runs(cache.total_rows, 33, [0, 5], off=(1, 8))])
    return cache, bits


def end_to_end_cache():
    """(cache, hparams (17, 3), base configuration): files of 1, 6 and 40 chunks (8 local speakers, 4 centroids); the
    six chunks are tune_cases.failing_step_inputs, whose chain stops at its chunk 3 under the first trial (the base
    configuration's values); 16 uniform draws follow."""
    import types
    K, G, seg, emb = tc.failing_step_inputs(tc.RAISES_SEED)
    F, D = seg.shape[1], emb.shape[2]
    files = [tc.file_of(*tc.random_outputs(301, 1, F, K, D), shift=0.0, uri="one"),
             tc.file_of(seg, emb, shift=-1.25, uri="six"),
             tc.file_of(*tc.random_outputs(302, 40, F, K, D), shift=-0.5, uri="forty")]
    config = tc.config_of(*tc.RAISES_OWN, G, 2.5)
    from diart_amd.optim import TuneCache
    return TuneCache.from_arrays(files, config), tc.random_trials(tc.RAISES_OWN, 17, seed=5), types.SimpleNamespace(**config)


def bars(host):
    """1e-9 x the pair's total, per component: the project's figure for this comparison (tests/test_tune_host.py
    test_score_is_the_diarization_error_rate): the two sides differ only in the order in which at most ~1e5 non-negative
    durations are summed, which moves a sum by at most n x 2^-53 x total."""
    return 1e-9 * host[..., :1]


def check_against_host(cache, bits, got, what):
    host = cache.score(bits)
    assert got.shape == host.shape and (host[..., 0] > 0).all(), what
    worst = np.abs(got - host).max(axis=(0, 1))
    print(what, "largest difference per component", worst, "smallest total", host[..., 0].min())
    assert (np.abs(got - host) <= bars(host)).all(), (what, worst)
    return host


def check_against_metric(cache, bits, got, what):
    from diart_amd.features import Annotation, Segment
    from diart_amd.metrics import COMPONENTS, DiarizationErrorRate
    for n, f in enumerate(cache.files):
        ref = Annotation(uri=f["uri"])
        for i, (s, e, label) in enumerate(f["turns"]):
            ref[Segment(s, e), i] = label
        for t in range(bits.shape[0]):
            comp = DiarizationErrorRate().components(ref, cache.hypothesis(bits[t], n))
            for i, c in enumerate(COMPONENTS):
                assert abs(got[t, n, i] - comp[c]) <= 1e-9 * comp["total"], (what, t, n, c, got[t, n, i], comp[c])
