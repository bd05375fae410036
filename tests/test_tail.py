"""Aggregation / binarisation tail (host code, no GPU): the product blocks and the oracle
restatement against ``tests/golden/tail.npz`` — outputs of the reference's own
``blocks/aggregation.py`` + ``blocks/utils.py`` (tests/golden/make_golden.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import scenarios  # noqa: E402

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "tail.npz")


def _drive(make_swf, make_pred, make_audio, make_mean, binarize, start_time, latency):
    scores, starts, res = scenarios.tail_inputs(start_time)
    pred, audio, mean = make_pred(latency), make_audio(latency), make_mean(latency)
    pbuf, abuf = [], []
    for i in range(scores.shape[0]):
        pbuf.append(make_swf(scores[i], starts[i], res))
        wav = (np.arange(80000, dtype=np.float64) + 8000.0 * i)[:, None]
        abuf.append(make_swf(wav, starts[i], 1 / 16000))
        agg, aud, mn = pred(pbuf), audio(abuf), mean(pbuf)
        yield i, agg, aud, mn, binarize(agg)
        if len(pbuf) == pred.num_overlapping_windows:
            pbuf, abuf = pbuf[1:], abuf[1:]


def _check(i, tag0, latency, agg, aud, mn, turns):
    tag = f"{tag0}_l{latency:g}_t{i}"
    assert agg.data.shape == GOLD[tag + "_agg"].shape
    assert np.array_equal(agg.data, GOLD[tag + "_agg"]), tag
    assert np.allclose([agg.sliding_window.start, agg.sliding_window.step], GOLD[tag + "_aggsw"], rtol=0, atol=1e-12)
    assert np.array_equal(mn.data, GOLD[tag + "_mean"]), tag
    want = GOLD[tag + "_turns"]
    got = np.array(turns, dtype=np.float64).reshape(-1, 3)
    assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-12), tag
    a = GOLD[tag + "_aud"]
    assert aud.data.shape[0] == int(a[0]) and aud.data[0, 0] == a[1] and aud.data[-1, 0] == a[2]
    assert np.allclose([aud.sliding_window.start, aud.sliding_window.step], a[3:], rtol=0, atol=1e-12)


@pytest.mark.parametrize("start_time", [0.0, 7.5])
@pytest.mark.parametrize("latency", scenarios.TAIL_LATENCIES)
def test_product_tail_matches_reference_golden(start_time, latency):
    from diart_amd.blocks import Binarize, DelayedAggregation
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    binarize = Binarize(0.5)

    def turns(agg):
        return sorted((s.start, s.end, float(t)) for s, t, _ in binarize(agg).itertracks(yield_label=True))
    for i, agg, aud, mn, tr in _drive(
            lambda d, s, r: SlidingWindowFeature(d, SlidingWindow(start=s, duration=r, step=r)),
            lambda l: DelayedAggregation(0.5, l, "hamming", "loose"),
            lambda l: DelayedAggregation(0.5, l, "first", "center"),
            lambda l: DelayedAggregation(0.5, l, "mean", "strict"), turns, start_time, latency):
        _check(i, f"s{start_time:g}", latency, agg, aud, mn, tr)


@pytest.mark.parametrize("start_time", [0.0, 7.5])
@pytest.mark.parametrize("latency", scenarios.TAIL_LATENCIES)
def test_oracle_tail_matches_reference_golden(start_time, latency):
    from oracle.pyannote_stub import SlidingWindow, SlidingWindowFeature
    from oracle.tail_ref import DelayedAggregationRef, binarize_ref
    for i, agg, aud, mn, tr in _drive(
            lambda d, s, r: SlidingWindowFeature(d, SlidingWindow(start=s, duration=r, step=r)),
            lambda l: DelayedAggregationRef(0.5, l, "hamming", "loose"),
            lambda l: DelayedAggregationRef(0.5, l, "first", "center"),
            lambda l: DelayedAggregationRef(0.5, l, "mean", "strict"),
            lambda agg: binarize_ref(agg, 0.5), start_time, latency):
        _check(i, f"s{start_time:g}", latency, agg, aud, mn, tr)


@pytest.mark.parametrize("latency", scenarios.TAIL_LATENCIES)
def test_cpp_batched_tail_matches_reference_golden(latency):
    """dz_tail_step_batch (C++, what StreamBatch uses for N streams) against the same goldens of
    the reference's aggregation.py + utils.py: two streams (starting at 0 s and 7.5 s) stepped
    together; hamming/loose aggregation + turns, mean/strict aggregation, first/center audio."""
    from diart_amd.blocks.aggregation import BatchedOutputTail
    starts_of = (0.0, 7.5)
    inputs = [scenarios.tail_inputs(s0) for s0 in starts_of]
    T, F, G = inputs[0][0].shape
    res = inputs[0][2]
    pred = BatchedOutputTail(2, F, G, 0.5, latency, threshold=0.5, num_threads=2)
    mean = BatchedOutputTail(2, F, G, 0.5, latency, strategy="mean", cropping_mode="strict", num_threads=1)
    audio = BatchedOutputTail(2, 80000, 1, 0.5, latency, strategy="first", cropping_mode="center",
                              max_turns=4)
    assert pred.num_overlapping_windows == int(round(latency / 0.5))
    for i in range(T):
        scores = np.stack([inp[0][i] for inp in inputs])
        starts = np.array([inp[1][i] for inp in inputs])
        agg, rows, t0, r, turns, nturns = pred(scores, starts, res)
        magg, mrows, _, _, _, _ = mean(scores, starts, res)
        wav = np.repeat((np.arange(80000, dtype=np.float64) + 8000.0 * i)[None, :, None], 2, axis=0)
        aagg, arows, at0, ar, _, _ = audio(wav, starts, 1 / 16000)
        for k, s0 in enumerate(starts_of):
            tag = f"s{s0:g}_l{latency:g}_t{i}"
            want = GOLD[tag + "_agg"]
            assert rows[k] == want.shape[0] and np.array_equal(agg[k, :rows[k]], want), tag
            assert np.allclose([t0[k], r[k]], GOLD[tag + "_aggsw"], rtol=0, atol=1e-12), tag
            assert np.array_equal(magg[k, :mrows[k]], GOLD[tag + "_mean"]), tag
            wt = GOLD[tag + "_turns"]
            got = np.array(sorted(map(tuple, turns[k, :nturns[k]])), dtype=np.float64).reshape(-1, 3)
            assert got.shape == wt.shape and np.allclose(got, wt, rtol=0, atol=1e-12), tag
            a = GOLD[tag + "_aud"]
            assert arows[k] == int(a[0]) and aagg[k, 0, 0] == a[1] and aagg[k, arows[k] - 1, 0] == a[2], tag
            assert np.allclose([at0[k], ar[k]], a[3:], rtol=0, atol=1e-12), tag
    pred.reset()
    agg, rows, *_ = pred(np.stack([inp[0][0] for inp in inputs]), np.array([0.0, 7.5]), res)
    assert np.array_equal(agg[0, :rows[0]], GOLD[f"s0_l{latency:g}_t0_agg"])


def test_cpp_tail_equals_the_python_blocks_for_every_strategy_and_mode():
    """dz_tail_step against DelayedAggregation + Binarize (which the goldens above pin) for all nine strategy x cropping
    mode pairs, on three frame grids, four (step, latency) pairs and four first starts, 14 steps of seeded uniform
    scores each: the aggregated rows, t0, res and the sorted turns are EQUAL (no tolerance) at every step.  Where the
    Python block raises (np.stack on unequal crops) dz_tail_step returns 4 and the other way round; the chain ends
    there.  Both are counted and the counts must agree; fewer than 2 % of the steps may end so, or the sweep would
    check little.  For hamming / loose the tuner's plan (dz_tune_plan) of the chain's starts must give the same rows,
    t0 and res: the GPU tuner hangs on the same text (csrc/tail_core.h).

    (step, latency) = (0.1, 2.0) — 20 buffers — is not in the sweep on purpose: from the 8th buffer on, where the region
    has one or two rows, numpy sums the short stacked axis pairwise and the C++ tail sums in order, and "hamming" differs
    in the last bits.  The shipped shape (293 frames, step 0.5, up to 10 buffers) is exact."""
    import ctypes as C
    import itertools
    from diart_amd import _lib
    from diart_amd.blocks import Binarize, DelayedAggregation
    from diart_amd.blocks.aggregation import _MODE, _STRATEGY
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    lib = _lib.load()
    binarize = Binarize(0.5)
    rng = np.random.default_rng(0)
    steps = py_raised = cpp_rc4 = 0
    bad = []
    for (F, G), strategy, mode, (step, latency), first_start in itertools.product(
            [(7, 2), (59, 3), (293, 4)], _STRATEGY, _MODE, [(0.5, 0.5), (0.5, 1.5), (0.5, 5.0), (0.3, 0.9)],
            [0.0, 7.5, -1.75, 0.3]):
        case = (F, G, strategy, mode, step, latency, first_start)
        res = 5 / F
        hamming = np.ascontiguousarray(np.hamming(F))
        h = _lib.vp()
        _lib.check(lib.dz_tail_create(F, G, step, latency, 0.5, _STRATEGY[strategy], _MODE[mode], hamming.ctypes.data,
                                      C.byref(h)), "dz_tail_create")
        agg = DelayedAggregation(step, latency, strategy, mode)
        out, max_turns = np.empty((F + 2, G)), G * ((F + 2) // 2 + 1)
        turns = np.empty((max_turns, 3))
        rows, nturns, t0, r = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        buffers, start, starts, done = [], first_start, [], []
        failed = False
        for i in range(14):
            scores = rng.random((F, G))
            buffers.append(SlidingWindowFeature(scores, SlidingWindow(start=start, duration=res, step=res)))
            starts.append(start)
            rc = lib.dz_tail_step(h, scores.ctypes.data, start, res, out.ctypes.data, C.byref(rows), C.byref(t0),
                                  C.byref(r), turns.ctypes.data, max_turns, C.byref(nturns))
            steps += 1
            try:
                want = agg(buffers)
            except (ValueError, ZeroDivisionError):   # np.stack on unequal crops; a region of no rows at all
                want = None
            py_raised += want is None
            cpp_rc4 += rc == 4
            if want is None or rc:
                failed = True
                if not (want is None and rc == 4):
                    bad.append((case, i, f"rc {rc}, python {'raised' if want is None else 'did not raise'}"))
                break
            sw = want.sliding_window
            want_turns = sorted((s.start, s.end, float(t)) for s, t, _ in binarize(want).itertracks(yield_label=True))
            got_turns = sorted(map(tuple, turns[:nturns.value]))
            if not (rows.value == want.data.shape[0] and np.array_equal(out[:rows.value], want.data)
                    and t0.value == sw.start and r.value == sw.step and got_turns == want_turns):
                bad.append((case, i, "rows / t0 / res / turns differ"))
            done.append((rows.value, t0.value, r.value))
            if len(buffers) == agg.num_overlapping_windows:
                buffers = buffers[1:]
            start += step
        lib.dz_tail_destroy(h)
        if strategy == "hamming" and mode == "loose":
            nwin = agg.num_overlapping_windows
            s_arr, r_arr = np.array(starts), np.full(len(starts), res)
            plan = np.zeros((len(starts), 4 + nwin), dtype=np.int32)
            pt0, pres = np.zeros(len(starts)), np.zeros(len(starts))
            rc = lib.dz_tune_plan(len(starts), F, step, latency, s_arr.ctypes.data, r_arr.ctypes.data, plan.ctypes.data,
                                  pt0.ctypes.data, pres.ctypes.data)
            if rc != (4 if failed else 0):
                bad.append((case, len(starts) - 1, f"dz_tune_plan returned {rc}"))
            got = [(int(p[0] + p[1]), a, b) for p, a, b in zip(plan[:len(done)], pt0, pres)]   # (the steps before a 4)
            if got != done:
                bad.append((case, -1, "dz_tune_plan and dz_tail_step differ in rows / t0 / res"))
    print(f"{steps} steps, python raised at {py_raised}, dz_tail_step returned 4 at {cpp_rc4}, {len(bad)} differ")
    assert not bad, bad[:5]
    assert py_raised == cpp_rc4
    assert py_raised < 0.02 * steps, (steps, py_raised)


@pytest.mark.parametrize("threads", [1, 4])
def test_batches_report_the_lowest_failing_item(threads):
    """Two items of a batch fail: the code and the message are those of the LOWEST index, on one thread and on the
    pool (where which worker met a failure first is a matter of timing).  On the pool the items that did not fail have
    been stepped; on one thread the call ends at the first failure."""
    import ctypes as C
    from diart_amd import _lib
    lib = _lib.load()
    F, n, res = 59, 4, 5 / 59
    hamming = np.ascontiguousarray(np.hamming(F))
    hs = []
    for _ in range(n):
        h = _lib.vp()
        _lib.check(lib.dz_tail_create(F, 1, 0.5, 0.5, 0.5, 0, 1, hamming.ctypes.data, C.byref(h)), "dz_tail_create")
        hs.append(h)
    handles = (_lib.vp * n)(*hs)
    # dz_tail_step_batch: stream 1 gets resolution 0 (code 2), stream 3 a region of more than F + 2 rows (code 4)
    scores = np.zeros((n, F, 1))
    scores[:, 10:20] = 1.0
    scores[:, 30:40] = 1.0            # two speech turns per stream
    starts = np.zeros(n)
    resolution = np.array([res, 0.0, res, res / 100])
    agg, turns = np.empty((n, F + 2, 1)), np.empty((n, 8, 3))
    rows = np.full(n, -1, dtype=np.int32)
    nturns = np.full(n, -1, dtype=np.int32)
    t0, r = np.empty(n), np.empty(n)
    rc = lib.dz_tail_step_batch(handles, n, scores.ctypes.data, starts.ctypes.data, resolution.ctypes.data, agg.ctypes.data,
                                rows.ctypes.data, t0.ctypes.data, r.ctypes.data, turns.ctypes.data, 8, nturns.ctypes.data,
                                threads)
    assert rc == 2 and lib.dz_last_error() == b"dz_tail_step_batch: bad arguments"
    assert rows[0] > 0 and nturns[0] == 2 and rows[1] == -1 and rows[3] == -1
    assert (rows[2] > 0 and nturns[2] == 2) if threads > 1 else rows[2] == -1
    # dz_file_vad_step_batch: one window per file, room for one turn: files 1 and 2 have two (code 5), file 0 is silent
    for h in hs:
        lib.dz_tail_reset(h)
    track = np.ascontiguousarray(scores[:3, :, 0], dtype=np.float32)
    track[0] = 0.0
    row0, count = np.arange(3, dtype=np.int32), np.ones(3, dtype=np.int32)
    fstarts, fturns, fn = np.zeros(3), np.empty((3, 1, 3)), np.zeros(3, dtype=np.int32)
    rc = lib.dz_file_vad_step_batch(handles, 3, row0.ctypes.data, count.ctypes.data, track.ctypes.data, F, fstarts.ctypes.data,
                                    res, fturns.ctypes.data, 1, fn.ctypes.data, threads)
    assert rc == 5
    assert lib.dz_last_error() == b"dz_file_vad_step_batch: file 1 of 3 failed (code 5): dz_tail_step: more speech turns than max_turns"
    for h in hs:
        lib.dz_tail_destroy(h)


def test_docstring_example_of_the_reference():
    """aggregation.py:141-161: 5 s / 500 frames / step 0.5 / latency 2 -> 4 windows, (51, 2)."""
    from diart_amd.blocks import DelayedAggregation
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    dagg = DelayedAggregation(step=0.5, latency=2, strategy="mean")
    res = 5 / 500
    bufs = [SlidingWindowFeature(np.random.rand(500, 2), SlidingWindow(start=(i + 10) * 0.5, duration=res, step=res))
            for i in range(dagg.num_overlapping_windows)]
    assert dagg.num_overlapping_windows == 4 and dagg(bufs).data.shape == (51, 2)


def test_der_metric_known_answers():
    from diart_amd.features import Annotation, Segment
    from diart_amd.metrics import DetectionErrorRate, DiarizationErrorRate
    ref, hyp = Annotation("f"), Annotation("f")
    ref[Segment(0, 10), 0] = "A"
    ref[Segment(5, 15), 1] = "B"          # 5 s of overlap: total = 20
    hyp[Segment(0, 10), 0] = "x"          # = A
    hyp[Segment(10, 15), 1] = "y"         # = B on [10,15]; B missed on [5,10]
    hyp[Segment(15, 17), 2] = "y"         # 2 s false alarm
    der = DiarizationErrorRate()
    d = der(ref, hyp, detailed=True)
    assert d["total"] == 20 and d["missed detection"] == 5 and d["false alarm"] == 2 and d["confusion"] == 0
    assert abs(d["diarization error rate"] - 7 / 20) < 1e-12 and abs(abs(der) - 7 / 20) < 1e-12
    # label permutation does not matter, swapping speakers mid-way is confusion
    hyp2 = Annotation("f")
    hyp2[Segment(0, 5), 0] = "p"
    hyp2[Segment(5, 10), 1] = "q"
    ref2 = Annotation("f")
    ref2[Segment(0, 10), 0] = "A"
    assert abs(DiarizationErrorRate()(ref2, hyp2) - 0.5) < 1e-12
    assert DiarizationErrorRate()(ref, ref) == 0.0
    det = DetectionErrorRate()(ref, hyp, detailed=True)
    assert det["total"] == 15 and det["false alarm"] == 2 and det["missed detection"] == 0


def test_rttm_roundtrip(tmp_path):
    from diart_amd.features import Annotation, Segment, load_rttm
    ann = Annotation("meeting1")
    ann[Segment(0.5, 2.25), 0] = "speaker0"
    ann[Segment(1.0, 3.0), 1] = "speaker1"
    p = tmp_path / "x.rttm"
    with open(p, "w") as f:
        ann.write_rttm(f)
    assert p.read_text().splitlines()[0] == "SPEAKER meeting1 1 0.500 1.750 <NA> <NA> speaker0 <NA> <NA>"
    back = load_rttm(p)["meeting1"]
    assert [(s.start, s.end, l) for s, _, l in back.itertracks(yield_label=True)] == \
           [(0.5, 2.25, "speaker0"), (1.0, 3.0, "speaker1")]
