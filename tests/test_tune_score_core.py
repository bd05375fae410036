"""The tuner's device scoring without a GPU: the text tune_score_kernel is compiled from (csrc/tune_core.h tc_score_pair),
run on host threads with the workgroup's 256 lanes played in order (backend="core", scoring="device";
dz_tune_score_core), against dz_tune_score on the same masks and, for the small cases, against
metrics.DiarizationErrorRate on cache.hypothesis.  Never against itself.  Tolerance: 1e-9 x the pair's total per
component (tune_score_cases.bars): the two sides differ only in the order in which the durations are summed."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402
import tune_score_cases as sc  # noqa: E402


def _core(cache, bits, **kw):
    return cache.score(bits, scoring="device", backend="core", **kw)


def test_gap_masks():
    """Gaps of 2, 3 and 4 frames inside a step and across a step's end, an empty hypothesis, two hypothesis speakers
    against four reference speakers, three hypothesis speakers at once."""
    cache, bits = sc.gap_masks()
    got = _core(cache, bits)
    sc.check_against_host(cache, bits, got, "gaps")
    sc.check_against_metric(cache, bits, got, "gaps")
    assert got[1, 0, 3] == got[1, 0, 0] and got[1, 0, 2] == 0.0 and got[1, 0, 1] == 0.0 and got[1, 0, 4] == 0.0


def test_more_steps_than_lanes():
    """300 chunks on 256 lanes: a turn through dozens of lanes, a label whose carried end crosses empty lanes,
    sub-collar gaps exactly on a lane boundary and on a step boundary."""
    cache, bits = sc.lanes_case()
    got = _core(cache, bits)
    host = sc.check_against_host(cache, bits, got, "lanes")
    sc.check_against_metric(cache, bits[:1], got[:1], "lanes")
    assert (host[:, 0, 1] > 10.0).all() and (host[:, 0, 2] > 1.0).all() and (host[:, 0, 4] > 1.0).all()
    # the 2-frame gaps of speaker 2 are patched and the 4-frame gaps are not, wherever they fall
    turns = sorted((s.start, s.end) for s, _, l in cache.hypothesis(bits[0], 0).itertracks(yield_label=True) if l == "speaker2")
    assert len(turns) == 4, turns


@pytest.mark.parametrize("name", ["str_order", "ref34", "hyp5_ref2", "no_overlap"])
def test_labels(name):
    """The hypothesis labels in str order ("10" < "2"), reference bits above 31, both orientations of the assignment
    problem, a hypothesis speaker whose co-occurrence row is zero."""
    cache, bits = sc.label_cases()[name]
    got = _core(cache, bits)
    host = sc.check_against_host(cache, bits, got, name)
    sc.check_against_metric(cache, bits, got, name)
    assert (host[:, 0, 1] > 0.5).all(), "nothing was mapped"
    if name == "ref34":
        assert len(cache.ref_labels[0]) == 34 and int(cache.cell_ref.max()) >> 32
    if name == "no_overlap":
        assert (host[:, 0, 2] > 1.0).all()


def test_pairs_share_two_slices():
    """Three files of 5, 12 and 300 chunks with different shifts, four trials, two workgroups: every scratch slice is
    reused and the empty hypothesis follows a busy one on the same slice.  The same numbers whatever the number of
    workgroups and of host threads: a pair's result does not depend on what its slice held."""
    cache, bits = sc.pairs_case()
    got = _core(cache, bits, score_blocks=2)
    host = sc.check_against_host(cache, bits, got, "pairs")
    assert (host[1, :, 1] == 0).all() and (host[1, :, 3] == host[1, :, 0]).all() and (host[[0, 2, 3], :, 1] > 0).all()
    assert np.array_equal(got, _core(cache, bits, score_blocks=1, num_threads=1))
    assert np.array_equal(got, _core(cache, bits, score_blocks=5))
    assert np.array_equal(got, _core(cache, bits))


def test_refusals():
    cache, bits = sc.gap_masks()
    hp = np.array([[0.5, 0.3, 1.0]])
    with pytest.raises(ValueError, match="scoring='device'.*backend='gpu'.*backend='core'"):
        cache.evaluate(hp, backend="host", scoring="device")
    with pytest.raises(ValueError, match="scoring 'gpu'"):
        cache.evaluate(hp, backend="host", scoring="gpu")
    with pytest.raises(ValueError, match="scoring 'fast'"):
        cache.score(bits, scoring="fast")
    # steps whose grids are not sorted by time: the kernel's text refuses, dz_tune_score sorts
    f = sc.masks_file(6, tc.reference_for(6, 0.0, 2))
    f["starts"] = f["starts"][::-1].copy()
    backwards = sc.cache_of([f], 4)
    assert not backwards.sorted_steps and cache.sorted_steps
    some = sc.runs(backwards.total_rows, 41, [0, 1])[None]
    with pytest.raises(ValueError, match="not sorted by time"):
        backwards.score(some, scoring="device", backend="core")
    with pytest.raises(ValueError, match="not sorted by time"):
        backwards.evaluate(hp, backend="core", scoring="device")
    backwards.score(some)
    # a bit at or above max_speakers is no speaker, as in dz_tune_score
    extra = bits.copy()
    extra[:, 50:300] |= np.uint32(1 << 4) | np.uint32(1 << 31)
    assert cache.G == 4 and np.array_equal(cache.score(extra), cache.score(bits))
    assert np.array_equal(_core(cache, extra), _core(cache, bits))
    from diart_amd.blocks.diarization import SpeakerDiarization
    from diart_amd.blocks.vad import VoiceActivityDetection
    from diart_amd.optim import Optimizer
    with pytest.raises(ValueError, match="scoring 'fast'"):
        Optimizer(SpeakerDiarization, None, None, "study", cache=cache, scoring="fast")
    with pytest.raises(ValueError, match="VoiceActivityDetection is scored where it is replayed"):
        Optimizer(VoiceActivityDetection, None, None, "study", scoring="device")


def test_default_path_is_host_scoring():
    """evaluate(scoring=None) is evaluate(scoring="host"), array for array, and the kernel's text gives the same statuses
    and, within the tolerance, the same components through evaluate (one trial's chain stops)."""
    cache, hp, _ = sc.end_to_end_cache()
    a, b = cache.evaluate(hp, backend="host"), cache.evaluate(hp, backend="host", scoring="host")
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    c = cache.evaluate(hp, backend="core", scoring="device", memory_budget=4 * cache.bytes_per_trial)
    assert np.array_equal(a.status, c.status) and a.status[0].tolist() == [-1, 3, -1] and (a.status[1:] == -1).all()
    assert (np.abs(a.per_file - c.per_file) <= sc.bars(a.per_file)).all()
    assert np.array_equal(np.isnan(a.rate), np.isnan(c.rate)) and np.isnan(a.rate).sum() == 1


def test_command_line_and_optimizer_take_scoring(tmp_path):
    from diart_amd import tune
    from diart_amd.blocks.diarization import SpeakerDiarization
    from diart_amd.optim import Optimizer
    args = tune.parser().parse_args(["wav", "--reference", "rttm", "--output", "study", "--scoring", "device"])
    assert args.scoring == "device"
    assert tune.parser().parse_args(["wav", "--reference", "rttm", "--output", "study"]).scoring is None
    cache, _, config = sc.end_to_end_cache()
    rates = {}
    for scoring in (None, "device"):
        opt = Optimizer(SpeakerDiarization, None, None, tmp_path / f"study_{scoring}", base_config=config, cache=cache,
                        backend="core", scoring=scoring, seed=2)
        opt(6, show_progress=False)
        rates[scoring] = np.array([np.nan if t["value"] is None else t["value"] for t in opt.trials])
    assert np.isnan(rates[None][0]) and np.isfinite(rates[None][1:]).all()
    assert np.allclose(rates[None], rates["device"], rtol=1e-9, atol=0.0, equal_nan=True)
