"""The tuner's scoring kernel (csrc/k_tune_score.hip) against dz_tune_score on the same masks: the five components of
every (trial, file) pair within 1e-9 x the pair's total (tune_score_cases.bars: the two sides differ only in the order
in which the durations are summed), and two calls of the kernel bitwise equal (no floating-point atomics).  The masks
are tests/tune_score_cases.py's, the ones tests/test_tune_score_core.py scores with the kernel's text on the host."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_score_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"gaps": sc.gap_masks, "lanes": sc.lanes_case, "pairs": sc.pairs_case,
         **{name: (lambda name=name: sc.label_cases()[name]) for name in ("str_order", "ref34", "hyp5_ref2", "no_overlap")}}


@pytest.mark.parametrize("name", list(CASES))
def test_masks(gpu, name):
    """Gap masks, more steps than lanes, the label cases, and three files x four trials on two scratch slices."""
    import torch
    cache, bits = CASES[name]()
    blocks = 2 if name == "pairs" else None
    got = cache.score(bits, scoring="device", score_blocks=blocks)
    sc.check_against_host(cache, bits, got, name)
    if name != "pairs":
        sc.check_against_metric(cache, bits[:1], got[:1], name)
    # from a device tensor, as evaluate has them: the same doubles, call after call
    d_bits = torch.from_numpy(bits.view(np.int32)).to(gpu)
    again = cache.score(d_bits, scoring="device", score_blocks=blocks)
    assert np.array_equal(got, again), name
    if name == "pairs":          # whatever a slice held before: one slice for all pairs, one per pair
        assert np.array_equal(got, cache.score(d_bits, scoring="device", score_blocks=1))
        assert np.array_equal(got, cache.score(d_bits, scoring="device"))


def test_evaluate_end_to_end(gpu):
    """Replay and scoring both on the device against the replay on the device and dz_tune_score on the host: 16 random
    trials and one whose chain stops, trials in batches of five."""
    cache, hp, _ = sc.end_to_end_cache()
    host = cache.evaluate(hp, backend="gpu")
    dev = cache.evaluate(hp, backend="gpu", scoring="device", memory_budget=5 * cache.bytes_per_trial)
    assert np.array_equal(host.status, dev.status) and host.status[0].tolist() == [-1, 3, -1]
    print("largest difference per component", np.abs(host.per_file - dev.per_file).max(axis=(0, 1)))
    assert (np.abs(host.per_file - dev.per_file) <= sc.bars(host.per_file)).all()
    assert np.array_equal(np.isnan(host.rate), np.isnan(dev.rate)) and np.isnan(host.rate).sum() == 1
    assert np.abs(host.rate - dev.rate)[1:].max() <= 3e-9
    again = cache.evaluate(hp, backend="gpu", scoring="device")
    assert np.array_equal(dev.per_file, again.per_file)


def test_optimizer(gpu, tmp_path):
    """Optimizer(..., scoring="device") and Optimizer(...) on the same cache and seed: the stored rates agree within
    1e-9 relative, and so does the best trial unless two rates tie within that."""
    from diart_amd.blocks.diarization import SpeakerDiarization
    from diart_amd.optim import Optimizer
    cache, _, config = sc.end_to_end_cache()
    opts = {}
    for scoring in (None, "device"):
        opts[scoring] = Optimizer(SpeakerDiarization, None, None, tmp_path / f"study_{scoring}", base_config=config,
                                  cache=cache, backend="gpu", scoring=scoring, seed=7, do_kickstart_hparams=False)
        opts[scoring](32, show_progress=False)
    a, b = opts[None].trials, opts["device"].trials
    assert len(a) == 32 and [t["params"] for t in a] == [t["params"] for t in b]
    assert [t["value"] is None for t in a] == [t["value"] is None for t in b]
    va, vb = (np.array([t["value"] for t in ts if t["value"] is not None]) for ts in (a, b))
    assert va.shape[0] >= 16 and (np.abs(va - vb) <= 1e-9 * np.abs(va)).all()
    best = np.sort(va)
    if best[1] - best[0] > 1e-9 * best[1]:
        assert opts[None].best_trial["number"] == opts["device"].best_trial["number"]
    assert abs(opts[None].best_performance - opts["device"].best_performance) <= 1e-9 * opts[None].best_performance
