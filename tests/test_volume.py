"""The ``AdjustVolume`` block without a GPU (DESIGN.md "Volume adjustment"): its public face against the reference's,
the float64 restatement the GPU tests measure the kernel with against what the reference's own block computed
(``tests/golden/adjust_volume.npz``, written by ``tools/make_volume_golden.py``), and that fixture's regeneration."""
import importlib.util
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "adjust_volume.npz"
REFERENCE = Path("/root/reference/src/diart")


def has_reference() -> bool:
    try:
        return (REFERENCE / "blocks" / "utils.py").is_file()
    except OSError:           # a checkout this user may not read counts as absent
        return False

# the largest relative distance between the reference's float32 chain and the float64 restatement over the golden
# cases, measured on the CPU (see test_restatement_matches_the_reference_outputs)
MEASURED_REL = 3.42e-7


# ---------------------------------------------------------------- float64 restatement of blocks/utils.py:125-137
def volumes_f64(x: np.ndarray) -> np.ndarray:
    """(batch, samples, channels) -> (batch, 1, channels) dB: 10 log10(mean(|x|^2))."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return 10.0 * np.log10(np.mean(np.abs(x) ** 2, axis=1, keepdims=True))


def adjust_volume_f64(x: np.ndarray, target_db: float) -> np.ndarray:
    """(batch, samples, channels) -> the same shape: gain = 10 ** ((target_db - volume) / 20), y = gain x,
    out = y / max(max|y|, 1).  A NaN maximum stays NaN (``amax`` and ``clamp`` propagate it): a signal of zero energy
    (inf * 0) or with a NaN / Inf sample comes out all NaN."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        gain = 10.0 ** ((float(target_db) - volumes_f64(x)) / 20.0)
        y = gain * x
        top = np.max(np.abs(y), axis=1, keepdims=True)          # np.max propagates NaN, like torch.amax
        m = np.where(np.isnan(top), np.nan, np.maximum(top, 1.0))
        return y / m


def rel_distance(got: np.ndarray, want: np.ndarray) -> float:
    """Largest |got - want| / |want| over the finite, non-zero entries of ``want``; the NaN patterns must agree."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN patterns differ"
    ok = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def golden_cases():
    g = np.load(GOLDEN)
    return [(g[f"x{i}"], float(g[f"db{i}"]), g[f"y{i}"], g[f"v{i}"]) for i in range(len(g.files) // 4)]


# ---------------------------------------------------------------- tests
def test_block_is_exported_with_the_reference_signature():
    from diart_amd import blocks
    from diart_amd.blocks import AdjustVolume
    from diart_amd.features import TemporalFeatureFormatter
    assert "AdjustVolume" in blocks.__all__
    params = list(inspect.signature(AdjustVolume.__init__).parameters)
    assert params[:2] == ["self", "volume_in_db"]                  # reference: __init__(self, volume_in_db)
    assert inspect.signature(AdjustVolume.__init__).parameters["device"].default is None
    assert isinstance(inspect.getattr_static(AdjustVolume, "get_volumes"), staticmethod)
    assert list(inspect.signature(AdjustVolume.get_volumes).parameters) == ["waveforms"]
    block = AdjustVolume(-20)
    assert block.target_db == -20 and isinstance(block.formatter, TemporalFeatureFormatter)
    if has_reference():
        from oracle.pyannote_stub import load_reference
        ref = load_reference(str(REFERENCE)).blocks_utils.AdjustVolume
        ref_params = list(inspect.signature(ref.__init__).parameters)
        assert params[:len(ref_params)] == ref_params
        assert list(inspect.signature(ref.get_volumes).parameters) == ["waveforms"]
        assert isinstance(inspect.getattr_static(ref, "get_volumes"), staticmethod)
        assert sorted(vars(ref(-20))) == sorted(k for k in vars(block) if k != "device")


def test_get_volumes_matches_the_reference_volumes():
    """(batch, 1, channels), the reference's float32 values to within 1e-5 dB: the golden volumes lie below 64 dB in
    magnitude, where a float32 ulp is 3.8e-6 dB, and the mean and the logarithm each round once."""
    from diart_amd.blocks import AdjustVolume
    for x, _, _, v in golden_cases():
        got = AdjustVolume.get_volumes(torch.from_numpy(x))
        assert tuple(got.shape) == (x.shape[0], 1, x.shape[2]) and got.dtype == torch.float32
        got = got.numpy()
        assert np.array_equal(np.isnan(got), np.isnan(v))
        fin = np.isfinite(v)
        assert np.array_equal(got[~fin & ~np.isnan(v)], v[~fin & ~np.isnan(v)])       # -inf (silence), +inf
        assert np.abs(got[fin] - v[fin]).max(initial=0.0) <= 1e-5


def test_restatement_matches_the_reference_outputs():
    """The float64 restatement above against the outputs of the reference's own block.  Largest relative distance over
    the golden cases, measured on the CPU: 3.42e-7 (cases 256 x 1 and 257 x 2 at -20 dB; the others 0.4 .. 3.0e-7).
    That is the reference's float32 chain: a volume near 40 dB carries an ulp of 3.8e-6 dB, which the exponent turns
    into 4.4e-7 relative per ulp.  The assertion allows twice the measured figure.  NaN rows must match as NaN; the
    reference's volumes agree with the restatement's to 1e-5 dB."""
    worst = 0.0
    for x, db, y, v in golden_cases():
        want = adjust_volume_f64(x, db)
        worst = max(worst, rel_distance(y, want))
        vv = volumes_f64(x)
        fin = np.isfinite(vv)
        assert np.array_equal(np.isnan(v), np.isnan(vv)) and np.array_equal(v[~fin & ~np.isnan(vv)], vv[~fin & ~np.isnan(vv)])
        assert np.abs(v[fin] - vv[fin]).max(initial=0.0) <= 1e-5
    print(f"restatement vs reference: largest relative distance {worst:.3e}")
    assert worst <= 2 * MEASURED_REL
    # the special case: zero energy, NaN first / middle / last, +Inf -> all NaN; its two ordinary rows are not
    x, db, y, _ = golden_cases()[-1]
    assert np.isnan(y[1:6]).all() and np.isfinite(y[0]).all() and np.isfinite(y[6]).all()
    # both branches occur in the fixture: rows divided by their peak (max exactly 1) and rows divided by exactly 1
    peaks = np.concatenate([np.abs(y).max(axis=1).ravel() for _, _, y, _ in golden_cases()[:-1]])
    assert (peaks == 1.0).any() and (peaks < 1.0).any()


@pytest.mark.skipif(not has_reference(), reason="needs the reference checkout")
def test_golden_regenerates_bit_for_bit():
    spec = importlib.util.spec_from_file_location("make_volume_golden", ROOT / "tools" / "make_volume_golden.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    fresh = tool.make(str(REFERENCE))
    g = np.load(GOLDEN)
    assert sorted(g.files) == sorted(fresh)
    for name in g.files:
        a, b = np.asarray(fresh[name]), g[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), name


def test_bad_targets_are_value_errors_before_any_device():
    from diart_amd.blocks import AdjustVolume
    from diart_amd.functional import adjust_volume
    for bad in (float("nan"), float("inf"), "loud", None, True):
        with pytest.raises(ValueError):
            AdjustVolume(bad)
        with pytest.raises(ValueError):
            adjust_volume(np.zeros(4, np.float32), bad)
