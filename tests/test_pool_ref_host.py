"""tests/pool_ref.py on the CPU: the restatement against the oracle and torch's own resampling, the float32 floor of every
cell tests/test_gpu_pool_f64.py gates, and that the measure catches each planted fault where that fault is visible.
No GPU, no library."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pool_ref as R  # noqa: E402


# --------------------------------------------------------------------------- resampling
def _pairs():
    used = {(Fw, geom[1]) for geom in R.GEOMETRIES for _, Fw in R.modes(geom)} | {(R.RANDOM_FW, R.RANDOM_GEOM[1])}
    # thinned from the full sweep 2 <= F < 700, 2 <= T <= 640 (no disagreement anywhere): every 7th x every 5th, and the edges
    sweep = {(Fw, T) for Fw in range(2, 700, 7) for T in range(2, 641, 5)}
    edges = {(Fw, T) for Fw in (2, 3, 293, 589, 699) for T in (2, 3, 279, 575, 640)}
    return sorted(used | sweep | edges)


def test_resampling_is_torch_interpolate():
    g = torch.Generator().manual_seed(1)
    for Fw, T in _pairs():
        w = torch.rand(2, Fw, generator=g, dtype=torch.float64)
        if Fw == T:
            assert torch.equal(R.resample(w, T, "linear"), w) and torch.equal(R.resample(w, T, "nearest"), w)
            continue
        # nearest picks elements.  The rule is the one of float32 tensors (what the model runs on: scale and product in
        # float32; on a float64 tensor torch takes them in float64 and, e.g., (F, T) = (2, 82) picks another frame) and
        # the float64 restatement keeps it: same elements, wider arithmetic behind them
        idx = F.interpolate(torch.arange(Fw, dtype=torch.float32)[None, None], size=T, mode="nearest")[0, 0].long()
        assert torch.equal(R.nearest_index(Fw, T), idx), (Fw, T)
        assert torch.equal(R.resample(w, T, "nearest"), w[:, idx])
        assert torch.equal(R.resample(w.float(), T, "nearest", R.F32), F.interpolate(w.float()[:, None], size=T, mode="nearest")[:, 0])
        lin = F.interpolate(w[:, None], size=T, mode="linear", align_corners=False)[:, 0]
        assert (R.resample(w, T, "linear") - lin).abs().max().item() <= 1e-13, (Fw, T)
        lin32 = F.interpolate(w.float()[:, None], size=T, mode="linear", align_corners=False)[:, 0]
        assert (R.resample(w.float(), T, "linear", R.F32) - lin32).abs().max().item() <= 4 * Fw * 2.0 ** -24, (Fw, T)   # the source position, <= Fw, in float32


def test_pool_is_the_oracle_in_float64():
    from oracle.models_ref import stats_pool_ref
    g = torch.Generator().manual_seed(2)
    nx, K, T, C = 3, 2, 279, 24
    x = torch.randn(nx, T, C, generator=g)
    seq = x.double().permute(0, 2, 1).repeat_interleave(K, dim=0)                # (rows, C, T)
    for mode, Fw in (("linear", 293), ("nearest", 293), ("linear", 279), (None, 0)):
        w = torch.rand(nx * K, Fw, generator=g, dtype=torch.float64) ** 2 + 1e-8 if Fw else None
        want = stats_pool_ref(seq, w, interp_mode=mode or "linear")
        mean, std = R.pool(x, None if w is None else R.resample(w, T, mode), K)
        got = torch.cat([mean, std], 1)
        assert got.dtype == torch.float64
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), (mode, Fw)


def test_planes_value_is_exact():
    v = torch.randn(1000) * torch.exp2(torch.randint(-6, 6, (1000,)).float())
    q = R.q22(v)
    assert ((q - v).abs() <= v.abs() * 2.0 ** -21).all() and torch.equal(R.q22(q), q)


# --------------------------------------------------------------------------- the float32 floor of every cell
@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=R.geom_id)
def test_float32_floor_and_degenerate_rows_of_every_cell(geom):
    """e32 <= 2e-5 wherever the GPU test gates, and the inputs hold exactly the degenerate rows they are built to hold"""
    P, T, nx = geom
    worst = {}
    for feat in R.FEATURES:
        for K, mode, Fw, fam in R.cells(geom):
            w, ref, e32 = R.cell_ref(geom, feat, K, mode, Fw, fam)
            assert e32 <= R.E32_CAP, (geom, feat, K, mode, Fw, fam, e32)
            worst[(feat, fam)] = max(worst.get((feat, fam), 0.0), e32)
            single = int((ref.mean_ok & ~ref.std_ok).sum())
            none = int((~ref.mean_ok).sum())
            assert (single, none) == R.expected_degenerate(fam, geom, K, mode, Fw), (geom, K, mode, Fw, fam, single, none)
            ok = ref.std_ok
            assert torch.isfinite(ref.mean[ref.mean_ok]).all() and torch.isfinite(ref.std[ok]).all()
            assert torch.isfinite(ref.std_scale[ok]).all() and (ref.std_scale[ok] > 0).all()
            assert torch.isnan(ref.mean[~ref.mean_ok]).all() and torch.isnan(ref.std[~ref.mean_ok]).all()
    print("\n" + R.geom_id(geom) + " worst e32: " + "  ".join(f"{k[0]}/{k[1]} {v:.1e}" for k, v in sorted(worst.items())))


def test_random_case_floor():
    c = R.random_case()
    assert c["e32"] <= R.E32_CAP and c["ref"].std_ok.all()


def test_features_are_what_the_layer_computes():
    """the exact features against the layer in float64: leaky(X W^T + 0) * e0 + 0 on the 22-bit operands"""
    for geom in ((129, 129, 9), (293, 279, 5)):
        for feat in R.FEATURES:
            f = R.features(geom, feat)
            assert torch.equal(R.q22(f["W"]), f["W"]) and torch.equal(R.q22(f["X"]), f["X"]) and (f["W"] >= 0).all()
            v = f["X"].double() @ f["W"].double().t()
            y = torch.where(v > 0, v, 0.01 * v) * f["e0"].double()
            assert torch.equal(y.view(f["y"].shape), f["y"].double())
            assert (f["e0"] == 1).any() and (f["e0"] == -1).any()
            P, T, nx = geom
            if P > T:                                  # the frames nobody may read are 2^10 larger than their family
                assert f["y"][:, T:].abs().max() >= 100 * f["y"][:, :T].abs().max()


# --------------------------------------------------------------------------- the measure catches each planted fault
# (fault, geometry, feature family, K, mode, Fw, weight family): cases on which the fault changes the result at all
PLANTED = [
    ("biased_denominator", (293, 279, 5), "randn", 3, "linear", 293, "dense"),
    ("biased_denominator", (293, 279, 5), "offset", 4, "nearest", 293, "peaky"),
    ("biased_denominator", (129, 129, 9), "sparse", 2, "identity", 129, "two_frames"),
    ("biased_denominator", (128, 2, 3), "randn", 1, "identity", 2, "unweighted"),
    ("boundary_frame", (129, 129, 9), "randn", 3, "identity", 129, "dense"),
    ("boundary_frame", (129, 2, 9), "offset", 1, "identity", 2, "dense"),
    ("boundary_frame", (293, 279, 5), "sparse", 4, "identity", 279, "unweighted"),
    ("boundary_frame", (589, 575, 2), "randn", 2, "identity", 575, "dense"),
    ("pitch_frames", (293, 279, 5), "randn", 3, "linear", 293, "dense"),
    ("pitch_frames", (293, 279, 5), "offset", 1, "identity", 279, "unweighted"),
    ("pitch_frames", (320, 300, 2), "sparse", 4, "identity", 300, "peaky"),
    ("pitch_frames", (129, 2, 9), "randn", 2, "identity", 2, "dense"),
    ("swapped_mode", (293, 279, 5), "randn", 3, "nearest", 293, "peaky"),
    ("swapped_mode", (293, 279, 5), "offset", 2, "linear", 293, "peaky"),
    ("swapped_mode", (293, 279, 5), "sparse", 4, "linear", 293, "peaky"),
    ("next_speaker", (293, 279, 5), "randn", 3, "linear", 293, "dense"),
    ("next_speaker", (129, 129, 9), "offset", 2, "identity", 129, "peaky"),
    ("next_speaker", (589, 575, 2), "sparse", 4, "identity", 575, "stretch"),
    ("one_pass", (293, 279, 5), "offset", 3, "linear", 293, "dense"),
    ("one_pass", (293, 279, 5), "offset", 4, "nearest", 293, "peaky"),
    ("one_pass", (589, 575, 2), "offset", 2, "identity", 575, "stretch"),
    ("one_pass", (129, 129, 9), "offset", 1, "identity", 129, "unweighted"),
]


@pytest.mark.parametrize("fault,geom,feat,K,mode,Fw,fam", PLANTED,
                         ids=[f"{p[0]}-{R.geom_id(p[1])}-{p[2]}-K{p[3]}-{p[4]}-{p[6]}" for p in PLANTED])
def test_measure_catches_the_planted_fault(fault, geom, feat, K, mode, Fw, fam):
    """each fault, planted into the float32 restatement, leaves the gate of its cell — in the half it damages"""
    P, T, nx = geom
    assert (K, mode, Fw, fam) in R.cells(geom)                 # a cell the GPU test runs
    w, ref, e32 = R.cell_ref(geom, feat, K, mode, Fw, fam)
    g = R.gate(e32)
    em, es = ref.errors(*R.pool_faulty(fault, R.features(geom, feat)["y"][:, :, :R.CHANNELS], w, K, T, mode))
    print(f"\n{fault}: gate {g:.1e} (e32 {e32:.1e})  err_mean {em:.1e} ({em / g:.0f} x)  err_std {es:.1e} ({es / g:.0f} x)")
    if fault in ("biased_denominator", "one_pass"):            # the mean is computed as before
        assert em <= g and not es <= g, (em, es, g)
    else:                                                      # (NaN, a std lost altogether, is beyond any gate)
        assert not em <= g and not es <= g, (em, es, g)
