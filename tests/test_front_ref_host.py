"""tests/front_ref.py on the CPU: the float32 floor of every stage-0 cell the GPU test gates, that the measure
catches what the old one let through, and the restatement against torch's own layers ("Accuracy of
the front end").  No GPU, no library."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import front_ref as R  # noqa: E402

FLOOR_BOUND = 2e-5          # no cell's float32 error may leave this: beyond it the CASE is wrong, not a kernel
OLD_GATE = 2e-5             # test_gpu_kernels.py::test_sinc_conv0*: _rel(got, ref) < 2e-5


def test_float32_floor_of_every_cell():
    """e32 = cond_err of the float32 restatement, per (bank, case, S) of tests/test_gpu_front_f64.py"""
    worst, den_min = {}, float("inf")
    for net, case, S in R.stage0_cells():
        _, _, den, e32 = R.stage0_ref(net, case, S)
        den_min = min(den_min, den.min().item())
        worst.setdefault((net, case), {})[S] = e32
    print(f"\nsmallest denominator of any cell: {den_min:.3g}")
    print(f"{'bank':4s} {'case':13s} " + " ".join(f"{S:>8d}" for S in R.STAGE0_S))
    for (net, case), row in worst.items():
        print(f"{net:4s} {case:13s} " + " ".join(f"{row[S]:8.1e}" if S in row else " " * 8 for S in R.STAGE0_S))
    assert den_min > 0.0                       # |beta| * sum |filt| at the least: the division is safe
    bad = {k: v for k, v in worst.items() if max(v.values()) > FLOOR_BOUND}
    assert not bad, bad


def _defects(net, case, S):
    """-> (gate, [new, old] of "channels 64..79 lost the samples' low plane", quietest channel, [new, old] of "the
    quietest channel's bank row lost its low plane"); float64 arithmetic around the one rounded operand"""
    gamma, beta = R.AFFINE[net]
    x, ref, den, e32 = R.stage0_ref(net, case, S)
    xn, filt = R.normalise(x, gamma, beta), R.bank(net).double()
    hi = ref.clone()
    hi[:, 64:] = R.bank_pool(R.round_f16(xn), filt)[:, 64:]
    q = int(ref.pow(2).mean(2)[0].argmin())
    f2 = filt.clone()
    f2[q] = R.round_f16(f2[q])
    lo = ref.clone()
    lo[:, q] = R.bank_pool(xn, f2)[:, q]
    m = lambda got: (R.cond_err(got, ref, den).max().item(), R.old_rel(got, ref))
    return R.gate(e32), m(hi), q, m(lo)


def test_measure_has_teeth_on_the_light_wave_channels():
    """channels 64..79 (other waves, other arithmetic in the shipped kernel) computed from f16-rounded samples: beyond the
    GPU gate in every case but silence (2.6 x at the least, 20 .. 170 x outside the DC windows); the old measure of the same
    defect is printed beside it (1 .. 30 x its gate on these windows)"""
    missed_by_old = []
    for net in ("seg", "emb"):
        for S in (281, 2661, 80000):
            for case in R.ALL_CASES:
                if case == "silence" or (S == 80000 and case not in ("speech", "lowpass")):
                    continue
                g, (new, old), _, _ = _defects(net, case, S)
                print(f"{net} {S:6d} {case:13s} gate {g:.1e}  new {new:.1e} ({new / g:6.1f} x gate)  old {old:.1e}")
                assert new > g, (net, S, case, new, g)
                if old < OLD_GATE:
                    missed_by_old.append((net, S, case, old))
    print("passed the old gate:", missed_by_old)


# the cells of the quietest-channel demonstration: the segmentation bank at the three-tile length
TEETH_NET, TEETH_S = "seg", 2661


@pytest.mark.parametrize("case", ["lowpass", "tone", "click"])
def test_measure_has_teeth_on_the_quietest_channel(case):
    """the quietest channel's bank row rounded to f16: at least 10 x the GPU gate"""
    g, _, q, (new, old) = _defects(TEETH_NET, case, TEETH_S)
    print(f"\n{case}: channel {q}, gate {g:.1e}, new measure {new:.1e} ({new / g:.1f} x gate), old measure {old:.1e}")
    assert new >= 10.0 * g, (case, q, new, g)


@pytest.mark.parametrize("case", ["lowpass", "click"])
def test_old_measure_is_blind_on_the_quietest_channel(case):
    """... and the same defect stays under the old gate: the two cells where it sees nothing"""
    g, _, q, (new, old) = _defects(TEETH_NET, case, TEETH_S)
    assert old < OLD_GATE, (case, q, old)
    assert new >= 10.0 * g, (case, q, new, g)


# --------------------------------------------------------------------------- the restatement itself
def test_f64_restatement_against_torch_layers():
    x = torch.stack([R.make_case(c, 2663) for c in ("speech", "tone", "dc", "click")])
    for net in ("seg", "emb"):
        gamma, beta = R.AFFINE[net]
        filt = R.bank(net).double()
        mean, rstd = R.wave_stats(x)
        assert torch.allclose(mean, x.double().mean(1), rtol=0, atol=1e-15)
        assert torch.allclose(rstd, 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5), rtol=1e-13)
        xn = F.instance_norm(x.double()[:, None, :]) * gamma + beta
        want = F.max_pool1d(F.conv1d(xn, filt[:, None, :], stride=10).abs(), 3, 3)
        y0 = R.stage0(x, R.bank(net), gamma, beta)
        assert y0.dtype == torch.float64 and y0.shape == (4, 80, R.geometry(2663)[1])
        assert (y0 - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        # partials -> finalize_norm -> stage 1 -> stage 2 against InstanceNorm1d(affine) -> LeakyReLU -> Conv1d -> MaxPool1d
        y, frames = y0, R.geometry(2663)[0]
        for i in (1, 2):
            w, b, g, bt = R.conv_weights(net, i)
            for tile in (96, 192):
                part = R.tile_partials(y, tile, frames)
                assert part.shape[1] == R.ntile(frames, tile)
                assert torch.allclose(part.sum(1)[..., 0], y.sum(2), rtol=1e-13, atol=1e-13)
                assert torch.allclose(part.sum(1)[..., 1], (y * y).sum(2), rtol=1e-13, atol=1e-13)
            sc, sh = R.finalize_norm(R.tile_partials(y, 96, frames), y.shape[2], g, bt)
            sc2, sh2 = R.norm_of(y, g, bt)
            assert torch.allclose(sc, sc2, rtol=1e-9) and torch.allclose(sh, sh2, rtol=1e-9, atol=1e-12)
            a = F.leaky_relu(F.instance_norm(y, weight=g.double(), bias=bt.double()), 0.01)
            want = F.max_pool1d(F.conv1d(a, w.double(), b.double()), 3, 3)
            frames = y.shape[2] - 4
            y = R.stage(y, sc, sh, w, b)
            assert y.shape == want.shape == (4, 60, frames // 3)
            assert (y - want).abs().max().item() <= 1e-9 * want.abs().max().item()
        ys = R.chain(x, net)
        assert torch.equal(ys[0], y0) and torch.equal(ys[2], y)


def test_f64_restatement_against_the_f32_reference_of_test_sinc_conv0():
    """the reference of test_gpu_kernels.py::test_sinc_conv0 (float32 F.instance_norm / F.conv1d / F.max_pool1d, its
    windows and affine pair) agrees with the float64 restatement to float32 round-off"""
    from diart_amd.synth import sliding_chunks, synth_stream
    filt = R.bank("seg")
    x = torch.from_numpy(sliding_chunks(synth_stream(5, 8.0))[:3].copy())
    gamma, beta = 1.3, -0.05
    xn = F.instance_norm(x[:, None, :]) * gamma + beta
    ref32 = F.max_pool1d(F.conv1d(xn, filt[:, None, :], stride=10).abs(), 3, 3)
    ref64 = R.stage0(x, filt, gamma, beta)
    assert ref32.shape == ref64.shape == (3, 80, 2658)
    assert R.old_rel(ref32, ref64) < 2e-6
    assert R.cond_err(ref32, ref64, R.stage0_den(x, filt, gamma, beta)).max().item() < 2e-6


def test_partial_measures_on_the_float32_restatement():
    """the two partial measures on the float32 restatement's own partials stay at the float32 floor in every case at the
    three-tile length — the sums of squares only in the exact form (den (|ref| + |got|)): its first-order form
    (2 den |ref|) is 0 / 0 on silence, where the odd filters' reference is ~1e-17 of what the channel resolves"""
    for net in ("seg", "emb"):
        gamma, beta = R.AFFINE[net]
        for case in R.ALL_CASES:
            x, ref, den, e32 = R.stage0_ref(net, case, 2661)
            y32 = R.stage0(x, R.bank(net), gamma, beta, R.F32)
            part = R.tile_partials(y32, 96, R.geometry(2661)[0], R.F32)
            e1, e2 = (v.max().item() for v in R.part_err(part, ref, den, y32))
            first = R.part_err(part, ref, den)[1].max().item()
            print(f"{net} {case:13s} e32 {e32:.1e}  sums {e1:.1e}  sums of squares {e2:.1e}  (first-order form {first:.1e})")
            assert e1 <= R.gate(e32) and e2 <= R.gate(e32), (net, case, e1, e2, e32)
            if case == "silence":
                assert first > 1.0
            else:
                assert abs(first - e2) <= 0.01 * e2 + 1e-12


def test_cases_are_fixed_and_shaped():
    for case in R.ALL_CASES:
        for S in (31, 281, 2663):
            a, b = R.make_case(case, S, 1), R.make_case(case, S, 1)
            assert a.dtype == torch.float32 and a.shape == (S,) and torch.equal(a, b) and torch.isfinite(a).all()
    assert R.make_case("silence", 100).abs().max() == 0
    assert (R.make_case("tail", 1000)[600:] == 0).all() and R.make_case("tail", 1000)[:600].abs().max() > 0
    dc = R.make_case("dc_large", 80000).double()
    assert abs(dc.mean().item() - 1.0) < 1e-4 and 5e-4 < dc.std().item() < 2e-3
    assert int((R.make_case("click", 2661) != 0).sum()) == 1
