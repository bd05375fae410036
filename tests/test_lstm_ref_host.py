"""The LSTM recurrence's host half ("Accuracy of the recurrence"): the float64 restatement of
tests/lstm_ref.py pinned to ``torch.nn.LSTM`` in float64, the conditioning of every input regime the GPU tests
(tests/test_gpu_lstm_f64.py) run — float32 arithmetic alone must stay within 1e-5 of the reference, or a tolerance
built on it means nothing — and the variant-4 operands of ``weights.py`` (column permutation, folded activation
scales), which no test saw without a GPU.  No GPU."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lstm_ref as R  # noqa: E402

H = R.H


# --------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("B,T", [(1, 1), (1, 7), (3, 1), (2, 2), (5, 40), (17, 64)])
def test_bilstm_f64_is_torch_lstm_in_float64(B, T):
    """weights copied into nn.LSTM(...).double(), gx = x W_ih^T + b_ih + b_hh: the loop and the module agree to 1e-12"""
    g = torch.Generator().manual_seed(B * 100 + T)
    I = 32
    lstm = torch.nn.LSTM(I, H, 1, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) * 0.25).float().double())   # float32 values: what a kernel gets
        x = torch.randn(B, T, I, generator=g).double()
        want, _ = lstm(x)
        gx = torch.cat([x @ lstm.weight_ih_l0.t() + lstm.bias_ih_l0 + lstm.bias_hh_l0,
                        x @ lstm.weight_ih_l0_reverse.t() + lstm.bias_ih_l0_reverse + lstm.bias_hh_l0_reverse], -1)
        whh = torch.stack([lstm.weight_hh_l0, lstm.weight_hh_l0_reverse])
    # (bilstm_f64 converts from whatever it is given: handing it float64 keeps gx unrounded, as the module sees it)
    got = R.bilstm_f64(gx, whh)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, T, 2 * H)
    assert (got - want).abs().max().item() <= 1e-12


def test_lstm_on_gx_feeds_the_given_projection():
    """the identity-W_ih module behind e32 computes the recurrence OF gx: in float64 it is the restatement"""
    gx, whh = R.make_case("saturated8", 3, 9)
    assert (R.lstm_on_gx(gx, whh, torch.float64) - R.bilstm_f64(gx, whh)).abs().max().item() <= 1e-12


def test_return_pre_gives_the_gate_pre_activations():
    gx, whh = R.make_case("benign", 2, 5)
    h, pre = R.bilstm_f64(gx, whh, return_pre=True)
    assert torch.equal(pre[:, 0, :4 * H], gx[:, 0, :4 * H].double())          # h_{-1} = 0: the first forward step is gx
    assert torch.equal(pre[:, -1, 4 * H:], gx[:, -1, 4 * H:].double())        # ... and the first backward step
    want = gx[:, 1, :4 * H].double() + h[:, 0, :H] @ whh[0].double().t()
    assert (pre[:, 1, :4 * H] - want).abs().max().item() <= 1e-14


# --------------------------------------------------------------------------- the regimes
@pytest.mark.parametrize("regime", R.REGIMES)
def test_every_regime_is_well_conditioned_in_float32(regime):
    """e32 = max |nn.LSTM float32 on the CPU - bilstm_f64| at (B, T) = (17, 293) stays within 1e-5 (the GPU tolerance is
    max(2e-5, 4 e32)), W_hh stays within U(+-0.25), and the regime reaches what its name says."""
    gx, whh, ref, e32 = R.case(regime, 17, 293)
    print(f"LSTM_E32 regime={regime} B=17 T=293 e32={e32:.3e}")
    assert whh.abs().max().item() <= R.WHH_BOUND
    assert torch.isfinite(ref).all()
    assert e32 <= R.E32_CAP, (regime, e32)
    _, pre = R.bilstm_f64(gx, whh, return_pre=True)
    big = pre.abs().max().item()
    if regime == "benign":
        assert big < 8
    elif regime == "saturated8":
        assert big > 30 and (pre.abs() > 8).float().mean().item() > 0.25
    elif regime == "saturated32":
        assert big > 100                                     # exp beyond float32 (|x| > 88.7)
    elif regime == "overflow":
        assert big >= 1e30
        for mag in R.OVERFLOW_MAGNITUDES:                    # every magnitude in both signs
            assert (gx == mag).any() and (gx == -mag).any()
    elif regime == "integrator":
        # |c| = atanh-free restatement: c_t = sum of tanh(g) with i = f = 1 to 1e-8; the walkers pass 22, the ramps reach T
        # (at this shape, in both directions; the T = 7 / 11 integrator shapes of the GPU file are too short
        # for a walker to come near the clamp: they run the ramps through the T mod 4 == 3 epilogue)
        for d in range(2):
            g = torch.tanh(pre.view(17, 293, 2, 4, H)[:, :, d, 2, :])
            c = (g.flip(1) if d else g).cumsum(1)
            assert c[:, :, :H // 2].abs().max().item() > 292 and c[:, :, H // 2:].abs().max().item() > 22.2
            assert (c[:, :, :H // 2].amax() > 0) and (c[:, :, :H // 2].amin() < 0)
    elif regime == "tiny":
        assert 1e-6 < ref.abs().max().item() < 5e-3
    elif regime == "zero":
        assert (ref == 0).all() and e32 == 0.0


def test_overflow_patterns_cover_each_gate_alone_in_each_sign_and_all_four():
    pats = set(R.OVERFLOW_PATTERNS)
    for gate in range(4):
        for s in (1, -1):
            assert tuple(s if k == gate else 0 for k in range(4)) in pats
    assert (1, 1, 1, 1) in pats and (-1, -1, -1, -1) in pats
    units = [(37 * k + 11) % H for k in range(len(R.OVERFLOW_PATTERNS) * len(R.OVERFLOW_MAGNITUDES))]
    assert len(set(units)) == len(units)                     # every (pattern, magnitude) on its own unit


# --------------------------------------------------------------------------- weights.py: the variant-4 operands
def _unsplit(p):
    h = p.view(torch.float16).double()
    return h[..., 0, :, :] + h[..., 1, :, :] / 2048.0


def test_lstm_k_order_is_the_documented_permutation():
    from diart_amd.weights import lstm_k_order
    order = lstm_k_order()
    assert sorted(order.tolist()) == list(range(H))
    for a in range(2):
        for p in range(32):
            for e in range(2):
                assert int(order[64 * a + 2 * p + e]) == 4 * p + 2 * a + e      # k' = 64a + 2p + e  <-  u = 4p + 2a + e


def test_lstm_whh_planes_variant_4_recovers_whh():
    """undo the split (hi + lo 2^-11), the column order and the gate scales: W_hh to 2^-21 of each row's maximum"""
    from diart_amd.weights import LSTM_GATE_SCALE, lstm_k_order, lstm_whh_planes
    g = torch.Generator().manual_seed(4)
    whh = (torch.rand(2, 4 * H, H, generator=g) * 2 - 1) * 0.25
    planes = lstm_whh_planes(whh, 4)
    assert planes.dtype == torch.int16 and tuple(planes.shape) == (2, 2, 4 * H, H)
    w = _unsplit(planes)                                              # [dir][512][k']
    back = torch.empty_like(w)
    back[:, :, lstm_k_order()] = w                                    # column k' holds unit order[k']
    back = back.view(2, 4, H, H) / torch.tensor(LSTM_GATE_SCALE, dtype=torch.float64).view(1, 4, 1, 1)
    err = (back.view(2, 4 * H, H) - whh.double()).abs()
    bound = 2.0 ** -21 * whh.double().abs().amax(dim=2, keepdim=True)
    assert (err <= bound).all(), (err / bound).max().item()
    # a permutation that is wrong in ONE entry is seen here (what the GPU tests would show as garbage)
    bad = lstm_k_order().clone()
    bad[[5, 6]] = bad[[6, 5]]
    wrong = torch.empty_like(w)
    wrong[:, :, bad] = w
    wrong = wrong.view(2, 4, H, H) / torch.tensor(LSTM_GATE_SCALE, dtype=torch.float64).view(1, 4, 1, 1)
    assert not ((wrong.view(2, 4 * H, H) - whh.double()).abs() <= bound).all()


@pytest.mark.parametrize("variant", [0, 3])
def test_lstm_whh_planes_variants_0_and_3_are_split_f16_per_direction(variant):
    from diart_amd.weights import lstm_whh_planes, split_f16
    g = torch.Generator().manual_seed(5)
    whh = (torch.rand(2, 4 * H, H, generator=g) * 2 - 1) * 0.25
    planes = lstm_whh_planes(whh, variant)
    for d in range(2):
        assert torch.equal(planes[d], split_f16(whh[d]))
    assert (_unsplit(planes) - whh.double()).abs().max().item() <= 2.0 ** -21 * 0.25


def test_lstm_scale_gx_agrees_with_the_gate_scales_in_both_row_orders():
    from diart_amd.weights import LSTM_GATE_SCALE, lstm_scale_gx
    assert LSTM_GATE_SCALE == (-1.44269504088896341, -1.44269504088896341, -2.88539008177792681, -1.44269504088896341)
    g = torch.Generator().manual_seed(6)
    sc = torch.tensor(LSTM_GATE_SCALE, dtype=torch.float64)
    for shape in ((8 * H,), (8 * H, 60)):
        t = torch.randn(shape, generator=g)
        rows = torch.arange(8 * H)
        for um, gate in ((True, rows % 4), (False, (rows % (4 * H)) // H)):
            want = (t.double() * sc[gate].view((-1,) + (1,) * (t.dim() - 1))).float()
            assert torch.equal(lstm_scale_gx(t, unit_major=um), want)
    # the two row orders are the same operand: scaling commutes with the re-ordering the model applies
    t = torch.randn(8 * H, 60, generator=g)
    um = lambda v: v.reshape(2, 4, H, 60).transpose(1, 2).reshape(8 * H, 60)
    assert torch.equal(lstm_scale_gx(um(t), True), um(lstm_scale_gx(t, False)))
    # ... and prescale_um of the test operands is that scaling applied to gx columns
    gx = torch.randn(2, 3, 8 * H, generator=g)
    assert torch.equal(R.prescale_um(R.unit_major(gx))[1, 2], lstm_scale_gx(R.unit_major(gx)[1, 2], True))


def test_unit_major_is_the_models_row_order():
    gx = torch.arange(8 * H, dtype=torch.float32).view(1, 1, 8 * H)
    um = R.unit_major(gx)[0, 0]
    for d, gate, unit in ((0, 0, 0), (0, 2, 5), (1, 3, 127), (1, 1, 64)):
        assert um[d * 512 + unit * 4 + gate].item() == d * 512 + gate * H + unit


# --------------------------------------------------------------------------- the stack through the model
SEG_MAX = 1e-4                                               # the segmentation gate of tests/test_gpu_parity_r2.py


def _stack_drift(sd, audio):
    """(max |float32 oracle - the same network with its LSTM stack and head in float64|, layer-0 fraction beyond |8|)"""
    ref, frac = R.stack_reference_f64(sd, audio, return_frac=True)
    got = R.oracle_segmentation(sd, audio)
    assert ref.dtype == torch.float64 and got.dtype == torch.float32
    assert (ref.max() - ref.min()).item() > 0.5              # an output that still moves
    return (got.double() - ref).abs().max().item(), frac


def test_saturating_state_changes_what_it_says():
    from diart_amd.synth import synth_segmentation_state
    base, sd = synth_segmentation_state(), R.saturating_segmentation_state()
    assert (R.STACK_FACTOR, R.STACK_FORGET_BIAS, R.STACK_LAYERS) == (8.0, 3.0, (0,))
    for k in base:
        if k.startswith("lstm.weight_ih_l0"):
            assert torch.equal(sd[k], base[k] * 8.0)
        elif k.startswith("lstm.bias_ih_l0"):
            assert torch.equal(sd[k][H:2 * H], base[k][H:2 * H] + 3.0)
            assert torch.equal(sd[k][:H], base[k][:H]) and torch.equal(sd[k][2 * H:], base[k][2 * H:])
        else:
            assert torch.equal(sd[k], base[k]), k            # W_hh, the upper layers, SincNet and the head: untouched


def test_saturating_stack_is_saturated_and_well_conditioned():
    """The state and the 16 windows tests/test_gpu_lstm_f64.py drives through all four layers: the float32 oracle is within
    SEG_MAX / 10 of the float64 reference (measured 2.5e-6), and at least 5 % of the layer-0 gate pre-activations exceed
    |8| (measured 19 %)."""
    drift, frac = _stack_drift(R.saturating_segmentation_state(), R.stack_windows())
    print(f"LSTM_STACK layer 0 x8 +3: float32 oracle vs float64 stack {drift:.3e}; layer-0 |pre| > 8: {frac:.3f}")
    assert frac >= 0.05, frac
    assert drift <= SEG_MAX / 10, drift


def test_modifying_every_layer_is_not_a_usable_regime():
    """Why only layer 0 is modified.  W_ih x8 and forget bias +3 in ALL four layers: the same saturation of layer 0, but
    the float32 oracle is already further than SEG_MAX / 10 from the float64 stack (measured 6.8e-5 on these 4 windows,
    1.1e-4 on 16; x4 +3: 5.3e-5 with 4.8 % of the gates beyond |8|) — a SEG_MAX gate on it would measure float32
    conditioning, not a kernel.  The unmodified state, for scale: 1.7e-6."""
    audio = R.stack_windows(4)
    drift, frac = _stack_drift(R.saturating_segmentation_state(layers=(0, 1, 2, 3)), audio)
    print(f"LSTM_STACK every layer x8 +3: float32 oracle vs float64 stack {drift:.3e}; layer-0 |pre| > 8: {frac:.3f}")
    assert frac >= 0.05 and drift > SEG_MAX / 10, (drift, frac)
    base, _ = _stack_drift(R.saturating_segmentation_state(1.0, 0.0), audio)
    assert base <= SEG_MAX / 10, base
