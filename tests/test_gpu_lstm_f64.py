"""The LSTM recurrence kernels against the float64 restatement of tests/lstm_ref.py where their gates saturate
("Accuracy of the recurrence").

Kernels: every shipped recurrence — ``valu`` (k_lstm.hip, ``dz_k_lstm``) and the matrix-core variants 0, 3, 4
(k_lstm_mfma.hip, ``dz_k_lstm_mfma``; both gx column orders where a variant takes both), variants 1 / 2 in the
experiments build — each through its f32 output AND through ``dz_k_lstm_planes`` (kb-major f16 planes,
re-assembled as ``hi + lo / 2048``).  Every output buffer is pre-filled with NaN (planes: 0x7e00) and carries guard
rows behind row B * T: no NaN inside, guard untouched.

Regimes (tests/lstm_ref.py ``make_case``; tests/test_lstm_ref_host.py asserts on the CPU that float32 arithmetic alone
stays within 1e-5 of the reference in each of them): benign, saturated (x8, x32), overflow (gates forced to +-100 ..
+-1e30), integrator (|c| up to T), tiny, zero.

Tolerance, one rule for all kernels: max |h - bilstm_f64| <= max(2e-5, 4 e32), with 2e-5 the figure of
test_gpu_kernels.py::test_lstm_recurrence and e32 the error of float32 ``nn.LSTM`` on the CPU on the same case (the
factor 4: 22 mantissa bits of the f16x3 operands against float32's 24); tiny regime 2^-19; zero regime exactly 0;
planes against the same kernel's f32 output 2^-21 max(1, |h|max).

NaN / Inf inputs are out of scope (the model flags such rows before the LSTM).
"""
import sys
from pathlib import Path

import pytest
import torch

from diart_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lstm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3                      # rows behind B * T in every output buffer
SEG_MAX, SEG_MEAN = 1e-4, 3e-5     # the project's segmentation gates (tests/test_gpu_parity_r2.py), unchanged
F16_NAN = 0x7E00


def _ctx(dev):
    return _lib.context(dev.index or 0)


def _skip_unless_built(kernel):
    if kernel[:5] in ("mfma1", "mfma2") and not _lib.experiments():
        pytest.skip("matrix-core recurrence variants 1 / 2 exist in the experiments build only")


def _has_planes_entry(kernel):
    """dz_k_lstm_planes reads gx in PyTorch column order for variants 0..2 and unit-major for 3 / 4"""
    return kernel == "valu" or (int(kernel[4]) >= 3) == kernel.endswith("_um")


def _launch(gpu, kernel, gx, whh, B, T, out):
    """one launch into a fresh NaN-filled buffer with guard rows -> (h (B,T,256) on the CPU: float32 for out == "f32",
    float64 hi + lo / 2048 for "planes"; the raw buffer on the CPU).  Asserts the guard and the absence of NaN."""
    dgx, dw, um, variant = R.kernel_operands(kernel, gx, whh)
    dgx, dw = dgx.to(gpu), dw.to(gpu)
    lib, rows = _lib.load(), B * T + GUARD
    if out == "f32":
        buf = torch.full((rows, 256), float("nan"), device=gpu)
        if kernel == "valu":
            _lib.check(lib.dz_k_lstm(_ctx(gpu), dgx.data_ptr(), dw.data_ptr(), buf.data_ptr(), B, T, None))
        else:
            _lib.check(lib.dz_k_lstm_mfma(_ctx(gpu), dgx.data_ptr(), dw.data_ptr(), buf.data_ptr(), B, T, um, variant, None))
        torch.cuda.synchronize()
        raw = buf.cpu()
        assert torch.isnan(raw[B * T:]).all(), f"{kernel}: wrote behind row B * T"
        h = raw[:B * T].view(B, T, 256)
        assert not torch.isnan(h).any(), f"{kernel}: NaN in (or rows missing from) the f32 output"
        return h, raw
    assert _has_planes_entry(kernel)
    buf = torch.full((2, rows * 256), F16_NAN, dtype=torch.int16, device=gpu)
    if kernel == "valu":
        _lib.check(lib.dz_k_lstm_planes(_ctx(gpu), dgx.data_ptr(), dw.data_ptr(), None, 0, buf.data_ptr(), rows * 256, B, T, None))
    else:
        _lib.check(lib.dz_k_lstm_planes(_ctx(gpu), dgx.data_ptr(), None, dw.data_ptr(), variant, buf.data_ptr(), rows * 256, B, T, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    from diart_amd.weights import from_kb
    p = from_kb(raw, rows, 256)                                   # (2, rows, 256)
    assert (p[:, B * T:] == F16_NAN).all(), f"{kernel}: wrote behind row B * T of a plane"
    f = p[:, :B * T].view(torch.float16)
    assert not torch.isnan(f).any(), f"{kernel}: NaN in (or rows missing from) the planes"
    return (f[0].double() + f[1].double() / 2048.0).view(B, T, 256), raw


# --------------------------------------------------------------------------- regimes x shapes x kernels
SHAPES = [(regime, B, 293) for regime in R.REGIMES for B in (17, 64)]
SHAPES += [("benign", 17, T) for T in (1, 2, 3, 4, 5, 6, 7, 8, 11, 589)]              # every T mod 4, the 10 s geometry
SHAPES += [("benign", B, 43) for B in (1, 15, 16, 31, 33, 65, 130)]                   # around 16 chains per workgroup
SHAPES += [(regime, 17, T) for regime in ("overflow", "integrator") for T in (7, 11)]  # T mod 4 == 3
# the case is the outer loop: lstm_ref.case keeps its reference for all kernels
CASES = [pytest.param(regime, B, T, kernel, id=f"{regime}-B{B}-T{T}-{kernel}") for regime, B, T in SHAPES for kernel in R.KERNELS]


def tolerance(regime, e32):
    if regime == "tiny":
        # 2e-5 is vacuous at |h| ~ 1e-3.  8 ulp(1) = 2^-20 per step on c from the cancelling 2 rcp(1 + exp2) - 1 forms,
        # times the geometric factor 2 of a forget gate at 1/2
        return 2.0 ** -19
    return max(2e-5, 4.0 * e32)


@pytest.mark.parametrize("regime,B,T,kernel", CASES)
def test_recurrence_against_float64(gpu, regime, B, T, kernel):
    _skip_unless_built(kernel)
    gx, whh, ref, e32 = R.case(regime, B, T)
    assert e32 <= R.E32_CAP, (regime, B, T, e32)              # (asserted at (17, 293) on the CPU; holds at every shape)
    tol = tolerance(regime, e32)
    h, _ = _launch(gpu, kernel, gx, whh, B, T, "f32")
    err = (h.double() - ref).abs().max().item()
    perr = derr = float("nan")
    hp = None
    if _has_planes_entry(kernel):
        hp, _ = _launch(gpu, kernel, gx, whh, B, T, "planes")
        perr = (hp - ref).abs().max().item()
        derr = (hp - h.double()).abs().max().item()
    # (variants 0..2 with unit-major gx have no planes entry point: their planes half runs under the gate-major name)
    planes = f"planes_err={perr:.3e} planes_vs_f32={derr:.3e} " if hp is not None else ""
    print(f"LSTM_F64 regime={regime} B={B} T={T} kernel={kernel} err={err:.3e} {planes}e32={e32:.3e} tol={tol:.3e}")
    if regime == "zero":
        assert (h == 0).all() and (hp is None or (hp == 0).all())
    assert err <= tol, (err, tol)
    if hp is not None:
        assert derr <= 2.0 ** -21 * max(1.0, h.abs().max().item()), derr
        assert perr <= tol, (perr, tol)


# --------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("kernel", ["valu", "mfma0", "mfma0_um", "mfma3_um", "mfma4_um"])
def test_a_saturated_chain_does_not_disturb_its_workgroup(gpu, kernel):
    """include/diart_amd.h: rows never touch each other.  B = 32 benign chains; chains 5 and 20 (one per workgroup of 16)
    replaced by overflow-regime rows: the other 30 chains keep every bit, the two match the reference."""
    B, T = 32, 50
    gx, whh = R.make_case("benign", B, T)
    gx2 = gx.clone()
    for chain in (5, 20):
        R.force_overflow(gx2, chain, shift=chain)
    outs = ["f32"] + (["planes"] if _has_planes_entry(kernel) else [])
    ref2 = R.bilstm_f64(gx2, whh)
    tol = tolerance("overflow", R.e32_of(gx2, whh, ref2))
    others = [b for b in range(B) if b not in (5, 20)]
    for out in outs:
        h1, _ = _launch(gpu, kernel, gx, whh, B, T, out)
        h2, _ = _launch(gpu, kernel, gx2, whh, B, T, out)
        assert torch.equal(h1[others], h2[others]), (kernel, out)
        assert not torch.equal(h1[5], h2[5]) and not torch.equal(h1[20], h2[20])
        err = (h2.double() - ref2).abs().max().item()
        print(f"LSTM_ISOLATION kernel={kernel} out={out} err={err:.3e} tol={tol:.3e}")
        assert err <= tol, (kernel, out, err)


# --------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("regime", ["benign", "saturated8", "saturated32"])
def test_two_launches_give_the_same_bits(gpu, regime, kernel):
    """The pipelined kernel double-buffers h in LDS behind two barriers per step: a race shows as run-to-run bit noise
    far below any tolerance.  Two launches into fresh buffers, f32 and planes (guard rows and all)."""
    _skip_unless_built(kernel)
    B, T = 64, 293
    gx, whh = R.make_case(regime, B, T)
    for out in ["f32"] + (["planes"] if _has_planes_entry(kernel) else []):
        _, raw1 = _launch(gpu, kernel, gx, whh, B, T, out)
        _, raw2 = _launch(gpu, kernel, gx, whh, B, T, out)
        a, b = (raw1.view(torch.int32), raw2.view(torch.int32)) if out == "f32" else (raw1, raw2)
        assert torch.equal(a, b), (kernel, out)


# --------------------------------------------------------------------------- the stack through the model
@pytest.fixture(scope="module")
def saturated_stack():
    sd, audio = R.saturating_segmentation_state(), R.stack_windows()
    return sd, audio, R.stack_reference_f64(sd, audio), R.oracle_segmentation(sd, audio)


@pytest.mark.parametrize("recurrence", ["valu", "0", "3", "4"])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_saturated_stack_through_the_model(gpu, saturated_stack, precision, recurrence, monkeypatch):
    """All four layers through HipSegmentation — the x-projection epilogue that emits unit-major (variant 4: pre-scaled)
    gx, layers 1..3 reading the recurrence's own planes — with a first layer whose gates saturate
    (lstm_ref.saturating_segmentation_state; conditioning asserted in test_lstm_ref_host.py), against the network with
    its LSTM stack and head restated in float64 on the oracle's SincNet output (lstm_ref.stack_reference_f64).  The
    project's own gates.  (Exact f32 has one recurrence kernel, "valu": precision="f32" runs it whatever is asked.)"""
    from diart_amd import models as M
    sd, audio, ref, o32 = saturated_stack
    monkeypatch.delenv("DZ_ENGINE", raising=False)
    seg = M.HipSegmentation(sd, max_batch=16, precision=precision, recurrence=recurrence).to(gpu)
    got = seg(audio[:, None, :].to(gpu)).cpu()
    assert not torch.isnan(got).any()
    d = (got.double() - ref).abs()
    print(f"LSTM_STACK precision={precision} recurrence={recurrence} max={d.max().item():.3e} mean={d.mean().item():.3e} "
          f"vs_float32_oracle={(got - o32).abs().max().item():.3e}")
    assert d.max().item() < SEG_MAX and d.mean().item() < SEG_MEAN, (precision, recurrence, d.max().item(), d.mean().item())
