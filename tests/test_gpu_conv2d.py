"""k_conv2d.hip (WeSpeaker ResNet34's 3x3 / 1x1 convolutions) on its own, through dz_k_conv2d, against float64
F.conv2d in both arithmetic modes: split-f16 (tiles 128 x 32 / 64 / 128) and exact f32 (96 x BN, BN = 32 / 64 / 128).

Cases cover Cout x (taps, stride) x epilogue x Cin pairwise (27 cases), each on an output geometry B x Fo x To whose
M = B Fo To lands on the residues 0, 1 and -1 of both tile heights (M mod 384 in {0, 1, 383}), odd and even input
sizes, heights and widths 1 - 3, tiles that straddle batch rows; then the network's own layer geometries at 2 s and
at the shortest length the API accepts.

Gate: per element |y - y64| / (sum |x w| + |b| + |r|), the measure of test_gpu_kernels.py's
test_split_gemm_dynamic_range, at about 3x the worst element measured on an MI355X over every case (f16x3 1.5e-7,
f32 3.0e-7: the exact-f32 path sums in another order, not more precisely).  Y is NaN-prefilled with slack past
M Cout: every element in range is written, the slack is not."""
import math

import pytest
import torch

import wespeaker_ref as R
from diart_amd import _lib
from diart_amd.weights import split_f16, wsp_conv_matrix

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")
GATE = {"f16x3": 4.5e-7, "f32": 9e-7}
EPI = {"b": (False, False), "br": (False, True), "bR": (True, False), "bRr": (True, True)}     # (residual, relu)

# (Cout, (taps, stride), epilogue, Cin): every pair of values of two dimensions occurs
PAIRWISE = [
    (32, (9, 1), "b", 32), (32, (9, 2), "br", 64), (64, (9, 2), "bR", 32), (32, (1, 2), "bR", 128),
    (64, (9, 1), "bRr", 64), (128, (1, 2), "br", 32), (32, (1, 1), "bRr", 256), (64, (1, 1), "b", 128),
    (128, (1, 1), "bR", 64), (128, (9, 2), "bRr", 128), (256, (1, 2), "b", 64), (256, (9, 1), "br", 128),
    (512, (9, 1), "bR", 256), (512, (9, 2), "b", 512), (256, (1, 1), "bRr", 32), (64, (1, 2), "br", 256),
    (512, (1, 2), "bRr", 512), (512, (1, 1), "br", 512), (128, (9, 1), "b", 256), (256, (9, 2), "bR", 256),
    (32, (9, 1), "bR", 512), (512, (9, 1), "b", 32), (64, (9, 1), "b", 512), (512, (9, 1), "b", 64),
    (128, (9, 1), "b", 512), (512, (9, 1), "b", 128), (256, (9, 1), "b", 512),
]
# output geometries (B, Fo, To): M = 1, 383, 384, 385, 767, 768, 1537, 18, 12 (mod 384: 1, -1, 0, 1, -1, 0, 1)
GEOMS = [(1, 1, 1), (1, 1, 383), (3, 8, 16), (5, 7, 11), (13, 1, 59), (2, 12, 32), (1, 29, 53), (3, 2, 3), (2, 3, 2)]
FLOP_BUDGET = 6e8               # M Cout K of one case: the float64 reference stays well under a second


def _cases():
    out, g = [], 0
    for i, (cout, (taps, stride), epi, cin) in enumerate(PAIRWISE):
        while True:               # the next geometry in turn that the budget allows (M = 1 always does)
            B, Fo, To = GEOMS[g % len(GEOMS)]
            g += 1
            if B * Fo * To * cout * taps * cin <= FLOP_BUDGET:
                break
        # input sizes: stride 2 alternates odd / even heights and widths for the same output
        Fi = Fo if stride == 1 else 2 * Fo - (i % 2)
        Ti = To if stride == 1 else 2 * To - ((i // 2) % 2)
        out.append((B, Fi, Ti, cin, cout, taps, stride, epi))
    # the network's convolutions: 2 s (T = 198 -> 99 -> 50 -> 25) and 1680 samples (T = 9 -> 5 -> 3 -> 2)
    out += [(1, 80, 198, 32, 32, 9, 1, "bRr"), (1, 80, 198, 32, 64, 9, 2, "br"), (1, 80, 198, 32, 64, 1, 2, "b"),
            (1, 40, 99, 64, 64, 9, 1, "bRr"), (1, 40, 99, 64, 128, 9, 2, "br"), (1, 20, 50, 128, 256, 1, 2, "b"),
            (2, 10, 25, 256, 256, 9, 1, "bRr"), (2, 80, 9, 32, 32, 9, 1, "bRr"), (3, 40, 5, 64, 128, 9, 2, "br"),
            (3, 20, 3, 128, 256, 1, 2, "b"), (5, 10, 2, 256, 256, 9, 1, "bRr")]
    return out


CASES = _cases()
_REF = {}


def _ids(c):
    B, Fi, Ti, cin, cout, taps, stride, epi = c
    return f"B{B}-{Fi}x{Ti}-{cin}to{cout}-k{taps}s{stride}-{epi}"


def _operands(case):
    """Distinct activations per (f, t, c) (non-negative, as after a ReLU, in every other case), weights at folded-BN
    scale, bias, residual; the test's own weight matrix, checked against the product's packing."""
    B, Fi, Ti, cin, cout, taps, stride, epi = case
    g = torch.Generator().manual_seed(B * 7919 + Fi * 131 + Ti * 17 + cin + cout + taps + stride)
    n = B * Fi * Ti * cin
    x = 0.25 + (torch.randperm(n, generator=g).double() + 0.5) / n          # distinct in f32: spacing > 1 ulp
    if CASES.index(case) % 2:
        x = x * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    x = x.float().view(B, Fi, Ti, cin)
    k = 3 if taps == 9 else 1
    w4 = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * taps))
    w4 = w4 * (0.8 + 0.4 * torch.rand(cout, 1, 1, 1, generator=g)) / torch.sqrt(0.5 + torch.rand(cout, 1, 1, 1, generator=g))
    b = 0.1 * torch.randn(cout, generator=g)
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    r = torch.randn(B, Fo, To, cout, generator=g) if EPI[epi][0] else None
    m = R.conv_matrix(w4)
    return x, w4, m, b, r


def _reference(case):
    if case not in _REF:
        x, w4, m, b, r = _operands(case)
        stride, relu = case[6], EPI[case[7]][1]
        _REF[case] = R.conv_ref(x, w4, b, r, relu, stride)
    return _REF[case]


def run_conv2d(gpu, x, m, b, r, *, taps, stride, relu, precision, cout, slack=None):
    """One dz_k_conv2d call -> (return code, Y with its slack (flat, on the host))."""
    B, Fi, Ti, cin = x.shape
    Fo, To = (Fi - 1) // max(stride, 1) + 1, (Ti - 1) // max(stride, 1) + 1
    M = B * Fo * To
    slack = 128 * max(cout, 1) + 64 if slack is None else slack
    Y = torch.full((max(M * cout, 0) + slack,), float("nan"), device=gpu)
    dx, dm, db = x.contiguous().to(gpu), m.float().contiguous().to(gpu), b.float().to(gpu)
    dr = r.float().contiguous().to(gpu) if r is not None else None
    dsp = split_f16(m.float()).to(gpu) if precision == "f16x3" else None
    lib = _lib.load()
    rc = lib.dz_k_conv2d(_lib.context(gpu.index or 0), dx.data_ptr(), dm.data_ptr(),
                         dsp.data_ptr() if dsp is not None else None, db.data_ptr(),
                         dr.data_ptr() if dr is not None else None, Y.data_ptr(), B, Fi, Ti, cin, cout, taps, stride,
                         int(relu), None)
    torch.cuda.synchronize(gpu)
    return rc, Y.cpu()


def element_error(y, want, scale):
    return ((y.double() - want).abs() / scale).max().item()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_conv2d_against_float64(gpu, case, precision):
    B, Fi, Ti, cin, cout, taps, stride, epi = case
    x, w4, m, b, r = _operands(case)
    assert torch.equal(m, wsp_conv_matrix(w4))                     # the test's matrix is the product's packing
    if precision == "f16x3":
        assert torch.equal(R.split_planes(m), split_f16(m))        # and so are its split planes
    want, scale = _reference(case)
    _lib.range_check(gpu.index or 0)                               # (a clean flag to start from)
    rc, Y = run_conv2d(gpu, x, m, b, r, taps=taps, stride=stride, relu=EPI[epi][1], precision=precision, cout=cout)
    _lib.check(rc, "dz_k_conv2d")
    _lib.range_check(gpu.index or 0)                               # in range: the flag stays clear
    n = want.numel()
    assert torch.isfinite(Y[:n]).all(), f"{int((~torch.isfinite(Y[:n])).sum())} elements not written"
    assert torch.isnan(Y[n:]).all(), "a store past M Cout"
    err = element_error(Y[:n].view(want.shape), want, scale)
    print(f"CONV2D {precision} {_ids(case)} M={want.shape[0] * want.shape[1] * want.shape[2]} err={err:.3e}")
    assert err <= GATE[precision], err


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conv2d_mixed_magnitudes_inside_one_row(gpu, precision):
    """Activations from 1e-7 to 1e4 mixed inside every im2col row stay f32-grade in both modes; the flag stays
    clear (nothing passes 65504)."""
    g = torch.Generator().manual_seed(3)
    B, Fi, Ti, cin, cout = 2, 9, 13, 64, 128
    mags = torch.tensor([1e-7, 1e-5, 1e-3, 1.0, 30.0, 1e4])
    x = torch.randn(B, Fi, Ti, cin, generator=g) * mags[torch.randint(0, len(mags), (B, Fi, Ti, cin), generator=g)]
    w4 = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = torch.zeros(cout)
    m = R.conv_matrix(w4)
    want, scale = R.conv_ref(x, w4, b, None, False, 1)
    _lib.range_check(gpu.index or 0)
    rc, Y = run_conv2d(gpu, x, m, b, None, taps=9, stride=1, relu=False, precision=precision, cout=cout)
    _lib.check(rc, "dz_k_conv2d")
    _lib.range_check(gpu.index or 0)
    err = element_error(Y[:want.numel()].view(want.shape), want, scale)
    print(f"CONV2D-MIXED {precision} err={err:.3e}")
    assert err < 1e-6, err        # test_split_gemm_dynamic_range's gate


def test_conv2d_range_flag(gpu):
    """One activation above 65504 is clamped by the split-f16 path and raises the context's range flag; the same call
    in exact f32 computes it and leaves the flag clear.  (Its gate is 3x the 1.19e-6 measured: where the 1e5 operand
    dominates sum |x w|, every later addition rounds at that term's ulp.)"""
    g = torch.Generator().manual_seed(8)
    B, Fi, Ti, cin, cout = 1, 6, 7, 32, 64
    x = torch.rand(B, Fi, Ti, cin, generator=g)
    x[0, 3, 4, 5] = 1e5
    w4 = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = torch.zeros(cout)
    m = R.conv_matrix(w4)
    _lib.range_check(gpu.index or 0)
    rc, _ = run_conv2d(gpu, x, m, b, None, taps=9, stride=1, relu=False, precision="f16x3", cout=cout)
    _lib.check(rc, "dz_k_conv2d")
    with pytest.raises(_lib.DiartAmdError, match="65504"):
        _lib.range_check(gpu.index or 0)
    _lib.range_check(gpu.index or 0)                               # (reset by the check above)
    want, scale = R.conv_ref(x, w4, b, None, False, 1)
    rc, Y = run_conv2d(gpu, x, m, b, None, taps=9, stride=1, relu=False, precision="f32", cout=cout)
    _lib.check(rc, "dz_k_conv2d")
    _lib.range_check(gpu.index or 0)
    err = element_error(Y[:want.numel()].view(want.shape), want, scale)
    print(f"CONV2D-RANGE f32 err={err:.3e}")
    assert err <= 3.6e-6, err


@pytest.mark.parametrize("what,args,msg", [
    ("Cin 48", dict(cin=48), "Cin 48"), ("Cout 96", dict(cout=96), "Cout 96"), ("stride 3", dict(stride=3), "stride 3"),
    ("taps 4", dict(taps=4), "4 taps"), ("stride 0", dict(stride=0), "stride 0"), ("height 0", dict(fi=0), "empty"),
    ("batch 0", dict(batch=0), "empty")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_conv2d_refusals(gpu, precision, what, args, msg):
    """What the launcher refuses comes back as an error with a message, and nothing is written."""
    a = dict(batch=2, fi=5, ti=6, cin=64, cout=64, taps=9, stride=1)
    a.update(args)
    x = torch.rand(2 * 5 * 6 * 64).to(gpu)
    w = torch.rand(512 * 9 * 64).to(gpu)
    ws = torch.zeros(2 * 512 * 9 * 64, dtype=torch.int16).to(gpu)
    b = torch.zeros(512).to(gpu)
    Y = torch.full((2 * 5 * 6 * 512 + 64,), float("nan"), device=gpu)
    lib = _lib.load()
    rc = lib.dz_k_conv2d(_lib.context(gpu.index or 0), x.data_ptr(), w.data_ptr(),
                         ws.data_ptr() if precision == "f16x3" else None, b.data_ptr(), None, Y.data_ptr(),
                         a["batch"], a["fi"], a["ti"], a["cin"], a["cout"], a["taps"], a["stride"], 0, None)
    torch.cuda.synchronize(gpu)
    assert rc != 0, what
    assert msg in lib.dz_last_error().decode(), lib.dz_last_error()
    assert torch.isnan(Y.cpu()).all(), f"{what}: something was launched"
