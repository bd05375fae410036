"""The kernels the speechbrain ResNet adds, each on its own against float64: k_conv2d.hip's masked instances
(dz_k_conv2d_masked) and k_sb_resnet.hip's squeeze-excitation gate, apply and attention pooling kernels.

Masked conv2d: 3 rows on a 12 x 8 grid whose live steps are {1, 7, 12} and {2, 12, 7} — M = 288 (stride 1) or 72
(stride 2) is no multiple of a 128- or 96-row tile, tiles straddle rows, one row is wholly live — over Cin 32 / 64,
Cout 32 / 64 / 128 (every tile shape), taps 9 / 1, stride 1 / 2, both precisions.  The element gate is
tests/test_gpu_conv2d.py's (|y - y64| / (sum |x w| + |b| + |r|), 3x the 1.5e-7 / 3.0e-7 measured for the unmasked
instances, whose tiles and arithmetic these share).  Measured on an MI355X over every case here: f16x3 1.3e-7,
f32 2.3e-7.

The other kernels are gated by a worst-case forward error bound of their own float32 arithmetic (u = 2^-24, a sum of
n terms within (n + 1) u sum |terms|), evaluated in float64 per element: loose by the usual sqrt(n), and independent of
what the kernels return (measured: the gate within 1.4e-7 where the bound is 6e-5 .. 3e-4; mu within 1.1e-6, sg 4.2e-7)."""
import itertools
import math

import pytest
import torch

import wespeaker_ref as W
from diart_amd import _lib
from diart_amd.weights import split_f16, wsp_conv_matrix

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")
GATE = {"f16x3": 4.5e-7, "f32": 9e-7}
U = 2.0 ** -24
B, FI, TI = 3, 12, 8
EXTENTS = ((1, 7, 12), (2, 12, 7))
CASES = list(itertools.product((32, 64), (32, 64, 128), (9, 1), (1, 2)))       # (cin, cout, taps, stride)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def run_masked(gpu, x, m, b, r, ext, *, taps, stride, relu, precision, masked=True):
    """One dz_k_conv2d_masked (or dz_k_conv2d) call -> Y (batch, Fo, To, Cout) on the host, NaN where nothing was stored."""
    n, Fi, Ti, cin = x.shape
    cout = m.shape[0]
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    Y = torch.full((n * Fo * To * cout + 64,), float("nan"), device=gpu)
    dx, dm, db = x.contiguous().to(gpu), m.float().contiguous().to(gpu), b.float().to(gpu)
    dr = r.float().contiguous().to(gpu) if r is not None else None
    dsp = split_f16(m.float()).to(gpu) if precision == "f16x3" else None
    lib, ctx = _lib.load(), _lib.context(gpu.index or 0)
    if masked:
        de = torch.tensor(ext, dtype=torch.int32, device=gpu)
        rc = lib.dz_k_conv2d_masked(ctx, dx.data_ptr(), dm.data_ptr(), _ptr(dsp), db.data_ptr(), _ptr(dr), de.data_ptr(),
                                    Y.data_ptr(), n, Fi, Ti, cin, cout, taps, stride, int(relu), None)
    else:
        rc = lib.dz_k_conv2d(ctx, dx.data_ptr(), dm.data_ptr(), _ptr(dsp), db.data_ptr(), _ptr(dr), Y.data_ptr(), n, Fi,
                             Ti, cin, cout, taps, stride, int(relu), None)
    torch.cuda.synchronize(gpu)
    _lib.check(rc, "dz_k_conv2d_masked" if masked else "dz_k_conv2d")
    Y = Y.cpu()
    assert torch.isnan(Y[n * Fo * To * cout:]).all(), "a store past M Cout"
    return Y[:n * Fo * To * cout].view(n, Fo, To, cout)


def _operands(cin, cout, taps, stride):
    g = torch.Generator().manual_seed(cin * 1009 + cout * 31 + taps * 7 + stride)
    x = torch.randn(B, FI, TI, cin, generator=g)
    k = 3 if taps == 9 else 1
    w4 = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * taps))
    b = 0.1 * torch.randn(cout, generator=g)
    Fo, To = (FI - 1) // stride + 1, (TI - 1) // stride + 1
    r = torch.randn(B, Fo, To, cout, generator=g) if (cin + cout + taps) % 2 else None      # residual in half the cases
    return x, w4, b, r


_REF = {}


def _reference(case, ext_in):
    """Each row convolved alone over its own ext_in steps (zero padding at them): (y64, scale) over the live outputs."""
    key = (case, ext_in)
    if key not in _REF:
        cin, cout, taps, stride = case
        x, w4, b, r = _operands(*case)
        out = []
        for i, e in enumerate(ext_in):
            eo = (e - 1) // stride + 1
            out.append(W.conv_ref(x[i:i + 1, :e], w4, b, None if r is None else r[i:i + 1, :eo], stride == 1, stride))
        _REF[key] = out
    return _REF[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ext_in", EXTENTS, ids=lambda e: "ext" + "-".join(map(str, e)))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "cin{}-cout{}-taps{}-s{}".format(*c))
def test_masked_conv2d(gpu, case, ext_in, precision):
    cin, cout, taps, stride = case
    x, w4, b, r = _operands(*case)
    m = wsp_conv_matrix(w4)
    relu = stride == 1
    ext_out = tuple((e - 1) // stride + 1 for e in ext_in)
    xz = x.clone()
    for i, e in enumerate(ext_in):
        xz[i, e:] = 0.0                                   # the caller's contract: zeros at or past the input's live steps
    kw = dict(taps=taps, stride=stride, relu=relu, precision=precision)
    Y = run_masked(gpu, xz, m, b, r, ext_out, **kw)
    assert not torch.isnan(Y).any(), "an output position was not stored"
    worst = 0.0
    for i, (eo, (want, scale)) in enumerate(zip(ext_out, _reference(case, ext_in))):
        assert (Y[i, eo:].view(torch.int32) == 0).all(), f"row {i}: a position at or past step {eo} is not +0.0"
        worst = max(worst, ((Y[i, :eo].double() - want[0]).abs() / scale[0]).max().item())
        # the row alone gives the same bits
        alone = run_masked(gpu, xz[i:i + 1], m, b, None if r is None else r[i:i + 1], ext_out[i:i + 1], **kw)
        assert torch.equal(alone[0].view(torch.int32), Y[i].view(torch.int32)), f"row {i} depends on its batch"
    print(f"MASKED-CONV2D {precision} cin{cin} cout{cout} taps{taps} s{stride} ext{ext_in} err={worst:.3e}")
    assert worst <= GATE[precision], worst
    # with every row whole the masked instance is the unmasked one, bit for bit
    Fo = (FI - 1) // stride + 1
    full = run_masked(gpu, x, m, b, r, (Fo,) * B, **kw)
    plain = run_masked(gpu, x, m, b, r, None, masked=False, **kw)
    assert torch.equal(full.view(torch.int32), plain.view(torch.int32))


def test_masked_conv2d_dead_tiles(gpu):
    """Rows long enough for whole 128- and 96-row tiles inside a dead tail (the tiles that load nothing): zeros there,
    the live part unchanged."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 40, 8, 32, generator=g)
    w4 = torch.randn(64, 32, 3, 3, generator=g) * math.sqrt(2.0 / 288)
    b = 0.1 * torch.randn(64, generator=g)
    ext = (3, 17)
    for i, e in enumerate(ext):
        x[i, e:] = 0.0
    for precision in PRECISIONS:
        Y = run_masked(gpu, x, wsp_conv_matrix(w4), b, None, ext, taps=9, stride=1, relu=True, precision=precision)
        for i, e in enumerate(ext):
            want, scale = W.conv_ref(x[i:i + 1, :e], w4, b, None, True, 1)
            assert (Y[i, e:].view(torch.int32) == 0).all()
            assert ((Y[i, :e].double() - want[0]).abs() / scale[0]).max().item() <= GATE[precision]


# ---- squeeze-excitation ----------------------------------------------------------------------------------------------
SE_CASES = ((32, 32), (64, 16), (128, 128), (256, 256), (384, 96))          # (C, Cr); 384: 96 channel quads do not divide 256


def _se_operands(C, Cr):
    g = torch.Generator().manual_seed(C * 13 + Cr)
    rows, Tb, Fq = 3, 13, 5
    ext = (1, 6, 13)                                       # 5, 30 and 65 live positions: fewer than, and more than, the 16 slices
    y = torch.randn(rows, Tb, Fq, C, generator=g)
    for i, e in enumerate(ext):
        y[i, e:] = 0.0
    w1 = torch.randn(Cr, C, generator=g) / math.sqrt(C)
    w2 = torch.randn(C, Cr, generator=g) / math.sqrt(Cr)
    b1, b2 = 0.1 * torch.randn(Cr, generator=g), 0.1 * torch.randn(C, generator=g)
    return y, ext, w1, b1, w2, b2


@pytest.mark.parametrize("C,Cr", SE_CASES)
def test_se_gate(gpu, C, Cr):
    y, ext, w1, b1, w2, b2 = _se_operands(C, Cr)
    rows, Tb, Fq, _ = y.shape
    d = lambda t: t.contiguous().to(gpu)
    dy, de = d(y), torch.tensor(ext, dtype=torch.int32, device=gpu)
    dw1t, db1, dw2t, db2 = d(w1.t()), d(b1), d(w2.t()), d(b2)
    part = torch.full((rows * 16 * C,), float("nan"), device=gpu)
    gate = torch.full((rows * C + 8,), float("nan"), device=gpu)
    _lib.check(_lib.load().dz_k_sbr_se_gate(_lib.context(gpu.index or 0), dy.data_ptr(), rows, Tb, Fq, C, Cr, de.data_ptr(),
                                            dw1t.data_ptr(), db1.data_ptr(), dw2t.data_ptr(), db2.data_ptr(),
                                            part.data_ptr(), gate.data_ptr(), None), "dz_k_sbr_se_gate")
    torch.cuda.synchronize(gpu)
    got = gate.cpu()
    assert torch.isnan(got[rows * C:]).all() and torch.isfinite(got[:rows * C]).all()
    got = got[:rows * C].view(rows, C).double()
    yd, w1d, w2d = y.double(), w1.double(), w2.double()
    for i, e in enumerate(ext):
        n = e * Fq
        live = yd[i, :e].reshape(n, C)
        mean, e_mean = live.mean(0), (n + 2) * U * live.abs().mean(0)
        pre = mean @ w1d.t() + b1.double()
        e_h = e_mean @ w1d.abs().t() + (C + 2) * U * (mean.abs() @ w1d.abs().t() + b1.double().abs())
        h = pre.clamp(min=0)
        e_a = e_h @ w2d.abs().t() + (Cr + 2) * U * (h @ w2d.abs().t() + b2.double().abs())
        want = torch.sigmoid(h @ w2d.t() + b2.double())
        bound = 0.25 * e_a + 4 * U                          # sigmoid' <= 1 / 4; expf and the division: a few ulps of a value <= 1
        err = (got[i] - want).abs()
        print(f"SE-GATE C{C} Cr{Cr} ext{e}: err {err.max():.3e} (bound {bound.min():.3e} .. {bound.max():.3e})")
        assert (err <= bound).all(), (err / bound).max().item()


@pytest.mark.parametrize("C", (32, 384))
def test_se_apply(gpu, C):
    y, ext, *_ = _se_operands(C, C)
    rows, Tb, Fq, _ = y.shape
    g = torch.Generator().manual_seed(C)
    gate = torch.rand(rows, C, generator=g)
    r = torch.randn(rows, Tb, Fq, C, generator=g)
    y = torch.randn(rows, Tb, Fq, C, generator=g)           # (non-zero in the dead tail too: the kernel must not read it through)
    dy, dg, dr = y.to(gpu), gate.to(gpu), r.to(gpu)
    de = torch.tensor(ext, dtype=torch.int32, device=gpu)
    out = torch.full((y.numel() + 8,), float("nan"), device=gpu)
    _lib.check(_lib.load().dz_k_sbr_se_apply(_lib.context(gpu.index or 0), dy.data_ptr(), dg.data_ptr(), dr.data_ptr(), rows,
                                             Tb, Fq, C, de.data_ptr(), out.data_ptr(), None), "dz_k_sbr_se_apply")
    torch.cuda.synchronize(gpu)
    got = out.cpu()
    assert torch.isnan(got[y.numel():]).all()
    got = got[:y.numel()].view(y.shape)
    for i, e in enumerate(ext):
        assert (got[i, e:].view(torch.int32) == 0).all()
        prod = gate[i].double() * y[i, :e].double()
        want = (prod + r[i, :e].double()).clamp(min=0)
        bound = 2 * U * (prod.abs() + r[i, :e].double().abs())          # one fused multiply-add
        assert ((got[i, :e].double() - want).abs() <= bound).all()


# ---- attention pooling -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (640, 300))
def test_attention_pooling(gpu, C):
    """T4_g = 1, 2 and 63 frames of a 63-frame buffer; channel 7 is constant over time, so its variance reaches the
    1e-5 clamp (sg = sqrt(1e-5)); channel 9 varies by 1e-2 about 0.5: a variance of 1e-4, just above it, where sum w x^2 -
    mu^2 cancels four digits."""
    g = torch.Generator().manual_seed(C)
    rows, Tb, ext = 3, 63, (1, 2, 63)
    x = torch.randn(rows, Tb, C, generator=g)
    x[:, :, 7] = 0.75
    x[:, :, 9] = 0.5 + 1e-2 * torch.randn(rows, Tb, generator=g)
    logits = 2.0 * torch.randn(rows, Tb, C, generator=g)
    dx, dl = x.to(gpu), logits.to(gpu)
    de = torch.tensor(ext, dtype=torch.int32, device=gpu)
    out = torch.full((rows * 2 * C + 8,), float("nan"), device=gpu)
    _lib.check(_lib.load().dz_k_sbr_att_pool(_lib.context(gpu.index or 0), dx.data_ptr(), dl.data_ptr(), rows, Tb, C,
                                             de.data_ptr(), out.data_ptr(), None), "dz_k_sbr_att_pool")
    torch.cuda.synchronize(gpu)
    got = out.cpu()
    assert torch.isnan(got[rows * 2 * C:]).all() and torch.isfinite(got[:rows * 2 * C]).all()
    got = got[:rows * 2 * C].view(rows, 2 * C).double()
    for i, n in enumerate(ext):
        xd, ld = x[i, :n].double(), logits[i, :n].double()
        w = torch.softmax(ld, dim=0)
        mu = (xd * w).sum(0)
        var = ((xd ** 2) * w).sum(0) - mu ** 2                       # the definition's form, in float64
        sg = var.clamp(min=1e-5).sqrt()
        # weights: expf of a difference rounded at u |l - max|, a sum of n terms, a division
        k = n + 8 + (ld.max(0).values - ld.min(0).values)
        e_mu = 2 * k * U * (w * xd.abs()).sum(0)
        dev = (xd - mu).abs()
        e_var = 2 * k * U * (w * dev ** 2).sum(0) + 2 * (w * dev).sum(0) * e_mu + e_mu ** 2
        e_sg = e_var / (2 * sg) + 4 * U * sg
        err_mu, err_sg = (got[i, :C] - mu).abs(), (got[i, C:] - sg).abs()
        print(f"ATT-POOL C{C} T{n}: mu err {err_mu.max():.3e} sg err {err_sg.max():.3e}")
        assert (err_mu <= e_mu + 1e-300).all(), (err_mu / e_mu).max().item()
        assert (err_sg <= e_sg).all(), (err_sg / e_sg).max().item()
        assert abs(got[i, C + 7].item() - math.sqrt(1e-5)) <= 4 * U * math.sqrt(1e-5)          # the clamp
        if n == 1:
            assert torch.equal(got[i, :C].float(), x[i, 0]) and (got[i, C:] - math.sqrt(1e-5)).abs().max() <= 1e-9
