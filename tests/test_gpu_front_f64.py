"""The SincNet front end — wave_stats, the three stage-0 kernels, finalize_norm, the norm-from-partials prologue of
conv_pool / gemm_split, and the chain of the three — against the float64 restatement of tests/front_ref.py, channel
by channel ("Accuracy of the front end").

Measure: ``cond_err = |got - ref| / den`` per element, ``den`` the same stage on the operands' absolute values, so a
quiet channel's error counts against that channel and not against the loudest output of the tensor.  One gate for
every kernel: ``max(1e-6, 4 e32)``, e32 the same measure of the float32 restatement (plain torch on the CPU) on the
same case, computed here (4: 22 mantissa bits of the f16x3 operands against float32's 24, as in
tests/test_gpu_lstm_f64.py; 1e-6: what test_gpu_kernels.py::test_f16x3_dynamic_range_map grants f16x3).  The tile
partials are gated by ``part_err`` at the same bound (sums of squares against S den (|ref| + |got|): front_ref.part_err).  tests/test_front_ref_host.py asserts on the CPU that e32 stays
under 2e-5 in every cell used here and that the measure catches an operand that lost its low plane.

Waveform rows lie ``roundup4(S)`` floats apart with NaN in every float between sample S and the next row and in a
64-float tail: no kernel may depend on what lies behind sample S (include/diart_amd.h, next to dz_k_sinc_conv0).
Every output buffer is pre-filled with NaN and carries guard rows that must stay NaN.

Lines starting with ``FRONT|`` carry the measured figures (pytest -s).
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import pytest
import torch

from diart_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import front_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3
NAN = float("nan")


def _ctx(dev):
    return _lib.context(dev.index or 0)


def _sync():
    torch.cuda.synchronize()


def _rows(gpu, rows, S):
    """rows (each (S,)) -> one device buffer, rows roundup4(S) apart, NaN wherever there is no sample; stride"""
    stride = (S + 3) // 4 * 4
    flat = torch.full((len(rows) * stride + 64,), NAN)
    for i, r in enumerate(rows):
        flat[i * stride: i * stride + S] = r
    return flat.to(gpu), stride


def _guarded(gpu, rows, *shape):
    return torch.full((rows + GUARD, *shape), NAN, device=gpu)


def _take(buf, rows, what, strict=True):
    """the first `rows` rows of a guarded buffer on the CPU: guard untouched, no NaN left inside (strict)"""
    raw = buf.cpu()
    assert torch.isnan(raw[rows:]).all(), f"{what}: wrote behind its last row"
    assert not strict or not torch.isnan(raw[:rows]).any(), f"{what}: NaN in (or rows missing from) the output"
    return raw[:rows]


def _wave_stats(gpu, d, stride, B, S, finite=True):
    st = _guarded(gpu, B, 2)
    _lib.check(_lib.load().dz_k_wave_stats(_ctx(gpu), d.data_ptr(), stride, B, S, st.data_ptr(), None), "dz_k_wave_stats")
    _sync()
    raw = st.cpu()
    assert torch.isnan(raw[B:]).all(), "wave_stats: wrote behind row B"
    if finite:
        assert torch.isfinite(raw[:B]).all(), "wave_stats: non-finite statistics of a finite window"
    return st, raw[:B]


def _ulp32(t):
    t = t.float()
    return (torch.nextafter(t.abs(), torch.full_like(t, float("inf"))) - t.abs()).double()


# =========================================================================== a. wave_stats
WS_CASES = ("speech", "dc_large", "silence", "speech_x25", "speech_x1e-4")


@pytest.mark.parametrize("S", [80000, 81920, 81924, 160000, 2661, 2662, 2663, 281, 31, 9])
def test_wave_stats_lengths(gpu, S):
    """every length class of wave_stats_kernel: S % 4 != 0, the uncached loop behind 10240 samples per slice (S > 81920),
    slices shorter than one float4 (S = 31) and empty slices (S = 9: eight slices of 4 samples, five of them empty)"""
    x = torch.stack([R.make_case(c, S) for c in WS_CASES])
    got = []
    for lo, hi in ((0, 4), (4, 5)):
        d, stride = _rows(gpu, list(x[lo:hi]), S)
        got.append(_wave_stats(gpu, d, stride, hi - lo, S)[1])
    got = torch.cat(got).double()
    mean, rstd = R.wave_stats(x)
    std = ((x.double() - mean[:, None]) ** 2).mean(1).sqrt()
    for i, c in enumerate(WS_CASES):
        em, er = (got[i, 0] - mean[i]).abs().item(), ((got[i, 1] - rstd[i]).abs() / rstd[i]).item()
        tol = 2.0 ** -22 * max(mean[i].abs().item(), std[i].item())
        print(f"FRONT|wave_stats|{S}|{c}|mean err {em:.2e} (tol {tol:.2e})|rstd rel {er:.2e}")
        assert em <= tol, (S, c, em, tol)
        assert er <= 2e-6, (S, c, er)
    sil = WS_CASES.index("silence")
    want = torch.tensor(1.0 / (1e-5 ** 0.5), dtype=torch.float64)
    assert got[sil, 0] == 0.0 and (got[sil, 1] - want.float().double()).abs() <= _ulp32(want), got[sil]


@pytest.mark.parametrize("S", [2663, 80000])
def test_wave_stats_bad_rows_stay_alone(gpu, S):
    """row 1 holds a NaN, row 2 an Inf: their statistics are non-finite, rows 0 and 3 bit-identical to a run without them"""
    good = [R.make_case("speech", S), R.make_case("speech_x25", S, 1)]
    bad1, bad2 = R.make_case("speech", S, 2).clone(), R.make_case("speech", S, 3).clone()
    bad1[S // 3] = NAN
    bad2[S - 1] = float("inf")
    d, stride = _rows(gpu, [good[0], bad1, bad2, good[1]], S)
    four = _wave_stats(gpu, d, stride, 4, S, finite=False)[1]
    d, stride = _rows(gpu, good, S)
    two = _wave_stats(gpu, d, stride, 2, S)[1]
    assert not torch.isfinite(four[1]).any() and not torch.isfinite(four[2]).any(), four
    assert torch.equal(four[0], two[0]) and torch.equal(four[3], two[1])


# =========================================================================== b. stage 0
SHIPPED0 = ("f32", "split")
EXPERIMENT0 = {"split_h": ("DZ_CONV0_V2", "0"), "rot1": ("DZ_CONV0_ROT", "1"), "rot2": ("DZ_CONV0_ROT", "2"),
               "rot3": ("DZ_CONV0_ROT", "3"), "pair": None}
KERNELS0 = SHIPPED0 + tuple(EXPERIMENT0)


def _select0(kernel, monkeypatch):
    if kernel in EXPERIMENT0:
        if not _lib.experiments():
            pytest.skip("role / kernel switches and sinc_conv0_pair exist in the experiments build only")
        if EXPERIMENT0[kernel]:
            monkeypatch.setenv(*EXPERIMENT0[kernel])


@functools.lru_cache(maxsize=None)
def _bank_operands(net, kernel, gpu):
    from diart_amd.weights import PackedConv0Pair, _pad2, fold_sinc_filters, split_f16
    if kernel == "f32":
        return fold_sinc_filters(R.bank(net)).to(gpu)
    if kernel == "pair":
        sds = []
        for n in ("seg", "emb"):
            sd = dict(R._state(n))
            sd["sincnet.wav_norm1d.weight"] = torch.tensor([R.AFFINE[n][0]])
            sd["sincnet.wav_norm1d.bias"] = torch.tensor([R.AFFINE[n][1]])
            sds.append(sd)
        return PackedConv0Pair(sds[0], sds[1], gpu)
    return split_f16(_pad2(R.bank(net), 96, 256)).to(gpu)


def _stage0(gpu, kernel, net, d, stride, B, S, stats, strict=True):
    """one stage-0 launch -> y (B, 80, P0), partials (B, ntile, 80, 2), tile length in conv frames; strict: no NaN in any
    row (a batch with a non-finite window checks its healthy rows itself)"""
    lib = _lib.load()
    F0, P0 = R.geometry(S)
    tile = 192 if kernel == "f32" else 96
    nt = R.ntile(F0, tile)
    if kernel != "f32":
        assert lib.dz_k_conv0_split_ntile(S) == nt
    gamma, beta = R.AFFINE[net]
    ops = _bank_operands(net, "f32" if kernel == "f32" else "pair" if kernel == "pair" else "split", gpu)
    y0, part = _guarded(gpu, B * P0, 80), _guarded(gpu, B * nt, 80, 2)
    if kernel == "f32":
        _lib.check(lib.dz_k_sinc_conv0(_ctx(gpu), d.data_ptr(), stride, B, S, stats.data_ptr(), gamma, beta, ops.data_ptr(),
                                       y0.data_ptr(), part.data_ptr(), None), "dz_k_sinc_conv0")
    elif kernel == "pair":
        mom = torch.full((B, lib.dz_wave_stats_floats()), NAN, device=gpu)
        _lib.check(lib.dz_wave_stats(_ctx(gpu), d.data_ptr(), stride, B, S, mom.data_ptr(), None), "dz_wave_stats")
        y_o, p_o = _guarded(gpu, B * P0, 80), _guarded(gpu, B * nt, 80, 2)          # the other network's
        ys, ps = ((y0, y_o), (part, p_o)) if net == "seg" else ((y_o, y0), (p_o, part))
        _lib.check(lib.dz_k_sinc_conv0_pair(_ctx(gpu), d.data_ptr(), stride, B, S, mom.data_ptr(), ops.planes.data_ptr(),
                                            ops.bsum.data_ptr(), R.AFFINE["seg"][0], R.AFFINE["emb"][0], ys[0].data_ptr(),
                                            ys[1].data_ptr(), ps[0].data_ptr(), ps[1].data_ptr(), None), "dz_k_sinc_conv0_pair")
        _sync()
        _take(y_o, B * P0, "pair: the other network's y0", strict)
        _take(p_o, B * nt, "pair: the other network's partials", strict)
    else:
        _lib.check(lib.dz_k_sinc_conv0_split(_ctx(gpu), d.data_ptr(), stride, B, S, stats.data_ptr(), gamma, beta,
                                             ops.data_ptr(), y0.data_ptr(), part.data_ptr(), None), "dz_k_sinc_conv0_split")
    _sync()
    y = _take(y0, B * P0, f"{kernel}: y0", strict).view(B, P0, 80).permute(0, 2, 1)
    return y, _take(part, B * nt, f"{kernel}: partials", strict).view(B, nt, 80, 2), tile


def _gate0(kernel, net, cases, S, y, part):
    """gate (b) on rows of `cases` (None: not checked) -> list of failures"""
    fails = []
    for i, case in enumerate(cases):
        if case is None:
            continue
        _, ref, den, e32 = R.stage0_ref(net, case, S)
        g = R.gate(e32)
        e = R.cond_err(y[i: i + 1], ref, den)[0]
        lo, hi = e[:64].max().item(), e[64:].max().item()
        e1, e2 = (v.max().item() for v in R.part_err(part[i: i + 1], ref, den, y[i: i + 1]))
        print(f"FRONT|stage0|{kernel}|{net}|{S}|{case}|e32 {e32:.2e}|gate {g:.2e}|ch0-63 {lo:.2e}|ch64-79 {hi:.2e}|"
              f"sum {e1:.2e}|sumsq {e2:.2e}")
        for name, v in (("channels 0..63", lo), ("channels 64..79", hi), ("partial sums", e1), ("partial sums of squares", e2)):
            if not v <= g:
                fails.append((kernel, net, S, case, name, v, g))
    return fails


@pytest.mark.parametrize("S", R.STAGE0_S)
@pytest.mark.parametrize("net", ["seg", "emb"])
@pytest.mark.parametrize("kernel", KERNELS0)
def test_stage0_per_channel(gpu, monkeypatch, kernel, net, S):
    _select0(kernel, monkeypatch)
    cases = [c for n, c, s in R.stage0_cells() if n == net and s == S]
    fails = []
    for lo in range(0, len(cases), 4):
        batch = cases[lo: lo + 4]
        d, stride = _rows(gpu, [R.stage0_ref(net, c, S)[0][0] for c in batch], S)
        st, _ = _wave_stats(gpu, d, stride, len(batch), S)
        y, part, _ = _stage0(gpu, kernel, net, d, stride, len(batch), S, st)
        fails += _gate0(kernel, net, batch, S, y, part)
    _lib.range_check(gpu.index or 0)
    assert not fails, fails


# =========================================================================== c. row isolation in stage 0
@pytest.mark.parametrize("S", [2661, 2663])
@pytest.mark.parametrize("net", ["seg", "emb"])
@pytest.mark.parametrize("kernel", KERNELS0)
def test_stage0_rows_are_isolated(gpu, monkeypatch, kernel, net, S):
    """adjacent rows, NaN behind every row's last sample, and a NaN-and-Inf window as row 1: the healthy rows pass gate
    (b) and are bit-identical with and without the bad neighbour"""
    _select0(kernel, monkeypatch)
    cases = ["speech", "speech_x25", "speech_x1e-4"]
    rows = [R.stage0_ref(net, c, S)[0][0] for c in cases]
    bad = R.make_case("speech", S, 2).clone()
    bad[7], bad[S // 2], bad[S - 1] = float("-inf"), NAN, float("inf")
    d, stride = _rows(gpu, rows, S)
    st, _ = _wave_stats(gpu, d, stride, 3, S)
    y3, p3, _ = _stage0(gpu, kernel, net, d, stride, 3, S, st)
    d, stride = _rows(gpu, [rows[0], bad, rows[1], rows[2]], S)
    st, _ = _wave_stats(gpu, d, stride, 4, S, finite=False)
    # (the bad row's own outputs are not constrained here: the handles' last kernels write its NaN row)
    y4, p4, _ = _stage0(gpu, kernel, net, d, stride, 4, S, st, strict=False)
    try:
        _lib.range_check(gpu.index or 0)           # the bad row's Inf is reported (and clamped): reset the flag
    except _lib.DiartAmdError:
        pass
    keep = [0, 2, 3]
    assert not torch.isnan(y4[keep]).any() and not torch.isnan(p4[keep]).any()
    fails = _gate0(kernel, net, cases, S, y3, p3) + _gate0(kernel, net, [cases[0], None, cases[1], cases[2]], S, y4, p4)
    assert not fails, fails
    assert torch.equal(y4[keep], y3) and torch.equal(p4[keep], p3), "a healthy row changed with its neighbour"


# =========================================================================== d. finalize_norm alone
def _finalize_ref(part32, T, gamma, beta):
    """float64 arithmetic on the float32 partials, tiles in order -> scale, shift (float64), where the variance clamped"""
    p = part32.double()
    s = torch.zeros_like(p[:, 0, :, 0])
    ss = torch.zeros_like(s)
    for t in range(p.shape[1]):
        s, ss = s + p[:, t, :, 0], ss + p[:, t, :, 1]
    mean = s / T
    var = ss / T - mean * mean
    sc = gamma.double()[None, :] / torch.sqrt(torch.clamp(var, min=0.0) + 1e-5)
    return sc, beta.double()[None, :] - mean * sc, var < 0.0


def _finalize_gpu(gpu, part32, T, gamma, beta):
    B, nt, Cc, _ = part32.shape
    dp, dg, db = part32.contiguous().to(gpu), gamma.to(gpu), beta.to(gpu)
    sc, sh = _guarded(gpu, B, Cc), _guarded(gpu, B, Cc)
    _lib.check(_lib.load().dz_k_finalize_norm(_ctx(gpu), dp.data_ptr(), B, nt, Cc, T, dg.data_ptr(), db.data_ptr(),
                                             sc.data_ptr(), sh.data_ptr(), None), "dz_k_finalize_norm")
    _sync()
    return sc, sh


@pytest.mark.parametrize("Cc", [80, 60, 64])
def test_finalize_norm_alone(gpu, Cc):
    """float32 partials made on the CPU from a known float64 tensor -> scale / shift equal to float64 arithmetic on those
    partials to 1 ulp of float32; near-constant channels (3.0 + 1e-3 noise, 3.0 + 1e-4 noise: sum of squares / T - mean^2
    comes out negative and is clamped) and an exactly constant one stay finite and equal to the reference"""
    B, clamped = 3, 0
    for nt in (1, 2, 3, 11, 12, 13, 84):
        g = torch.Generator().manual_seed(100 * Cc + nt)
        T = 32 * nt - 5
        mag = 10.0 ** (torch.rand(B, Cc, 1, generator=g, dtype=torch.float64) * 5.0 - 3.0)       # 1e-3 .. 1e2 per channel
        y = torch.randn(B, Cc, T, generator=g, dtype=torch.float64).abs() * mag
        y[:, 0] = 3.0
        y[:, 1] = 3.0 + 1e-3 * torch.randn(B, T, generator=g, dtype=torch.float64)
        y[:, 2:6] = 3.0 + 1e-4 * torch.randn(B, 4, T, generator=g, dtype=torch.float64)
        part32 = R.tile_partials(y, 96, 3 * T + 2).float()
        assert part32.shape == (B, nt, Cc, 2)
        gamma = torch.rand(Cc, generator=g) + 0.5
        beta = torch.randn(Cc, generator=g) * 0.1
        sc64, sh64, neg = _finalize_ref(part32, T, gamma, beta)
        clamped += int(neg[:, 1:6].sum())
        sc, sh = _finalize_gpu(gpu, part32, T, gamma, beta)
        sc, sh = _take(sc, B, "finalize_norm: scale"), _take(sh, B, "finalize_norm: shift")
        assert torch.isfinite(sc).all() and torch.isfinite(sh).all()
        for name, got, want in (("scale", sc, sc64), ("shift", sh, sh64)):
            off = (got.double() - want.float().double()).abs() / _ulp32(want)
            assert off.max().item() <= 1.0, (Cc, nt, name, off.max().item(), int(off.argmax()))
        # the exactly constant channel: variance 0 (or clamped to it), scale = gamma / sqrt(1e-5)
        assert ((sc[:, 0].double() - (gamma[0].double() / 1e-5 ** 0.5).float().double()).abs() <= 2 * _ulp32(sc[:, 0])).all()
    print(f"FRONT|finalize_norm|C {Cc}|clamped variances among the near-constant channels: {clamped}")
    assert clamped > 0, "no near-constant channel met the clamp: the case does not test it"


# =========================================================================== e. norm from partials: the production path
E_S = 12000                                  # P0 = 391, P1 = 129: at least 84 frames for the 84-tile partials of both stages
E_CASES = ("lowpass", "tone", "speech")      # channel scales orders of magnitude apart, another statistic per row
POOL_KERNELS = {"conv_pool": 256, "conv_pool_v2": 512, "gemm_split": 384}       # threads per workgroup (the launch code)


@functools.lru_cache(maxsize=None)
def _e_inputs(net):
    """float32 roundings of the float64 stage-0 and stage-1 outputs of E_CASES: the inputs of stages 1 and 2"""
    x = torch.stack([R.make_case(c, E_S) for c in E_CASES])
    ys = R.chain(x, net)
    return {1: ys[0].float(), 2: ys[1].float()}


def _pool_desc(gpu, keep, X, Wp, ws, bias, **norm):
    """dz_convgemm_desc of a SincNet stage 1 / 2 call on X (B, Tin, Cp) channels-last; outputs NaN-filled with guards"""
    lib = _lib.load()
    B, Tin, Cp = X.shape
    Tout = Tin - 4
    Tst, nt = Tout // 3, lib.dz_k_convgemm_ntile(Tout)
    Y, part = _guarded(gpu, B * Tst, 64), _guarded(gpu, B * nt, 64, 2)
    d = _lib.ConvGemmDesc()
    d.X, d.W, d.Wsplit, d.bias, d.Y, d.partials = X.data_ptr(), Wp.data_ptr(), ws.data_ptr(), bias.data_ptr(), Y.data_ptr(), part.data_ptr()
    d.B, d.Tin, d.Tout, d.Cin, d.taps, d.dil = B, Tin, Tout, Cp, 5, 1
    d.K, d.Kpad, d.Npad, d.Nstore, d.ldx, d.ldy, d.nld, d.Tstore = 5 * Cp, Wp.shape[1], 64, 64, Cp, 64, Cp, Tst
    d.xbs, d.ybs, d.ysplit, d.norm_on_load, d.epi = Tin * Cp, Tst * 64, B * Tst * 64, 1, _lib.EPI_POOL3
    for k, v in norm.items():
        if isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        setattr(d, k, v)
    return d, Y, part, B * Tst, B * nt


def _pool_run(gpu, kernel, *args, **norm):
    keep = []
    d, Y, part, ry, rp = _pool_desc(gpu, keep, *args, **norm)
    fn = _lib.load().dz_k_gemm_split if kernel == "gemm_split" else _lib.load().dz_k_conv_pool
    _lib.check(fn(_ctx(gpu), C.byref(d), None), kernel)
    _sync()
    B = args[0].shape[0]
    return _take(Y, ry, f"{kernel}: Y").view(B, -1, 64), _take(part, rp, f"{kernel}: partials").view(B, -1, 64, 2)


def _stage_operands(gpu, net, i, Cp):
    from diart_amd.weights import _conv_pack, _pad1, split_f16
    w, b, g, bt = R.conv_weights(net, i)
    Wp = _conv_pack(w, Cp, 64, (5 * Cp + 31) // 32 * 32)
    return (w, b, g, bt), (Wp.to(gpu), split_f16(Wp).to(gpu), _pad1(b, 64).to(gpu), _pad1(g, Cp).to(gpu), _pad1(bt, Cp).to(gpu))


def _channels_last(y, Cp):
    B, Cc, T = y.shape
    X = torch.zeros(B, T, Cp)
    X[:, :, :Cc] = y.permute(0, 2, 1)
    return X


def _gate_stage(tag, Y, part, xin, sc, sh, w, b):
    """gate a stage 1 / 2 output Y (B, Tp, 64) and its partials against float64 on input xin (B, Cin, T) float32 with
    scale / shift (float64) -> failures"""
    ref = R.stage(xin, sc, sh, w, b)
    den = R.stage_den(xin, sc, sh, w, b)
    y32 = R.stage(xin, sc.float(), sh.float(), w, b, R.F32)
    got = Y[:, :, :60].permute(0, 2, 1)
    assert got.shape == ref.shape and (Y[:, :, 60:] == 0).all()
    fails = []
    for r in range(ref.shape[0]):
        e32 = R.cond_err(y32[r], ref[r], den[r]).max().item()
        g = R.gate(e32)
        e = R.cond_err(got[r], ref[r], den[r]).max().item()
        e1, e2 = (v.max().item() for v in R.part_err(part[r: r + 1, :, :60], ref[r: r + 1], den[r: r + 1], got[r: r + 1]))
        print(f"FRONT|{tag}|row {r}|e32 {e32:.2e}|gate {g:.2e}|out {e:.2e}|sum {e1:.2e}|sumsq {e2:.2e}")
        fails += [(tag, r, n, v, g) for n, v in (("out", e), ("sum", e1), ("sumsq", e2)) if not v <= g]
    return fails


@pytest.mark.parametrize("stage_i", [1, 2], ids=["Cin80", "Cin60"])
@pytest.mark.parametrize("net", ["seg", "emb"])
@pytest.mark.parametrize("kernel", list(POOL_KERNELS))
def test_norm_from_partials(gpu, monkeypatch, kernel, net, stage_i):
    """conv_pool / conv_pool_v2 / gemm_split(POOL3) handed the producer's tile partials (npart, ngamma, nbeta,
    npart_tiles, npart_T; nscale / nshift NULL), at the tile counts around the G = nthreads / C thread groups and the 4 G
    unrolling of dz_norm_from_partials: bit for bit what the same kernel gives with nscale / nshift from
    dz_k_finalize_norm on the same partials, and the float64 stage by the cond_err rule"""
    if kernel == "conv_pool_v2":
        if not _lib.experiments():
            pytest.skip("conv_pool_v2 is only in the experiments build")
        monkeypatch.setenv("DZ_CONV_POOL_V2", "1")
    Cp = 80 if stage_i == 1 else 64
    G = POOL_KERNELS[kernel] // Cp
    xin = _e_inputs(net)[stage_i]                                   # (3, Cin, T) float32
    B, Cin, T = xin.shape
    (w, b, g, bt), (Wp, ws, bias, dgam, dbet) = _stage_operands(gpu, net, stage_i, Cp)
    X = _channels_last(xin, Cp).to(gpu)
    fails = []
    for nt in sorted({1, G - 1, G, 4 * G - 1, 4 * G, 4 * G + 1, 84}):
        assert 1 <= nt <= T
        # the producer's partials: T frames in nt ragged tiles (T is no multiple of any tile length used)
        edges = [i * T // nt for i in range(nt + 1)]
        p64 = torch.zeros(B, nt, Cp, 2, dtype=torch.float64)
        for t in range(nt):
            blk = xin.double()[:, :, edges[t]: edges[t + 1]]
            p64[:, t, :Cin, 0], p64[:, t, :Cin, 1] = blk.sum(2), (blk * blk).sum(2)
        p32 = p64.float()
        dpart = p32.to(gpu)
        Ya, Pa = _pool_run(gpu, kernel, X, Wp, ws, bias, npart=dpart, ngamma=dgam, nbeta=dbet, npart_tiles=nt, npart_T=T)
        sc, sh = _finalize_gpu(gpu, p32, T, dgam.cpu(), dbet.cpu())
        _take(sc, B, "scale"), _take(sh, B, "shift")
        Yb, Pb = _pool_run(gpu, kernel, X, Wp, ws, bias, nscale=sc, nshift=sh)
        same = torch.equal(Ya, Yb) and torch.equal(Pa, Pb)
        print(f"FRONT|npart|{kernel}|{net}|Cin {Cin}|tiles {nt} (G = {G})|bit for bit: {same}")
        if not same:
            fails.append((kernel, net, Cin, nt, "not bit for bit", (Ya - Yb).abs().max().item()))
        sc64, sh64, _ = _finalize_ref(p32[:, :, :Cin], T, g, bt)
        fails += _gate_stage(f"npart|{kernel}|{net}|Cin {Cin}|tiles {nt}", Ya, Pa, xin, sc64, sh64, w, b)
    _lib.range_check(gpu.index or 0)
    assert not fails, fails


# =========================================================================== f. the chain, once
def _chain_err(got, ref):
    """per (row, channel): max over time |got - ref| / std of the reference channel -> the worst"""
    return ((got.double() - ref).abs().amax(2) / ref.std(2, unbiased=False)).max().item()


def test_front_end_chain(gpu):
    """speech / lowpass / click at S = 80000: wave_stats -> stage 0 -> norm from partials -> stage 1 -> stage 2 on the
    shipped kernels against float64 all the way, per channel relative to the channel's own spread; gate 4 x what the
    float32 restatement of the whole chain gives on this batch, floor 2e-5"""
    net, S, cases = "seg", 80000, ("speech", "lowpass", "click")
    x = torch.stack([R.make_case(c, S) for c in cases])
    ref, y32 = R.chain(x, net), R.chain(x, net, R.F32)
    d, stride = _rows(gpu, list(x), S)
    st, _ = _wave_stats(gpu, d, stride, 3, S)
    lib = _lib.load()
    F0, P0 = R.geometry(S)
    nt0 = lib.dz_k_conv0_split_ntile(S)
    assert (F0, P0, nt0) == (7975, 2658, 84)
    from diart_amd.weights import _pad2, split_f16
    fs = split_f16(_pad2(R.bank(net), 96, 256)).to(gpu)
    y0, part0 = _guarded(gpu, 3 * P0, 80), _guarded(gpu, 3 * nt0, 80, 2)
    _lib.check(lib.dz_k_sinc_conv0_split(_ctx(gpu), d.data_ptr(), stride, 3, S, st.data_ptr(), *R.AFFINE[net], fs.data_ptr(),
                                         y0.data_ptr(), part0.data_ptr(), None), "dz_k_sinc_conv0_split")
    _sync()
    got = [_take(y0, 3 * P0, "y0").view(3, P0, 80).permute(0, 2, 1)]
    _take(part0, 3 * nt0, "partials of stage 0")
    X, npart, ntiles = y0[:3 * P0].view(3, P0, 80), part0, nt0
    for i, Cp in ((1, 80), (2, 64)):
        _, (Wp, ws, bias, dgam, dbet) = _stage_operands(gpu, net, i, Cp)
        T = X.shape[1]
        keep = []
        desc, Y, part, ry, rp = _pool_desc(gpu, keep, X, Wp, ws, bias, npart=npart, ngamma=dgam, nbeta=dbet, npart_tiles=ntiles,
                                           npart_T=T)
        _lib.check(lib.dz_k_conv_pool(_ctx(gpu), C.byref(desc), None), "dz_k_conv_pool")
        _sync()
        Yc = _take(Y, ry, f"y{i}").view(3, -1, 64)
        _take(part, rp, f"partials of stage {i}")
        assert (Yc[:, :, 60:] == 0).all()
        got.append(Yc[:, :, :60].permute(0, 2, 1))
        X, npart, ntiles = Y[:ry].view(3, -1, 64), part, rp // 3
    _lib.range_check(gpu.index or 0)
    fails = []
    for i in range(3):
        assert got[i].shape == ref[i].shape
        e, e32 = _chain_err(got[i], ref[i]), _chain_err(y32[i], ref[i])
        g = max(2e-5, 4.0 * e32)
        print(f"FRONT|chain|{net}|y{i}|float32 chain {e32:.2e}|gate {g:.2e}|kernels {e:.2e}")
        if not e <= g:
            fails.append((i, e, g))
    assert not fails, fails
