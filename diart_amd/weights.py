"""State dict (pyannote checkpoint key names) -> packed fp32 device tensors for the kernels.

PyTorch-ROCm only *holds* the weights (north-star: "PyTorch-ROCm holds only the weight
tensors"); all arithmetic on them happens in ``libdiart_amd.so``.  Packing happens once,
on the CPU, at load time:

* sinc FIR bank generated from ``low_hz_ / band_hz_`` (asteroid ``ParamSincFB.filters``,
  SURVEY.md Appendix A.1) and stored k-major ``[252][80]`` (tap 251 is a zero pad);
* conv / TDNN weights reordered ``[co][tap][ci]`` so an im2col row of channels-last
  activations is contiguous, channel counts padded 60 -> 64 and 1500 -> 1536 with zeros;
* ``BatchNorm1d`` (eval) folded to a per-channel scale / shift applied after LeakyReLU;
* LSTM: both directions' ``W_ih`` stacked to one ``[1024][K]`` GEMM operand, ``b_ih+b_hh``
  pre-summed, ``W_hh`` as ``[2][512][128]``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import torch

from . import _lib

BN_EPS = 1e-5
# arithmetic of the GEMM-shaped layers: "f32" = exact-f32 MFMA (v_mfma_f32_16x16x4_f32);
# "f16x3" = both operands split into (hi, lo) f16 pairs (22 mantissa bits), 3 f16 MFMAs per product, f32
# accumulation (k_gemm_split.hip; ~2^-16 relative error per product)
PRECISIONS = ("f32", "f16x3")


def sinc_filters(low_hz_: torch.Tensor, band_hz_: torch.Tensor, window_: torch.Tensor,
                 n_: torch.Tensor, sample_rate: float = 16000.0, min_low_hz: float = 50.0,
                 min_band_hz: float = 50.0) -> torch.Tensor:
    """[80][251] band-pass filters: 40 cos (even) then 40 sin (odd)."""
    low = min_low_hz + torch.abs(low_hz_.float())
    high = torch.clamp(low + min_band_hz + torch.abs(band_hz_.float()), min_low_hz, sample_rate / 2)
    band = (high - low)[:, 0]
    n_ = n_.float().view(1, -1)
    window_ = window_.float()
    ft_low, ft_high = torch.matmul(low, n_), torch.matmul(high, n_)
    out = []
    for kind in ("cos", "sin"):
        if kind == "cos":
            left = ((torch.sin(ft_high) - torch.sin(ft_low)) / (n_ / 2)) * window_
            center = 2 * band.view(-1, 1)
            right = torch.flip(left, dims=[1])
        else:
            left = ((torch.cos(ft_low) - torch.cos(ft_high)) / (n_ / 2)) * window_
            center = torch.zeros_like(band.view(-1, 1))
            right = -torch.flip(left, dims=[1])
        out.append(torch.cat([left, center, right], dim=1) / (2 * band[:, None]))
    return torch.cat(out, dim=0)


def fold_sinc_filters(filt: torch.Tensor) -> torch.Tensor:
    """[80][251] symmetric bank -> the folded k-major image ``[128][96]`` ``sinc_conv0`` consumes.

    Row ``j`` is the tap at distance ``j`` from the centre (tap 125); columns 0..39 the cos (even)
    filters, 48..87 the sin (odd) filters, the rest zero.  ``conv = sum_j cos_j (x[c+j] + x[c-j])
    + sin_j (x[c+j] - x[c-j])``: the centre tap of the even filters is halved (exact), that of
    the odd filters is zero.  The symmetry is what ``ParamSincFB.filters`` builds (``right =
    flip(left)`` / ``-flip(left)``); a bank that does not have it is refused."""
    assert filt.shape == (80, 251), filt.shape
    f = filt.detach().float().cpu()
    left, right = torch.flip(f[:, :125], dims=[1]), f[:, 126:]
    scale = float(f.abs().max()) + 1e-30
    if float((right[:40] - left[:40]).abs().max()) > 1e-6 * scale or \
            float((right[40:] + left[40:]).abs().max()) > 1e-6 * scale or \
            float(f[40:, 125].abs().max()) > 1e-6 * scale:
        raise ValueError("sinc filter bank is not (anti)symmetric around its centre tap")
    out = torch.zeros(128, 96, dtype=torch.float32)
    out[0, :40] = 0.5 * f[:40, 125]
    out[1:126, :40] = right[:40].t()
    out[1:126, 48:88] = right[40:].t()
    return out


def split_f16(w: torch.Tensor, name: Optional[str] = None) -> torch.Tensor:
    """f32 matrix ``[N][K]`` -> int16 ``[2][N][K]`` of IEEE f16 bit patterns: plane 0 ``hi = f16(w)``,
    plane 1 ``lo = f16((w - hi) * 2^11)`` — the two-term split ``k_gemm_split.hip`` multiplies with
    (``w = hi + lo * 2^-11`` to 22 mantissa bits; the scale keeps ``lo`` a normal f16)."""
    w = w.detach().float().cpu().contiguous()
    if w.numel() and not bool(torch.isfinite(w).all()):
        # (max() of a tensor with NaN is NaN and every comparison below would pass: the kernels' clamps would then turn
        # the NaN planes into finite garbage where an f32 model gives NaN outputs)
        raise ValueError(f"split_f16({name or 'matrix'}): {int((~torch.isfinite(w)).sum())} non-finite weights — a damaged "
                         "checkpoint; the \"f16x3\" arithmetic refuses it (precision=\"f32\" computes NaN outputs like the reference)")
    big = float(w.abs().max()) if w.numel() else 0.0
    if big > 65504.0:
        raise ValueError(f"split_f16: |value| up to {big:g} does not fit the f16 range (+-65504) of the "
                         "\"f16x3\" arithmetic; load the model with precision=\"f32\"")
    hi = w.to(torch.float16)
    lo = ((w - hi.float()) * 2048.0).to(torch.float16)
    # How well do the two planes hold THIS matrix?  hi + lo * 2^-11 carries 22 mantissa bits while
    # |w| >= 2^-14; below, the f16 subnormal spacing leaves an ABSOLUTE error of 2^-36 per element
    # (tests/test_gpu_kernels.py::test_f16x3_dynamic_range_map: fp32-grade for magnitudes 2^-13 .. 2^15,
    # 4x worse per factor 4 below).  A layer whose energy sits in such tiny weights (nothing in the
    # published architectures does; a checkpoint with, say, a BatchNorm scale of 1e6 folded elsewhere
    # could) is measured here, once, at pack time: relative representation error of the layer, RMS.
    if w.numel():
        rep = (hi.double() + lo.double() / 2048.0 - w.double()).norm() / max(float(w.double().norm()), 1e-300)
        rep = float(rep)
        SPLIT_REPORT.append((name or f"matrix{len(SPLIT_REPORT)}", tuple(w.shape), rep))
        if rep > SPLIT_LIMIT:
            from .config import setting
            msg = (f"split_f16({name or 'matrix'}): the f16x3 planes represent this layer to {rep:.2e} (relative, RMS) — "
                   f"an f32 copy rounds to ~3e-8; its weights lie below the range the split holds to 22 bits "
                   f"(|w| >= 2^-14).  Load the model with precision=\"f32\"")
            if str(setting("split_strict", None, "1")) != "0":
                raise ValueError(msg + " (DZ_ENGINE=split_strict=0 turns this into a warning)")
            import warnings
            warnings.warn(msg)
    return torch.stack([hi, lo]).view(torch.int16).contiguous()


def kb_major(planes: torch.Tensor) -> torch.Tensor:
    """``[2][R][K]`` planes (``split_f16``) -> the same elements in the "kb-major" order the LDS-DMA kernels
    read (``k_gemm_pre.hip``, ``k_mlp_head.hip``; ``dz_kb`` in ``csrc/dz_common.h``): ``[2][K / 32][R][32]``,
    i.e. the 32-wide k-tile of consecutive rows is contiguous (16 rows = one 1 KiB LDS-DMA piece = 8 full
    cache lines; row-major planes made every piece 16 half lines).  ``K`` must be a multiple of 32."""
    two, rows, k = planes.shape
    assert two == 2 and k % 32 == 0, planes.shape
    return planes.reshape(2, rows, k // 32, 32).permute(0, 2, 1, 3).contiguous()


def from_kb(planes: torch.Tensor, rows: int, k: int) -> torch.Tensor:
    """Inverse of ``kb_major``: any tensor holding ``2 * rows * k`` kb-major elements -> ``[2][rows][k]``."""
    return planes.reshape(2, k // 32, rows, 32).permute(0, 2, 1, 3).reshape(2, rows, k).contiguous()


# (name, shape, relative RMS representation error) of every matrix split so far in this process, and
# the error above which a layer is refused: 2^-20 = 9.5e-7 is ~30x an f32 rounding and about where the
# whole-network gates of this package (segmentation 1e-4 abs, embedding 1e-4 rel) would start to notice
SPLIT_REPORT: list = []
SPLIT_LIMIT = 2.0 ** -20
# largest |w| of a kb-major weight matrix (the layers on k_gemm_pre.hip / k_gemm_g2.hip): 2^11 |w| must stay an f16
KB_WEIGHT_LIMIT = 31.98


def dft_matrices(n_fft: int = 400) -> torch.Tensor:
    """The windowed DFT of ECAPA's Fbank as ONE real GEMM operand, (2 * (n_fft // 2 + 1), n_fft) f64: rows
    0 .. 200 = cos(2 pi k n / N) * w[n], rows 201 .. 401 = sin(...) * w[n] (periodic Hamming window, like
    torch.stft's callers): frame @ rows.T = (Re, -Im) of rfft(frame * w); the power spectrum squares and adds
    the halves (pinned against numpy.fft by the DSP pin tests under tests/)."""
    n = torch.arange(n_fft, dtype=torch.float64)
    win = torch.hamming_window(n_fft, dtype=torch.float64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None]
    ang = 2.0 * math.pi * k * n[None, :] / n_fft
    return torch.cat([torch.cos(ang) * win, torch.sin(ang) * win], 0)


def lstm_whh_planes(whh: torch.Tensor, variant: int) -> torch.Tensor:
    """W_hh ``[2 dir][512][128]`` (PyTorch row order gate*128 + unit) -> int16 ``[2 dir][2 planes][512][128]``
    of f16 bit patterns for the matrix-core recurrence (``k_lstm_mfma.hip``).

    variant 0: ``split_f16`` per direction (lo scaled by 2^11, two accumulators in the kernel).
    variant 1 / 2: the activation scale of each gate row is folded in, ``W' = W * s * 2^SH`` with
    ``s = -log2(e)`` (i, f, o) or ``-2 log2(e)`` (g) and ``SH = 0 / 8``; ``hi = f16(W')``,
    ``lo = f16(W' - hi)`` UNSCALED, so that one accumulator holds ``hi.hi + hi.lo + lo.hi``."""
    whh = whh.detach().float().cpu()
    assert whh.shape == (2, 512, 128), whh.shape
    if variant in (0, 3):       # variant 3 = variant 0's planes, x-projection fetched by LDS-DMA
        return torch.stack([split_f16(whh[0]), split_f16(whh[1])]).contiguous()
    if variant >= 4:            # (> 4: timing-only forms of the experiments build, same planes)
        # the software-pipelined kernel: every gate row carries its activation scale (LSTM_GATE_SCALE: an accumulator
        # is then the exp2 argument), and the contraction index is re-ordered so that each half of K holds two of a
        # lane's four cells: column k' = 64 a + 2 p + e  <-  hidden unit u = 4 p + 2 a + e
        scale = torch.tensor(LSTM_GATE_SCALE, dtype=torch.float64).view(1, 4, 1, 1)
        w = (whh.double().view(2, 4, 128, 128) * scale).float().view(2, 512, 128)
        w = w[:, :, lstm_k_order()].contiguous()
        return torch.stack([split_f16(w[0], "lstm.weight_hh (scaled)"), split_f16(w[1], "lstm.weight_hh (scaled)")]).contiguous()
    sh = {1: 0, 2: 8}[variant]
    log2e = 1.44269504088896341
    scale = torch.full((4, 1, 1), -log2e, dtype=torch.float64)
    scale[2] = -2.0 * log2e                                   # PyTorch gate order i, f, g, o
    w = (whh.double().view(2, 4, 128, 128) * scale[None] * float(2 ** sh)).float().view(2, 512, 128)
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=1).view(torch.int16).contiguous()


# variant 4: exp(-x) = exp2(LSTM_GATE_SCALE x) for the gates i, f, o (sigmoid) and exp(-2x) for g (tanh), PyTorch's gate
# order i, f, g, o; folded into W_ih, the biases and W_hh of a variant-4 engine
LSTM_GATE_SCALE = (-1.44269504088896341, -1.44269504088896341, -2.88539008177792681, -1.44269504088896341)


def lstm_k_order() -> torch.Tensor:
    """hidden unit held by column k' of a variant-4 ``W_hh`` plane (and of ``h_t`` in the kernel's LDS)."""
    k = torch.arange(128)
    return 4 * ((k & 63) >> 1) + 2 * (k >> 6) + (k & 1)


def lstm_scale_gx(t: torch.Tensor, unit_major: bool = True) -> torch.Tensor:
    """rows of a stacked ``[1024][...]`` x-projection operand (weights or bias; row = dir*512 + unit*4 + gate when
    ``unit_major``, else dir*512 + gate*128 + unit) times the activation scale of their gate (variant 4)."""
    sc = torch.tensor(LSTM_GATE_SCALE, dtype=torch.float64)
    rows = torch.arange(t.shape[0])
    g = (rows & 3) if unit_major else ((rows % 512) // 128)
    shape = (-1,) + (1,) * (t.dim() - 1)
    return (t.double() * sc[g].view(shape)).float()


THROUGHPUT_LSTM_VARIANT = 4      # k_lstm_mfma.hip, the software-pipelined form: what a throughput engine runs unless told otherwise
RECURRENCES = ("valu", "0", "1", "2", "3", "4")


def lstm_variant_of(recurrence) -> int:
    """``recurrence`` ("valu" | "0" | "3" | "4"; "1" / "2": experiments build) -> -1 (one chain per CU on the f32
    vector units, k_lstm.hip) or the matrix-core variant of k_lstm_mfma.hip (``lstm_whh_planes``)."""
    r = "valu" if recurrence is None else str(recurrence)
    if r not in RECURRENCES:
        raise ValueError(f"recurrence={recurrence!r}: expected one of {RECURRENCES}")
    v = -1 if r == "valu" else int(r)
    if v in (1, 2) and not _lib.EXPERIMENTS:
        raise ValueError(f"recurrence={r}: matrix-core recurrence variants 1 / 2 exist in the experiments build only "
                         "(DZ_EXPERIMENTS=1); the shipped library has valu, 0, 3 and 4")
    return v


def _pad2(w: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    out = torch.zeros(rows, cols, dtype=torch.float32)
    out[: w.shape[0], : w.shape[1]] = w
    return out


def _pad1(v: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.float32)
    out[: v.shape[0]] = v
    return out


def _conv_pack(w: torch.Tensor, cin_pad: int, n_pad: int, k_pad: int) -> torch.Tensor:
    """Conv1d weight [co][ci][tap] -> [n_pad][k_pad] with k = tap*cin_pad + ci."""
    co, ci, taps = w.shape
    t = torch.zeros(co, taps, cin_pad, dtype=torch.float32)
    t[:, :, :ci] = w.float().permute(0, 2, 1)
    return _pad2(t.reshape(co, taps * cin_pad), n_pad, k_pad)


class _Packed:
    """Keeps the device tensors alive and exposes their addresses."""

    def __init__(self, device: torch.device):
        self.device = device
        self.tensors: List[torch.Tensor] = []

    def put(self, t: torch.Tensor) -> int:
        d = t.detach().to(dtype=torch.float32).contiguous().to(self.device)
        self.tensors.append(d)
        return d.data_ptr()

    def put_split(self, t: torch.Tensor, name: Optional[str] = None, kb: bool = False) -> int:
        """The matrix as two f16 planes (hi, lo * 2^11) for the split-f16 GEMM path; ``kb``: in the kb-major
        order of the layers that run on ``k_gemm_pre.hip`` / ``k_mlp_head.hip`` (``kb_major``)."""
        d = split_f16(t, name)
        # (only the experiments build's generation 2 / 3 GEMM has this limit: the shipped k_gemm_pre.hip keeps
        # two accumulators and takes any weight split_f16 accepts)
        if kb and _lib.exp_env("DZ_GEMM_GEN", "1") in ("2", "3") and t.numel() and float(t.detach().abs().max()) >= KB_WEIGHT_LIMIT:
            # k_gemm_g2.hip multiplies the hi plane of a weight fragment by 2^11 in f16 (one accumulator per
            # fragment): exact while |w| < 32, infinite beyond
            raise ValueError(f"{name or 'matrix'}: |weight| up to {float(t.detach().abs().max()):g} >= {KB_WEIGHT_LIMIT:g} "
                             "cannot be scaled by 2^11 inside the f16 range (k_gemm_g2.hip); load the model with "
                             "precision=\"f32\"")
        d = (kb_major(d) if kb else d).to(self.device)
        self.tensors.append(d)
        return d.data_ptr()

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors)


def _pack_sincnet(sd: Dict[str, torch.Tensor], pk: _Packed, prefix: str = "sincnet.",
                  split: bool = False) -> _lib.SincNetWeights:
    g = lambda k: sd[prefix + k].detach().cpu()
    filt = sinc_filters(g("conv1d.0.filterbank.low_hz_"), g("conv1d.0.filterbank.band_hz_"),
                        g("conv1d.0.filterbank.window_"), g("conv1d.0.filterbank.n_"))
    assert filt.shape == (80, 251)
    w = _lib.SincNetWeights()
    w.wav_gamma = float(g("wav_norm1d.weight").reshape(-1)[0])
    w.wav_beta = float(g("wav_norm1d.bias").reshape(-1)[0])
    w.filt = pk.put(fold_sinc_filters(filt))
    import os
    if split and _lib.exp_env("DZ_CONV0_SPLIT", "1") != "0":
        # the unfolded bank, zero padded to [96][256], as f16 planes for the matrix-core kernel
        w.filt_split = pk.put_split(_pad2(filt, 96, 256), prefix + "sinc filter bank")
    w.in0_g, w.in0_b = pk.put(g("norm1d.0.weight")), pk.put(g("norm1d.0.bias"))
    w.w1 = pk.put(_conv_pack(g("conv1d.1.weight"), 80, 64, 416))
    if split:
        w.w1_split = pk.put_split(_conv_pack(g("conv1d.1.weight"), 80, 64, 416), prefix + "conv1d.1")
        w.w2_split = pk.put_split(_conv_pack(g("conv1d.2.weight"), 64, 64, 320), prefix + "conv1d.2")
    w.b1 = pk.put(_pad1(g("conv1d.1.bias"), 64))
    w.in1_g, w.in1_b = pk.put(_pad1(g("norm1d.1.weight"), 64)), pk.put(_pad1(g("norm1d.1.bias"), 64))
    w.w2 = pk.put(_conv_pack(g("conv1d.2.weight"), 64, 64, 320))
    w.b2 = pk.put(_pad1(g("conv1d.2.bias"), 64))
    w.in2_g, w.in2_b = pk.put(_pad1(g("norm1d.2.weight"), 64)), pk.put(_pad1(g("norm1d.2.bias"), 64))
    return w


class PackedConv0Pair:
    """Operands of ``dz_sinc_conv0_pair`` (csrc/k_front.hip): the sinc banks of the segmentation and the embedding
    network as ONE f16x3 bank of 4 x 48 slots — wave ``w`` of the kernel owns slots ``48 w .. 48 w + 47``, of which
    the first 40 hold filters ``40 w .. 40 w + 39`` of (seg 0..79 | emb 0..79) and the rest are zero — plus, per
    slot, ``beta_net * sum_k filt[k]``: with xh the un-affine InstanceNorm1d(1) of the window,
    ``conv(gamma xh + beta) = gamma conv(xh) + beta sum(filt)``, so one split of ``xh`` serves both networks."""

    def __init__(self, seg_sd: Dict[str, torch.Tensor], emb_sd: Dict[str, torch.Tensor], device: torch.device,
                 seg_prefix: str = "sincnet.", emb_prefix: str = "sincnet."):
        banks, betas = [], []
        for sd, prefix in ((seg_sd, seg_prefix), (emb_sd, emb_prefix)):
            g = lambda k: sd[prefix + k].detach().cpu()
            filt = sinc_filters(g("conv1d.0.filterbank.low_hz_"), g("conv1d.0.filterbank.band_hz_"),
                                g("conv1d.0.filterbank.window_"), g("conv1d.0.filterbank.n_"))
            assert filt.shape == (80, 251)
            banks.append(filt)
            betas.append(float(g("wav_norm1d.bias").reshape(-1)[0]))
        full = torch.cat(banks, 0)                                   # (160, 251): seg | emb
        slots = torch.zeros(192, 256, dtype=torch.float32)
        bsum = torch.zeros(192, dtype=torch.float64)
        for w in range(4):
            slots[48 * w: 48 * w + 40, :251] = full[40 * w: 40 * w + 40]
            bsum[48 * w: 48 * w + 40] = betas[w // 2] * full[40 * w: 40 * w + 40].double().sum(1)
        self.planes = split_f16(slots, "sinc filter bank (pair)").to(device)      # int16 [2? see split_f16][192][256]
        self.bsum = bsum.float().to(device)


class PackedSegmentation:
    """``dz_seg_weights`` + the tensors behind it.

    ``struct`` is what the synchronous blocks API runs: the recurrence named by ``recurrence`` ("valu" by default: one
    chain per CU, the shortest layer).  ``struct_for(r)`` is the same network with another recurrence kernel (built on
    first use, cached): the W_hh planes of that matrix-core variant and, for variant 4, an x-projection whose rows carry
    the gates' activation scales; everything else is shared, not copied.  ``struct_throughput`` = what a throughput
    engine (``StreamBatch`` with >= 64 streams per step, several steps in flight) creates its handles from."""

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, powerset: bool = False,
                 num_speakers: int | None = None, precision: str = "f32", recurrence: Optional[str] = None):
        assert precision in PRECISIONS, precision
        split = precision == "f16x3"
        pk = _Packed(device)
        g = lambda k: sd[k].detach().cpu().float()
        w = _lib.SegWeights()
        w.sinc = _pack_sincnet(sd, pk, split=split)
        self._split, self._lstm, self._wih0_kb = split, [], {}
        for layer in range(4):
            # rows of the stacked W_ih (and the bias) go unit-major, dir*512 + unit*4 + gate, so the
            # x-projection GEMM writes the four gates of a unit next to each other and the recurrence
            # reads them as one 16-byte word (PyTorch's order is dir*512 + gate*128 + unit)
            um = lambda t: t.reshape(2, 4, 128, *t.shape[1:]).transpose(1, 2).reshape(t.shape).contiguous()
            wih = um(torch.cat([g(f"lstm.weight_ih_l{layer}"), g(f"lstm.weight_ih_l{layer}_reverse")], 0))
            bias = um(torch.cat([g(f"lstm.bias_ih_l{layer}") + g(f"lstm.bias_hh_l{layer}"),
                                 g(f"lstm.bias_ih_l{layer}_reverse") + g(f"lstm.bias_hh_l{layer}_reverse")], 0))
            whh = torch.stack([g(f"lstm.weight_hh_l{layer}"), g(f"lstm.weight_hh_l{layer}_reverse")], 0)
            assert whh.shape == (2, 512, 128)
            self._lstm.append((wih, bias, whh))
            w.wih[layer], sp, w.bih[layer] = self._put_proj(pk, layer, wih, bias, "")
            if split:
                w.wih_split[layer] = sp
            w.whh[layer] = pk.put(whh)
        w.lin0_w, w.lin0_b = pk.put(g("linear.0.weight")), pk.put(g("linear.0.bias"))
        w.lin1_w, w.lin1_b = pk.put(g("linear.1.weight")), pk.put(g("linear.1.bias"))
        if split:
            w.lin0_split = pk.put_split(g("linear.0.weight"), "linear.0", kb=True)
            w.lin1_split = pk.put_split(g("linear.1.weight"), "linear.1", kb=True)
        cls_w, cls_b = g("classifier.weight"), g("classifier.bias")
        ncls = cls_w.shape[0]
        w.cls_w, w.cls_b = pk.put(_pad2(cls_w, 64, 128)), pk.put(_pad1(cls_b, 64))
        w.num_classes = ncls
        w.powerset = 1 if powerset else 0
        if powerset:
            # classes = 1 + S + S(S-1)/2  ->  S
            s = num_speakers or int(round((-1 + math.sqrt(1 + 8 * (ncls - 1))) / 2))
            w.num_speakers = s
        else:
            w.num_speakers = ncls
        if split:
            w.wih0_split_kb = self._wih0_kb[""]
        self.pack = pk
        self.num_speakers = int(w.num_speakers)
        self._structs = {"valu": w}
        self.recurrence = "valu" if recurrence is None else str(recurrence)
        self.struct = self.struct_for(self.recurrence)

    def _put_proj(self, pk, layer, wm, bv, tag):
        """-> (f32 W_ih, its split planes or None, bias) of one layer on the device"""
        kpad = 64 if layer == 0 else 256
        # layer 0 runs on k_gemm_split.hip (row-major planes), layers 1..3 on k_gemm_pre.hip (kb-major)
        sp = pk.put_split(_pad2(wm, 1024, kpad), f"lstm.weight_ih_l{layer}{tag}", kb=layer > 0) if self._split else None
        if layer == 0 and self._split:      # ... and kb-major too: the first projection behind the norm + split pass (round 6)
            self._wih0_kb[tag] = pk.put_split(_pad2(wm, 1024, kpad), f"lstm.weight_ih_l0{tag} (kb)", kb=True)
        return pk.put(_pad2(wm, 1024, kpad)), sp, pk.put(bv)

    def struct_for(self, recurrence: Optional[str]):
        """The weight struct whose recurrence runs on ``recurrence`` ("valu" | "0" | "3" | "4"); exact f32 has only
        "valu" (the matrix-core kernels are split-f16 arithmetic)."""
        r = "valu" if recurrence is None else str(recurrence)
        v = lstm_variant_of(r)
        if not self._split:
            v, r = -1, "valu"
        got = self._structs.get(r)
        if got is None:
            got = _lib.SegWeights.from_buffer_copy(self._structs["valu"])
            for layer, (wih, bias, whh) in enumerate(self._lstm):
                d = lstm_whh_planes(whh, v).to(self.pack.device)        # [dir][plane][512][128] f16
                self.pack.tensors.append(d)
                got.whh_split[layer] = d.data_ptr()
                if v == 4:        # its x-projection carries the gates' activation scales
                    got.wih[layer], got.wih_split[layer], got.bih[layer] = self._put_proj(
                        self.pack, layer, lstm_scale_gx(wih), lstm_scale_gx(bias), " (scaled)")
                    if layer == 0:
                        got.wih0_split_kb = self._wih0_kb[" (scaled)"]
            got.lstm_variant = v
            self._structs[r] = got
        return got

    @property
    def struct_throughput(self):
        """A THROUGHPUT engine's weights (StreamBatch with many streams per launch and several steps in flight): the
        recurrence on the matrix cores, 16 chains per workgroup — a seventh of the CU-time of the one-chain-per-CU
        kernel at twice its latency — unless the model was built with an explicit recurrence."""
        if not self._split or self.recurrence != "valu":
            return self.struct
        return self.struct_for(str(THROUGHPUT_LSTM_VARIANT))


class PackedEmbedding:
    """``dz_emb_weights`` + the tensors behind it."""

    TDNN = [(64, 512, 512), (512, 512, 512), (512, 512, 512), (512, 512, 512), (512, 1500, 1536)]

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32",
                 weight_interp: str = "linear"):
        """``weight_interp``: how StatsPool resamples the pooling weights to the feature frames — "linear"
        (``F.interpolate(mode="linear")``, pyannote.audio 2.x .. 3.0) or "nearest" (pyannote.audio >= 3.1)."""
        assert precision in PRECISIONS, precision
        if weight_interp not in ("linear", "nearest"):
            raise ValueError(f"weight_interp={weight_interp!r}: expected 'linear' or 'nearest'")
        split = precision == "f16x3"
        pk = _Packed(device)
        g = lambda k: sd[k].detach().cpu().float()
        w = _lib.EmbWeights()
        w.pool_nearest = int(weight_interp == "nearest")
        w.sinc = _pack_sincnet(sd, pk, split=split)
        for i, (cin_pad, cout, npad) in enumerate(self.TDNN):
            cw = g(f"tdnns.{3 * i}.weight")
            assert cw.shape[0] == cout
            k = cw.shape[2] * cin_pad
            w.tw[i] = pk.put(_conv_pack(cw, cin_pad, npad, (k + 31) // 32 * 32))
            if split:
                # tdnn1 runs on k_gemm_split.hip (row-major planes), tdnn2..5 on k_gemm_pre.hip (kb-major)
                w.tw_split[i] = pk.put_split(_conv_pack(cw, cin_pad, npad, (k + 31) // 32 * 32), f"tdnn{i + 1}", kb=i > 0)
                if i == 0:      # ... and kb-major too: tdnn1 behind the norm + split pass (round 6)
                    w.tw0_split_kb = pk.put_split(_conv_pack(cw, cin_pad, npad, (k + 31) // 32 * 32), "tdnn1 (kb)", kb=True)
            w.tb[i] = pk.put(_pad1(g(f"tdnns.{3 * i}.bias"), npad))
            bn = f"tdnns.{3 * i + 2}."
            scale = g(bn + "weight") / torch.sqrt(g(bn + "running_var") + BN_EPS)
            shift = g(bn + "bias") - g(bn + "running_mean") * scale
            w.ts[i], w.th[i] = pk.put(_pad1(scale, npad)), pk.put(_pad1(shift, npad))
        ew = g("embedding.weight")
        assert ew.shape == (512, 3000), "only the 512-d x-vector head is built"
        w.emb_w, w.emb_b = pk.put(_pad2(ew, 512, 3008)), pk.put(g("embedding.bias"))
        w.dimension = 512
        self.struct, self.pack = w, pk


def _pack_ecapa_network(sd: Dict[str, torch.Tensor], pk: "_Packed", w, split: bool) -> None:
    """ECAPA_TDNN(80 -> 1024 x 4 -> 3072 -> 192) into ``w`` (a ``dz_ecapa_weights``: block0 .. fc, zeros), for the two
    models with this network: ``PackedEcapa`` and ``PackedEcapaMel``."""
    g = lambda k: sd[k].detach().cpu().float()

    def bn(prefix, npad):
        scale = g(prefix + ".norm.weight") / torch.sqrt(g(prefix + ".norm.running_var") + BN_EPS)
        shift = g(prefix + ".norm.bias") - g(prefix + ".norm.running_mean") * scale
        return _pad1(scale, npad), _pad1(shift, npad)

    def layer(dst, prefix, cin_pad, npad, kpad, norm=True, weight=None, wide=False, kb=False):
        cw = g(prefix + ".conv.weight") if weight is None else weight
        dst.w = pk.put(_conv_pack(cw, cin_pad, npad, kpad))
        if wide and split:   # also as split-f16 planes: the layer runs on k_gemm_split.hip, or (kb: planes in
            #                  kb-major order) with pre-split activations on k_gemm_pre.hip
            dst.wsplit = pk.put_split(_conv_pack(cw, cin_pad, npad, kpad), prefix, kb=kb)
        dst.b = pk.put(_pad1(g(prefix + ".conv.bias"), npad))
        if norm:
            sc, sh = bn(prefix.rsplit(".conv", 1)[0] + ".norm", npad)
            dst.s, dst.h = pk.put(sc), pk.put(sh)

    layer(w.block0, "blocks.0.conv", 80, 1024, 416, wide=True)
    for i in range(3):
        p, b = f"blocks.{i + 1}", w.ser[i]
        layer(b.tdnn1, p + ".tdnn1.conv", 1024, 1024, 1024, wide=True, kb=True)
        for j in range(7):
            layer(b.res[j], p + f".res2net_block.blocks.{j}.conv", 128, 128, 384, wide=True)
        layer(b.tdnn2, p + ".tdnn2.conv", 1024, 1024, 1024, wide=True, kb=True)
        layer(b.se1, p + ".se_block.conv1", 1024, 128, 1024, norm=False)
        layer(b.se2, p + ".se_block.conv2", 128, 1024, 128, norm=False)
    layer(w.mfa, "mfa.conv", 3072, 3072, 3072, wide=True, kb=True)
    aw = g("asp.tdnn.conv.conv.weight")                           # (128, 9216, 1)
    layer(w.asp_tdnn, "asp.tdnn.conv", 3072, 128, 3072, weight=aw[:, :3072], wide=True)
    w.asp_wms = pk.put(aw[:, 3072:, 0].contiguous())             # (128, 6144)
    layer(w.asp_conv, "asp.conv", 128, 3072, 128, norm=False, wide=True)
    sc, sh = bn("asp_bn", 6144)
    fw, fb = g("fc.conv.weight")[:, :, 0], g("fc.conv.bias")     # (192, 6144)
    w.fc.w = pk.put((fw * sc[None, :]).contiguous())
    w.fc.b = pk.put(fb + fw @ sh)
    w.zeros = pk.put(torch.zeros(6144))


class PackedEcapa:
    """``dz_ecapa_weights`` + the tensors behind it (speechbrain ECAPA_TDNN checkpoint keys:
    ``blocks.0.conv.conv.weight`` ... ``fc.conv.weight``).

    * the Hamming window is folded into the DFT matrix, so the STFT is one GEMM over the
      overlapping 400-sample rows of the signal (hop 160);
    * BatchNorm1d (eval) after ReLU is folded to scale / shift; ``asp_bn`` is folded into ``fc``;
    * the 9216-wide attention TDNN is split into the 3072 columns that see x and the 6144 columns
      that see the per-row global (mean | std), which become a per-row bias."""

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32"):
        assert precision in PRECISIONS, precision
        split = precision == "f16x3"
        pk = _Packed(device)
        w = _lib.EcapaWeights()
        # ---- features ------------------------------------------------------------------
        w.dft = pk.put(_pad2(dft_matrices().float(), 448, 416))
        if split:
            w.dft_split = pk.put_split(_pad2(dft_matrices().float(), 512, 416), "windowed DFT")
        w.mel = pk.put(_pad2(ecapa_mel_filterbank().t().contiguous(), 128, 224))
        # ---- network -------------------------------------------------------------------
        _pack_ecapa_network(sd, pk, w, split)
        self.struct, self.pack = w, pk


# The feature settings of speechbrain/spkrec-ecapa-voxceleb-mel-spec (its hyperparams.yaml, recalled: DESIGN.md 4.15
# (R)) in torchaudio.transforms.MelSpectrogram's names.  f_min / f_max only shape the packed mel bank and may differ;
# the kernels and the packer are built for the values of ECAPA_MEL_BUILT and every other value of those is refused by name.
ECAPA_MEL_FEATURES = {"sample_rate": 16000, "n_fft": 1024, "win_length": 1024, "hop_length": 256, "f_min": 0.0,
                      "f_max": 8000.0, "n_mels": 80, "power": 1, "normalized": False, "norm": "slaney",
                      "mel_scale": "slaney"}
ECAPA_MEL_BUILT = ("sample_rate", "n_fft", "win_length", "hop_length", "n_mels", "power", "normalized", "norm",
                   "mel_scale")
ECAPA_MEL_MIN_NUM_SAMPLES = 1024


def ecapa_mel_features(**given) -> dict:
    """``ECAPA_MEL_FEATURES`` with ``given`` laid over it; ValueError naming the setting for an unknown one or a value
    the kernels are not built for."""
    out = dict(ECAPA_MEL_FEATURES)
    for k, v in given.items():
        if k not in out:
            raise ValueError(f"ecapa-mel: unknown feature setting {k!r} (known: {sorted(out)})")
        want = out[k]
        if isinstance(want, bool):
            v = v if isinstance(v, bool) else str(v).strip().lower() in ("true", "1", "yes")
        elif isinstance(want, (int, float)):
            v = type(want)(float(v))
        else:
            v = None if v is None or str(v).strip().lower() in ("none", "null", "~") else str(v).strip().strip("\"'")
        if k in ECAPA_MEL_BUILT and v != want:
            raise ValueError(f"ecapa-mel: {k}={v!r} — the HIP front end is built for {k}={want!r} only")
        out[k] = v
    if not 0.0 <= out["f_min"] < out["f_max"] <= out["sample_rate"] / 2:
        raise ValueError(f"ecapa-mel: f_min={out['f_min']!r} / f_max={out['f_max']!r} outside 0 <= f_min < f_max <= Nyquist")
    return out


def ecapa_mel_spec_dft() -> torch.Tensor:
    """The STFT of the mel-spectrogram ECAPA as ONE real GEMM operand, (2 * 513, 1024) f64: rows 0 .. 512 =
    cos(2 pi k n / 1024) w[n], rows 513 .. 1025 = sin(...) w[n], w the periodic Hann window of 1024 samples:
    frame @ rows.T = (Re, -Im) of rfft(frame * w).  k n is reduced modulo 1024 in integers first, so the angle is exact
    to its last bit, and the zeros of the sine and the cosine (multiples of a quarter turn) are exact zeros."""
    n = torch.arange(1024, dtype=torch.int64)
    k = torch.arange(513, dtype=torch.int64)[:, None]
    r = torch.remainder(k * n[None, :], 1024)
    ang = 2.0 * math.pi * r.to(torch.float64) / 1024.0
    cos = torch.where(r % 512 == 256, torch.zeros((), dtype=torch.float64), torch.cos(ang))
    sin = torch.where(r % 512 == 0, torch.zeros((), dtype=torch.float64), torch.sin(ang))
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    return torch.cat([cos * win, sin * win], 0)


def ecapa_mel_spec_filterbank(f_min: float = 0.0, f_max: float = 8000.0) -> torch.Tensor:
    """torchaudio's melscale_fbanks(513, f_min, f_max, 80, 16000, "slaney", "slaney") as (80, 513) f64
    (``slaney_mel_filterbank``)."""
    return slaney_mel_filterbank(80, 1024, 16000, float(f_min), float(f_max))


class PackedEcapaMel:
    """``dz_ecm_weights`` + the tensors behind it: ``PackedEcapa``'s network (the same checkpoint keys, packed by the
    same code), the Hann-windowed DFT of 1024 samples built in float64 as one GEMM operand (1152 x 1024, for "f16x3"
    also as split-f16 planes) and the slaney mel bank (128 x 544, exact f32).  ``features``: ``ecapa_mel_features``."""

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32",
                 min_num_samples: int = ECAPA_MEL_MIN_NUM_SAMPLES, **features):
        assert precision in PRECISIONS, precision
        split = precision == "f16x3"
        self.features = ecapa_mel_features(**features)
        if int(min_num_samples) <= 512:
            raise ValueError(f"ecapa-mel: min_num_samples={min_num_samples} — the centred STFT reflects 512 samples, "
                             "which needs more than 512")
        pk = _Packed(device)
        w = _lib.EcmWeights()
        dft = _pad2(ecapa_mel_spec_dft().float(), 1152, 1024)
        w.dft = pk.put(dft)
        if split:
            w.dft_split = pk.put_split(dft, "Hann-windowed DFT (1024)")
        bank = ecapa_mel_spec_filterbank(self.features["f_min"], self.features["f_max"])
        w.mel = pk.put(_pad2(bank.float(), 128, 544))
        w.min_num_samples = int(min_num_samples)
        _pack_ecapa_network(sd, pk, w.net, split)
        self.struct, self.pack = w, pk


class PackedSbXvector:
    """``dz_sbx_weights`` + the tensors behind it (speechbrain ``Xvector`` checkpoint keys of
    spkrec-xvect-voxceleb: ``blocks.{0,3,6,9,12}.conv.{weight,bias}``, ``blocks.{2,5,8,11,14}.norm.{weight,bias,
    running_mean,running_var}``, ``blocks.16.w.{weight,bias}``).

    * the Fbank is ECAPA's (windowed DFT as one GEMM operand) with a 24-bin mel bank;
    * TDNN weights as ``[Npad][Kpad]`` with ``k = tap * Cin + c`` (channels-last activations), layer 5 padded
      1500 -> 1536 rows; BatchNorm1d (eval, eps 1e-5) after the LeakyReLU folded to scale / shift;
    * for "f16x3" the DFT and the five TDNN layers also as row-major split-f16 planes (k_gemm_split.hip); the mel
      bank and Linear(3000, 512) stay exact f32."""

    CONV_KEYS = (0, 3, 6, 9, 12)
    # (Cin, taps, Npad, Kpad) of the five TDNN layers
    TDNN = ((24, 5, 512, 128), (512, 3, 512, 1536), (512, 3, 512, 1536), (512, 1, 512, 512), (512, 1, 1536, 512))

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32"):
        assert precision in PRECISIONS, precision
        split = precision == "f16x3"
        pk = _Packed(device)
        g = lambda k: sd[k].detach().cpu().float()
        w = _lib.SbxWeights()
        w.dft = pk.put(_pad2(dft_matrices().float(), 448, 416))
        if split:
            w.dft_split = pk.put_split(_pad2(dft_matrices().float(), 512, 416), "windowed DFT")
        w.mel = pk.put(_pad2(ecapa_mel_filterbank(n_mels=24).t().contiguous(), 64, 224))
        for i, (cin, taps, npad, kpad) in enumerate(self.TDNN):
            c, n = f"blocks.{self.CONV_KEYS[i]}.conv", f"blocks.{self.CONV_KEYS[i] + 2}.norm"
            cw = g(c + ".weight")
            if tuple(cw.shape[1:]) != (cin, taps):
                raise ValueError(f"{c}.weight: shape {tuple(cw.shape)}, expected (Cout, {cin}, {taps}) "
                                 "(speechbrain spkrec-xvect-voxceleb geometry)")
            m = _conv_pack(cw, cin, npad, kpad)
            L = w.tdnn[i]
            L.w, L.b = pk.put(m), pk.put(_pad1(g(c + ".bias"), npad))
            if split:
                L.wsplit = pk.put_split(m, f"tdnn{i + 1}")
            scale = g(n + ".weight") / torch.sqrt(g(n + ".running_var") + BN_EPS)
            shift = g(n + ".bias") - g(n + ".running_mean") * scale
            L.s, L.h = pk.put(_pad1(scale, npad)), pk.put(_pad1(shift, npad))
        lw = g("blocks.16.w.weight")
        if tuple(lw.shape) != (512, 3000):
            raise ValueError(f"blocks.16.w.weight: shape {tuple(lw.shape)}, expected (512, 3000)")
        w.lin_w, w.lin_b = pk.put(_pad2(lw, 512, 3008)), pk.put(g("blocks.16.w.bias"))
        w.zeros = pk.put(torch.zeros(1536))
        self.struct, self.pack = w, pk


def ecapa_mel_filterbank(n_mels: int = 80, n_fft: int = 400, sample_rate: int = 16000) -> torch.Tensor:
    """speechbrain Filterbank (triangular, f_min = 0, f_max = sr / 2): (n_fft // 2 + 1, n_mels)."""
    to_mel = lambda hz: 2595.0 * math.log10(1.0 + hz / 700.0)
    mel = torch.linspace(to_mel(0.0), to_mel(sample_rate / 2), n_mels + 2)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    band = (hz[1:] - hz[:-1])[:-1]
    f_central = hz[1:-1]
    all_freqs = torch.linspace(0, sample_rate // 2, n_fft // 2 + 1)
    slope = (all_freqs.repeat(n_mels, 1) - f_central[:, None]) / band[:, None]
    return torch.max(torch.zeros(1), torch.min(slope + 1.0, -slope + 1.0)).t().contiguous()


def kaldi_mel_banks(num_bins: int = 80, n_fft: int = 512, sample_rate: int = 16000, low_freq: float = 20.0) -> torch.Tensor:
    """kaldi's triangular mel bank (torchaudio.compliance.kaldi.get_mel_banks with high_freq = Nyquist, no VTLN),
    mel = 1127 ln(1 + f / 700), as the (num_bins, n_fft / 2 + 1) matrix kaldi.fbank multiplies the power spectrum
    with: the n_fft / 2 FFT bins below Nyquist, then a zero column for the Nyquist bin.  Computed in float64."""
    mel = lambda f: 1127.0 * torch.log1p(torch.as_tensor(f, dtype=torch.float64) / 700.0)
    nyq = sample_rate / 2.0
    lo, hi = mel(low_freq), mel(nyq)
    delta = (hi - lo) / (num_bins + 1)
    b = torch.arange(num_bins, dtype=torch.float64)[:, None]
    left, center, right = lo + b * delta, lo + (b + 1) * delta, lo + (b + 2) * delta
    m = mel(sample_rate / n_fft * torch.arange(n_fft // 2, dtype=torch.float64))[None, :]
    up, down = (m - left) / (center - left), (right - m) / (right - center)
    banks = torch.clamp(torch.minimum(up, down), min=0.0)
    return torch.cat([banks, torch.zeros(num_bins, 1, dtype=torch.float64)], dim=1)


# BasicBlocks per layer of ResNet34 and their channel counts
WESPEAKER_BLOCKS = (3, 4, 6, 3)


def fold_conv_bn(w: torch.Tensor, bn: Dict[str, torch.Tensor], eps: float = BN_EPS):
    """Conv2d weight (Cout, Cin, kh, kw) without bias + BatchNorm2d (eval) -> (weight, bias) of the folded
    convolution, in the dtype of ``w``."""
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + eps)
    return w * scale[:, None, None, None], bn["bias"] - bn["running_mean"] * scale


def wsp_conv_matrix(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight (Cout, Cin, kh, kw) -> (Cout, kh kw Cin) with k = (kh 3 + kw) Cin + c: the tap-major K axis of
    the implicit GEMM over channels-last activations (k_conv2d.hip)."""
    co = w.shape[0]
    return w.permute(0, 2, 3, 1).reshape(co, -1).contiguous()


class PackedWeSpeaker:
    """``dz_wsp_weights`` + the tensors behind it (pyannote.audio 3.1 ``WeSpeakerResNet34`` checkpoint keys:
    ``resnet.conv1.weight``, ``resnet.bn1.*``, ``resnet.layer{1..4}.{i}.{conv1,bn1,conv2,bn2}.*``,
    ``resnet.layer{2,3,4}.0.shortcut.{0,1}.*``, ``resnet.seg_1.*``).

    * every BatchNorm2d (eval, eps 1e-5) is folded into the convolution before it: weight x scale, bias = shift;
    * weights as ``[Cout][(kh 3 + kw) Cin + c]`` f32 and, for "f16x3", also as split-f16 planes (the 3x3 / 1x1
      convolutions of the four layers; conv1 has Cin = 1 and runs on a direct f32 kernel);
    * the kaldi mel bank (80, 257)."""

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32"):
        assert precision in PRECISIONS, precision
        split = precision == "f16x3"
        pk = _Packed(device)
        g = lambda k: sd[k].detach().cpu().float()
        bnd = lambda p: {n: g(f"{p}.{n}") for n in ("weight", "bias", "running_mean", "running_var")}
        w = _lib.WspWeights()

        def conv(dst, wkey, bnprefix, name, planes=True):
            fw, fb = fold_conv_bn(g(wkey), bnd(bnprefix))
            m = wsp_conv_matrix(fw)
            dst.w, dst.b = pk.put(m), pk.put(fb)
            if split and planes:
                dst.wsplit = pk.put_split(m, name)

        w.mel = pk.put(kaldi_mel_banks().float())
        conv(w.conv1, "resnet.conv1.weight", "resnet.bn1", "conv1", planes=False)
        bi = 0
        for li, nb in enumerate(WESPEAKER_BLOCKS):
            for j in range(nb):
                p = f"resnet.layer{li + 1}.{j}"
                blk = w.block[bi]
                conv(blk[0], p + ".conv1.weight", p + ".bn1", p + ".conv1")
                conv(blk[1], p + ".conv2.weight", p + ".bn2", p + ".conv2")
                if p + ".shortcut.0.weight" in sd:
                    conv(blk[2], p + ".shortcut.0.weight", p + ".shortcut.1", p + ".shortcut")
                bi += 1
        w.seg_w = pk.put(g("resnet.seg_1.weight"))
        w.seg_b = pk.put(g("resnet.seg_1.bias"))
        self.struct, self.pack = w, pk


# --------------------------------------------------------------------------- #
# speechbrain ResNet (speechbrain/spkrec-resnet-voxceleb)
# --------------------------------------------------------------------------- #
# module prefixes of speechbrain.lobes.models.ResNet.ResNet's state dict
SB_RESNET_KEYS = {
    "stem": "conv1", "stem_bn": "bn1",
    "conv1": "layer{L}.{i}.conv1", "bn1": "layer{L}.{i}.bn1", "conv2": "layer{L}.{i}.conv2", "bn2": "layer{L}.{i}.bn2",
    "se1": "layer{L}.{i}.se.fc.0", "se2": "layer{L}.{i}.se.fc.2",
    "down": "layer{L}.{i}.downsample.0", "down_bn": "layer{L}.{i}.downsample.1",
    "att1": "attention.0", "att_bn": "attention.2", "att2": "attention.3",
    "norm_stats": "norm_stats", "fc": "fc_embed", "norm_embed": "norm_embed",
}
# what the loader recognises the state by
SB_RESNET_MARKERS = ("layer1.0.se.fc.0.weight", "fc_embed.weight")
SB_RESNET_STRIDES = (1, 2, 2, 2)        # hyperparams.yaml; not visible in the shapes where the width changes too
SB_RESNET_MIN_NUM_SAMPLES = 3           # what pyannote's bisection over [2, 8000] ends at when every length is accepted
SB_RESNET_MAX_BLOCKS = _lib.SBR_MAX_BLOCKS
_BN = ("weight", "bias", "running_mean", "running_var")


def sb_resnet_key(kind: str, L: int = 0, i: int = 0) -> str:
    return SB_RESNET_KEYS[kind].format(L=L, i=i)


def sb_resnet_shape(sd: Dict[str, torch.Tensor], strides=SB_RESNET_STRIDES) -> dict:
    """Widths, blocks per layer and squeeze-excitation widths read from the shapes of a speechbrain ResNet state;
    every tensor the packer reads is checked against them and a mismatch is refused by its key."""
    def need(key, shape):
        if key not in sd:
            raise ValueError(f"{key}: missing from the state (speechbrain ResNet)")
        got = tuple(sd[key].shape)
        if got != tuple(shape) and not (len(got) == len(shape) + 1 and got[-1] == 1 and got[:-1] == tuple(shape)):
            raise ValueError(f"{key}: shape {got}, expected {tuple(shape)}")

    def need_bn(prefix, n):
        for f in _BN:
            need(f"{prefix}.{f}", (n,))

    def gemm_width(key, c):
        if c not in (32, 64) and c % 128:
            raise ValueError(f"{key}: {c} channels; the 2-D convolution kernels take 32, 64 or a multiple of 128")
        if c > 1024:
            raise ValueError(f"{key}: {c} channels; the squeeze-excitation kernels take at most 1024")

    if len(strides) != 4 or any(s not in (1, 2) for s in strides):
        raise ValueError(f"strides={strides!r}: four strides of 1 or 2")
    k = sb_resnet_key
    if k("stem") + ".weight" not in sd:
        raise ValueError(f"{k('stem')}.weight: missing from the state (speechbrain ResNet)")
    c0 = int(sd[k("stem") + ".weight"].shape[0])
    need(k("stem") + ".weight", (c0, 1, 3, 3)); need(k("stem") + ".bias", (c0,)); need_bn(k("stem_bn"), c0)
    gemm_width(k("stem") + ".weight", c0)
    cin, f, widths, blocks, se = c0, 80, [], [], []
    for L in range(1, 5):
        n = 0
        while k("conv1", L, n) + ".weight" in sd:
            n += 1
        if n == 0:
            raise ValueError(f"{k('conv1', L, 0)}.weight: missing from the state (speechbrain ResNet)")
        c = int(sd[k("conv1", L, 0) + ".weight"].shape[0])
        gemm_width(k("conv1", L, 0) + ".weight", c)
        se.append([])
        for i in range(n):
            stride = strides[L - 1] if i == 0 else 1
            need(k("conv1", L, i) + ".weight", (c, cin, 3, 3)); need_bn(k("bn1", L, i), c)
            need(k("conv2", L, i) + ".weight", (c, c, 3, 3)); need_bn(k("bn2", L, i), c)
            if k("se1", L, i) + ".weight" not in sd:
                raise ValueError(f"{k('se1', L, i)}.weight: missing from the state (speechbrain ResNet)")
            cr = int(sd[k("se1", L, i) + ".weight"].shape[0])
            need(k("se1", L, i) + ".weight", (cr, c))
            if not 1 <= cr <= 1024:
                raise ValueError(f"{k('se1', L, i)}.weight: {cr} rows; the squeeze-excitation kernels take 1 .. 1024")
            need(k("se1", L, i) + ".bias", (cr,)); need(k("se2", L, i) + ".weight", (c, cr)); need(k("se2", L, i) + ".bias", (c,))
            has_down = k("down", L, i) + ".weight" in sd
            if (stride != 1 or cin != c) and not has_down:
                raise ValueError(f"{k('down', L, i)}.weight: missing, but the block has stride {stride} and widths {cin} -> {c}")
            if has_down:
                need(k("down", L, i) + ".weight", (c, cin, 1, 1)); need_bn(k("down_bn", L, i), c)
            se[-1].append(cr)
            cin = c
        f = (f - 1) // strides[L - 1] + 1
        widths.append(c); blocks.append(n)
    if sum(blocks) > SB_RESNET_MAX_BLOCKS:
        raise ValueError(f"{sum(blocks)} blocks; dz_sbr_weights holds {SB_RESNET_MAX_BLOCKS}")
    cf = f * cin
    need(k("att1") + ".weight", (128, cf)); need(k("att1") + ".bias", (128,)); need_bn(k("att_bn"), 128)
    need(k("att2") + ".weight", (cf, 128)); need(k("att2") + ".bias", (cf,))
    need_bn(k("norm_stats"), 2 * cf)
    need(k("fc") + ".weight", (256, 2 * cf)); need(k("fc") + ".bias", (256,)); need_bn(k("norm_embed"), 256)
    return {"stem": c0, "channels": tuple(widths), "block_sizes": tuple(blocks), "se": se, "strides": tuple(strides),
            "freq": f, "pooled": cf}


def sb_resnet_fold(sd: Dict[str, torch.Tensor], strides=SB_RESNET_STRIDES, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """Every matrix ``PackedSbResNet`` hands to the kernels, folded in ``dtype`` (the packer: float64, rounded once):
    ``stem.w|b`` ((C0, 9), k = kt 3 + kf), ``b{n}.conv1|conv2|down.w|b`` (``wsp_conv_matrix`` layout, time = kh),
    ``b{n}.se.w1t|b1|w2t|b2``, ``att1.w|b|s|h``, ``att2.w|b``, ``fc.w|b``.  The head's 2560 channels are re-ordered from
    speechbrain's c F4 + f (``transpose(2, 3).flatten(1, 2)``) to the activations' f C4 + c."""
    shape = sb_resnet_shape(sd, strides)
    g = lambda key: sd[key].detach().cpu().to(dtype)
    bnd = lambda p: {n: g(f"{p}.{n}") for n in _BN}
    k = sb_resnet_key
    out: Dict[str, torch.Tensor] = {}
    bn = bnd(k("stem_bn"))
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
    out["stem.w"] = (g(k("stem") + ".weight") * scale[:, None, None, None]).reshape(shape["stem"], 9).contiguous()
    out["stem.b"] = (g(k("stem") + ".bias") - bn["running_mean"]) * scale + bn["bias"]
    n = 0
    for L, nb in enumerate(shape["block_sizes"], start=1):
        for i in range(nb):
            for name, conv, norm in (("conv1", "conv1", "bn1"), ("conv2", "conv2", "bn2"), ("down", "down", "down_bn")):
                if k(conv, L, i) + ".weight" in sd:
                    fw, fb = fold_conv_bn(g(k(conv, L, i) + ".weight"), bnd(k(norm, L, i)))
                    out[f"b{n}.{name}.w"], out[f"b{n}.{name}.b"] = wsp_conv_matrix(fw), fb
            out[f"b{n}.se.w1t"] = g(k("se1", L, i) + ".weight").t().contiguous()
            out[f"b{n}.se.b1"] = g(k("se1", L, i) + ".bias")
            out[f"b{n}.se.w2t"] = g(k("se2", L, i) + ".weight").t().contiguous()
            out[f"b{n}.se.b2"] = g(k("se2", L, i) + ".bias")
            n += 1
    c4, f4, cf = shape["channels"][3], shape["freq"], shape["pooled"]
    perm = (torch.arange(c4)[None, :] * f4 + torch.arange(f4)[:, None]).reshape(-1)        # [f C4 + c] = c F4 + f
    bn = bnd(k("att_bn"))
    out["att1.w"] = g(k("att1") + ".weight").reshape(128, cf)[:, perm].contiguous()
    out["att1.b"] = g(k("att1") + ".bias")
    out["att1.s"] = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
    out["att1.h"] = bn["bias"] - bn["running_mean"] * out["att1.s"]
    out["att2.w"] = g(k("att2") + ".weight").reshape(cf, 128)[perm].contiguous()
    out["att2.b"] = g(k("att2") + ".bias")[perm].contiguous()
    bs, be = bnd(k("norm_stats")), bnd(k("norm_embed"))
    ss = bs["weight"] / torch.sqrt(bs["running_var"] + BN_EPS)
    sh = bs["bias"] - bs["running_mean"] * ss
    se = be["weight"] / torch.sqrt(be["running_var"] + BN_EPS)
    he = be["bias"] - be["running_mean"] * se
    fw, fb = g(k("fc") + ".weight"), g(k("fc") + ".bias")
    perm2 = torch.cat([perm, cf + perm])
    out["fc.w"] = (se[:, None] * fw * ss[None, :])[:, perm2].contiguous()
    out["fc.b"] = se * (fw @ sh + fb) + he
    return out


class PackedSbResNet:
    """``dz_sbr_weights`` + the tensors behind it (speechbrain ``ResNet`` checkpoint keys, ``SB_RESNET_KEYS``).

    * the Fbank is ECAPA's (windowed DFT as one GEMM operand, 80-bin mel bank);
    * every BatchNorm (eval, eps 1e-5) is folded in float64 (``sb_resnet_fold``): into the convolution before it, into
      scale / shift after attention.0's ReLU, and ``norm_stats`` / ``norm_embed`` into ``fc_embed``;
    * widths, blocks per layer and the squeeze-excitation reduction come from the shapes (``sb_resnet_shape``);
      ``strides``, ``min_num_samples`` and ``rows_per_pass`` (0: the library's default) are the caller's;
    * for "f16x3" the DFT, the 3x3 / 1x1 convolutions and the two attention convolutions also as split-f16 planes."""

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32",
                 strides=SB_RESNET_STRIDES, min_num_samples: int = SB_RESNET_MIN_NUM_SAMPLES, rows_per_pass: int = 0):
        assert precision in PRECISIONS, precision
        if int(min_num_samples) < 1 or int(rows_per_pass) < 0:
            raise ValueError(f"min_num_samples={min_num_samples!r}, rows_per_pass={rows_per_pass!r}")
        split = precision == "f16x3"
        pk = _Packed(device)
        self.shape = shape = sb_resnet_shape(sd, strides)
        f = sb_resnet_fold(sd, strides, torch.float64)
        w = _lib.SbrWeights()
        w.dft = pk.put(_pad2(dft_matrices().float(), 448, 416))
        if split:
            w.dft_split = pk.put_split(_pad2(dft_matrices().float(), 512, 416), "windowed DFT")
        w.mel = pk.put(_pad2(ecapa_mel_filterbank().t().contiguous(), 128, 224))
        w.stem_w, w.stem_b = pk.put(f["stem.w"]), pk.put(f["stem.b"])
        n = 0
        for L, nb in enumerate(shape["block_sizes"]):
            for i in range(nb):
                b = w.block[n]
                for j, name in enumerate(("conv1", "conv2", "down")):
                    if f"b{n}.{name}.w" in f:
                        m = f[f"b{n}.{name}.w"].float()
                        b.conv[j].w, b.conv[j].b = pk.put(m), pk.put(f[f"b{n}.{name}.b"])
                        if split:
                            b.conv[j].wsplit = pk.put_split(m, sb_resnet_key(name, L + 1, i))
                b.se_w1t, b.se_b1 = pk.put(f[f"b{n}.se.w1t"]), pk.put(f[f"b{n}.se.b1"])
                b.se_w2t, b.se_b2 = pk.put(f[f"b{n}.se.w2t"]), pk.put(f[f"b{n}.se.b2"])
                b.width, b.se_width = shape["channels"][L], shape["se"][L][i]
                b.stride, b.layer = (shape["strides"][L] if i == 0 else 1), L
                n += 1
        cf = shape["pooled"]
        cfpad = (cf + 127) // 128 * 128
        a1, a2 = f["att1.w"].float(), _pad2(f["att2.w"].float(), cfpad, 128)
        w.att1.w, w.att1.b = pk.put(a1), pk.put(f["att1.b"])
        w.att1.s, w.att1.h = pk.put(f["att1.s"]), pk.put(f["att1.h"])
        w.att2.w, w.att2.b = pk.put(a2), pk.put(_pad1(f["att2.b"].float(), cfpad))
        if split:
            w.att1.wsplit = pk.put_split(a1, "attention.0")
            w.att2.wsplit = pk.put_split(a2, "attention.3")
        w.fc.w, w.fc.b = pk.put(f["fc.w"]), pk.put(f["fc.b"])
        w.zeros = pk.put(torch.zeros(512))
        w.n_blocks, w.stem_width = n, shape["stem"]
        w.min_num_samples, w.rows_per_pass = int(min_num_samples), int(rows_per_pass)
        self.struct, self.pack = w, pk


# --------------------------------------------------------------------------- #
# NeMo TitaNet-L
# --------------------------------------------------------------------------- #
# (repeats, kernel, C_in, C_out, residual) of encoder.encoder.{0..4} (titanet-large.yaml: prolog, three mega blocks, epilog)
TITANET_BLOCKS = ((1, 3, 80, 1024, False), (3, 7, 1024, 1024, True), (3, 11, 1024, 1024, True), (3, 15, 1024, 1024, True),
                  (1, 1, 1024, 3072, False))
TITANET_BN_EPS = 1e-3
TITANET_MIN_NUM_SAMPLES = 257      # n_fft / 2 + 1: the first length the reflect-padded centred STFT accepts (two frames)
TITANET_PAD_MODES = ("reflect", "constant")
TITANET_FRAME_COUNTS = {"floor_plus_one": (0, 0), "padded": (256, 512)}     # -> (frame_pad, frame_nfft) of dz_ttn_weights
TITANET_ATTENTION_ORDERS = ("relu_bn_tanh", "bn_relu_tanh")
# THE key map of a NeMo EncDecSpeakerLabelModel checkpoint (model_weights.ckpt): every name the packer, the synthetic
# weights and the loader's recognition use comes from here.  {i}: encoder block, {m}: index inside its ``mconv``
# ModuleList — repeat j holds depthwise 5 j, pointwise 5 j + 1, BatchNorm 5 j + 2 (ReLU and Dropout at 5 j + 3, 5 j + 4
# except after the last repeat), the squeeze-excitation follows the last BatchNorm.
TITANET_KEYS = {
    "dw": "encoder.encoder.{i}.mconv.{m}.conv.weight",
    "pw": "encoder.encoder.{i}.mconv.{m}.conv.weight",
    "bn": "encoder.encoder.{i}.mconv.{m}",
    "se": "encoder.encoder.{i}.mconv.{m}.fc.{l}.weight",
    "res": "encoder.encoder.{i}.res.0.0.conv.weight",
    "res_bn": "encoder.encoder.{i}.res.0.1",
    "att_conv": "decoder._pooling.attention_layer.0.conv_layer",
    "att_bn": "decoder._pooling.attention_layer.0.bn",
    "att_out": "decoder._pooling.attention_layer.2",
    "emb_bn": "decoder.emb_layers.0.0",
    "emb_fc": "decoder.emb_layers.0.1",
}
# what the loader recognises a TitaNet state by
TITANET_MARKERS = (TITANET_KEYS["dw"].format(i=0, m=0), TITANET_KEYS["emb_fc"] + ".weight")


def titanet_key(kind: str, i: int = 0, j: int = 0, l: int = 0) -> str:
    """Checkpoint key (or prefix) of ``kind`` (``TITANET_KEYS``) for repeat ``j`` of encoder block ``i``."""
    m = {"dw": 5 * j, "pw": 5 * j + 1, "bn": 5 * j + 2, "se": 5 * (TITANET_BLOCKS[i][0] - 1) + 3}.get(kind, 0)
    return TITANET_KEYS[kind].format(i=i, m=m, l=l)


def titanet_dft_matrices() -> torch.Tensor:
    """The STFT of NeMo's front end as ONE real GEMM operand, (2 * 257, 400) f64: n_fft = 512 with a symmetric Hann
    window of 400 samples padded centrally (56 zeros each side), so a frame only reads the 400 samples under the
    window: rows 0 .. 256 = cos(2 pi k (n + 56) / 512) w[n], rows 257 .. 513 = sin(...) w[n]."""
    n = torch.arange(400, dtype=torch.float64)
    win = torch.hann_window(400, periodic=False, dtype=torch.float64)
    k = torch.arange(257, dtype=torch.float64)[:, None]
    ang = 2.0 * math.pi * k * (n[None, :] + 56.0) / 512.0
    return torch.cat([torch.cos(ang) * win, torch.sin(ang) * win], 0)


def slaney_mel_filterbank(n_mels: int, n_fft: int, sample_rate: int, f_min: float, f_max: float) -> torch.Tensor:
    """The slaney mel bank — librosa.filters.mel(htk=False, norm="slaney"), torchaudio's melscale_fbanks(norm="slaney",
    mel_scale="slaney") — as (n_mels, n_fft // 2 + 1) f64: a mel scale linear below 1 kHz (200 / 3 Hz per mel) and
    logarithmic above (27 mels per factor 6.4), n_mels + 2 points equally spaced on it between f_min and f_max,
    triangles between them over the bin frequencies, each scaled to unit area (2 / its width in Hz)."""
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    to_mel = lambda f: f / f_sp if f < min_log_hz else min_log_mel + math.log(f / min_log_hz) / logstep
    mels = torch.linspace(to_mel(f_min), to_mel(f_max), n_mels + 2, dtype=torch.float64)
    hz = torch.where(mels < min_log_mel, mels * f_sp, min_log_hz * torch.exp(logstep * (mels - min_log_mel)))
    freqs = torch.linspace(0.0, sample_rate / 2, n_fft // 2 + 1, dtype=torch.float64)
    lower = (freqs[None, :] - hz[:-2, None]) / (hz[1:-1] - hz[:-2])[:, None]
    upper = (hz[2:, None] - freqs[None, :]) / (hz[2:] - hz[1:-1])[:, None]
    return torch.clamp(torch.minimum(lower, upper), min=0.0) * (2.0 / (hz[2:] - hz[:-2]))[:, None]


def titanet_mel_filterbank() -> torch.Tensor:
    """librosa.filters.mel(sr=16000, n_fft=512, n_mels=80, fmin=0, fmax=8000, htk=False, norm="slaney") as (80, 257)
    f64 (``slaney_mel_filterbank``)."""
    return slaney_mel_filterbank(80, 512, 16000, 0.0, 8000.0)


def fold_pointwise_bn(w: torch.Tensor, bn: Dict[str, torch.Tensor], eps: float):
    """Conv1d weight (Cout, Cin, 1) without bias + BatchNorm1d (eval) -> (matrix (Cout, Cin), bias (Cout,)): the
    ``fold_conv_bn`` pattern for a pointwise 1-D convolution, in the dtype of ``w``."""
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + eps)
    return w[:, :, 0] * scale[:, None], bn["bias"] - bn["running_mean"] * scale


class PackedTitaNet:
    """``dz_ttn_weights`` + the tensors behind it (NeMo ``EncDecSpeakerLabelModel`` keys, ``TITANET_KEYS``).

    * the Hann window is folded into the DFT matrix (``titanet_dft_matrices``); the slaney mel bank stays exact f32;
    * depthwise taps as ``[taps][Cpad]``; every BatchNorm (eval, eps 1e-3) folded into the pointwise convolution in
      front of it (``fold_pointwise_bn``), as ``[Cout][Cpad]`` f32 and, for "f16x3", kb-major split-f16 planes;
    * the squeeze-excitation's second Linear transposed; the attention conv split into the columns that see x and the
      columns that see (mean | std); ``emb_layers.0.0`` (BatchNorm1d(6144), eps 1e-5) folded into ``emb_layers.0.1``.

    (R) switches, DESIGN.md 4.12: ``pad_mode`` "reflect" | "constant", ``frame_count`` "floor_plus_one" | "padded",
    ``min_num_samples``, ``attention_order`` "relu_bn_tanh" | "bn_relu_tanh"."""

    def __init__(self, sd: Dict[str, torch.Tensor], device: torch.device, precision: str = "f32",
                 pad_mode: str = "reflect", frame_count: str = "floor_plus_one",
                 min_num_samples: int = TITANET_MIN_NUM_SAMPLES, attention_order: str = "relu_bn_tanh"):
        assert precision in PRECISIONS, precision
        if pad_mode not in TITANET_PAD_MODES:
            raise ValueError(f"pad_mode={pad_mode!r}: expected one of {TITANET_PAD_MODES}")
        if frame_count not in TITANET_FRAME_COUNTS:
            raise ValueError(f"frame_count={frame_count!r}: expected one of {tuple(TITANET_FRAME_COUNTS)}")
        if attention_order not in TITANET_ATTENTION_ORDERS:
            raise ValueError(f"attention_order={attention_order!r}: expected one of {TITANET_ATTENTION_ORDERS}")
        if int(min_num_samples) <= 200:
            raise ValueError(f"min_num_samples={min_num_samples}: the centred STFT reads 200 samples back (> 200)")
        split = precision == "f16x3"
        pk = _Packed(device)
        f = titanet_fold(sd, attention_order, torch.float64)       # (folded in float64, rounded once by put)
        w = _lib.TtnWeights()
        w.dft = pk.put(_pad2(titanet_dft_matrices().float(), 640, 416))
        if split:
            w.dft_split = pk.put_split(_pad2(titanet_dft_matrices().float(), 640, 416), "windowed DFT (TitaNet)")
        w.mel = pk.put(_pad2(titanet_mel_filterbank().float(), 128, 288))

        def layer(dst, name, m, b, kb):
            dst.w, dst.b = pk.put(m), pk.put(b)
            if split:
                dst.wsplit = pk.put_split(m, name, kb=kb)

        for i, (reps, k, cin, cout, residual) in enumerate(TITANET_BLOCKS):
            blk, cpad = w.block[i], 96 if i == 0 else cin
            for j in range(reps):
                blk.rep[j].dw = pk.put(_pad2(f[f"dw{i}.{j}"], k, cpad))
                layer(blk.rep[j].pw, titanet_key("pw", i, j), _pad2(f[f"pw{i}.{j}.w"], cout, cpad), f[f"pw{i}.{j}.b"], True)
            blk.se1, blk.se2t = pk.put(f[f"se{i}.1"]), pk.put(f[f"se{i}.2t"])
            if residual:
                layer(blk.res, titanet_key("res", i), f[f"res{i}.w"], f[f"res{i}.b"], True)
        layer(w.asp_tdnn, TITANET_KEYS["att_conv"], f["att.w"], f["att.b"], False)
        w.asp_tdnn.s, w.asp_tdnn.h = pk.put(f["att.s"]), pk.put(f["att.h"])
        w.asp_wms = pk.put(f["att.wms"])
        layer(w.asp_conv, TITANET_KEYS["att_out"], f["att_out.w"], f["att_out.b"], False)
        w.fc.w, w.fc.b = pk.put(f["fc.w"]), pk.put(f["fc.b"])
        w.zeros = pk.put(torch.zeros(6144))
        w.pad_reflect = int(pad_mode == "reflect")
        w.frame_pad, w.frame_nfft = TITANET_FRAME_COUNTS[frame_count]
        w.min_num_samples = int(min_num_samples)
        self.struct, self.pack, self.folded = w, pk, f


def titanet_fold(sd: Dict[str, torch.Tensor], attention_order: str = "relu_bn_tanh", dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """Every matrix ``PackedTitaNet`` hands to the kernels, unpadded, in ``dtype`` (the packer folds in float64): ``dw{i}.{j}`` (taps, C), ``pw{i}.{j}.w|b``, ``se{i}.1|2t``, ``res{i}.w|b``,
    ``att.w|b|s|h|wms``, ``att_out.w|b``, ``fc.w|b``."""
    g = lambda k: sd[k].detach().cpu().to(dtype)
    bnd = lambda p: {n: g(f"{p}.{n}") for n in ("weight", "bias", "running_mean", "running_var")}
    out: Dict[str, torch.Tensor] = {}
    for i, (reps, k, cin, cout, residual) in enumerate(TITANET_BLOCKS):
        for j in range(reps):
            dw, pw = g(titanet_key("dw", i, j)), g(titanet_key("pw", i, j))
            if tuple(dw.shape) != (cin, 1, k) or pw.shape[1:] != (cin, 1):
                raise ValueError(f"{titanet_key('dw', i, j)}: shapes {tuple(dw.shape)} / {tuple(pw.shape)}, expected "
                                 f"({cin}, 1, {k}) / (Cout, {cin}, 1) (titanet-large geometry)")
            out[f"dw{i}.{j}"] = dw[:, 0, :].t().contiguous()
            out[f"pw{i}.{j}.w"], out[f"pw{i}.{j}.b"] = fold_pointwise_bn(pw, bnd(titanet_key("bn", i, j)), TITANET_BN_EPS)
        out[f"se{i}.1"] = g(titanet_key("se", i, l=0)).contiguous()
        out[f"se{i}.2t"] = g(titanet_key("se", i, l=2)).t().contiguous()
        if residual:
            out[f"res{i}.w"], out[f"res{i}.b"] = fold_pointwise_bn(g(titanet_key("res", i)), bnd(titanet_key("res_bn", i)),
                                                                 TITANET_BN_EPS)
    aw, ab = g(TITANET_KEYS["att_conv"] + ".weight")[:, :, 0], g(TITANET_KEYS["att_conv"] + ".bias")      # (128, 9216)
    bn = bnd(TITANET_KEYS["att_bn"])
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
    shift = bn["bias"] - bn["running_mean"] * scale
    if attention_order == "bn_relu_tanh":       # BatchNorm in front of the ReLU: folded into the convolution
        aw, ab = aw * scale[:, None], ab * scale + shift
        scale, shift = torch.ones_like(scale), torch.zeros_like(shift)
    out["att.w"], out["att.wms"], out["att.b"] = aw[:, :3072].contiguous(), aw[:, 3072:].contiguous(), ab
    out["att.s"], out["att.h"] = scale, shift
    out["att_out.w"], out["att_out.b"] = g(TITANET_KEYS["att_out"] + ".weight")[:, :, 0].contiguous(), g(TITANET_KEYS["att_out"] + ".bias")
    bn = bnd(TITANET_KEYS["emb_bn"])
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
    shift = bn["bias"] - bn["running_mean"] * scale
    fw, fb = g(TITANET_KEYS["emb_fc"] + ".weight")[:, :, 0], g(TITANET_KEYS["emb_fc"] + ".bias")
    out["fc.w"], out["fc.b"] = (fw * scale[None, :]).contiguous(), fb + fw @ shift
    return out
