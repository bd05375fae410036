"""Float64 (and float32) restatement of the SincNet front end every network here starts with, the test windows and
the error measures of tests/test_front_ref_host.py and tests/test_gpu_front_f64.py ("Accuracy of the
front end").  Plain torch on the CPU; imports no GPU code.

Stages (pyannote.audio SincNet.forward, the shapes of csrc/k_front.hip / k_conv_pool.hip):
  window statistics   mean, 1 / sqrt(biased var + 1e-5) of each window                       ``wave_stats``
  stage 0             InstanceNorm1d(1) * gamma + beta -> 80 x 251 bank, stride 10 -> |.| -> MaxPool1d(3)   ``stage0``
  tile partials       (sum, sum of squares) over the pooled frames of each tile              ``tile_partials``
  finalize_norm       partials -> InstanceNorm1d(C, affine) as (scale, shift)                ``finalize_norm``
  stages 1 / 2        x * scale + shift -> LeakyReLU(0.01) -> Conv1d(k = 5) -> MaxPool1d(3)  ``stage``
Every function takes ``dtype``: torch.float64 is the reference, torch.float32 the yardstick ("what plain float32
arithmetic gives on this case") that the gates are derived from — never the code under test.

The measure: an output is a sum of products, and what it can resolve is set by the sum of their magnitudes, not by the
largest output anywhere in the tensor: ``cond_err = |got - ref| / den`` with ``den`` the same stage on the operands'
absolute values (the ``|x| @ |w|`` denominator of test_split_gemm_dynamic_range).  The next operation is a per-channel
InstanceNorm, so a quiet channel's error counts against that channel.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
SLOPE = 0.01
F64, F32 = torch.float64, torch.float32

CASES = ("speech", "speech_x25", "speech_x1e-4", "lowpass", "tone", "dc", "click", "tail", "silence")
# ``dc_large``: the name under which the window-statistics test asks for "a DC level a thousand times the AC part";
# the same formula as ``dc`` (another seed offset only)
ALL_CASES = CASES + ("dc_large",)

# the affine pair of InstanceNorm1d(1) used with each network's bank: far from (1, 0), different per network
# (the pairs of test_gpu_kernels.py::test_sinc_conv0_pair); beta != 0 keeps ``den`` above |beta| * sum |filt| > 0
AFFINE = {"seg": (1.3, -0.05), "emb": (-0.7, 0.4)}


# --------------------------------------------------------------------------- banks and weights
@functools.lru_cache(maxsize=None)
def _state(net: str):
    from diart_amd.synth import synth_embedding_state, synth_segmentation_state
    return synth_segmentation_state() if net == "seg" else synth_embedding_state()


@functools.lru_cache(maxsize=None)
def bank(net: str) -> torch.Tensor:
    """(80, 251) float32 sinc bank of the synthetic ``seg`` / ``emb`` network: what the kernels are handed"""
    from diart_amd.weights import sinc_filters
    sd, p = _state(net), "sincnet.conv1d.0.filterbank."
    return sinc_filters(sd[p + "low_hz_"], sd[p + "band_hz_"], sd[p + "window_"], sd[p + "n_"])


def conv_weights(net: str, i: int):
    """(weight (60, Cin, 5), bias (60,), norm gamma (Cin,), norm beta (Cin,)) of stage i = 1, 2: the convolution and the
    InstanceNorm in FRONT of it (norm1d.{i - 1})"""
    sd = _state(net)
    return (sd[f"sincnet.conv1d.{i}.weight"], sd[f"sincnet.conv1d.{i}.bias"], sd[f"sincnet.norm1d.{i - 1}.weight"],
            sd[f"sincnet.norm1d.{i - 1}.bias"])


# --------------------------------------------------------------------------- windows
@functools.lru_cache(maxsize=None)
def _speech():
    from diart_amd.synth import synth_stream
    return synth_stream(5, 11.0)


def _noise(S: int, seed: int) -> np.ndarray:
    return np.random.default_rng(1000 + seed).standard_normal(S)


def make_case(name: str, S: int, seed: int = 0) -> torch.Tensor:
    """One window of S float32 samples.  Fixed seeds: the same (name, S, seed) is the same window everywhere."""
    if name.startswith("speech") or name == "tail":
        off = 2000 * (seed % 5) + 1234                 # (S up to 160000 of the 176000-sample stream)
        x = _speech()[off: off + S].astype(np.float64)
        if name == "speech_x25":
            x = x * 25.0
        elif name == "speech_x1e-4":
            x = x * 1e-4
        elif name == "tail":                       # the last 40 % of the window is the zero padding of a short file
            x = x.copy()
            x[int(0.6 * S):] = 0.0
    elif name == "lowpass":                        # noise behind a steep low-pass: 12th order, corner 300 Hz
        n = max(S, 4096)
        spec = np.fft.rfft(_noise(n, seed))
        f = np.fft.rfftfreq(n, 1.0 / 16000.0)
        x = np.fft.irfft(spec / (1.0 + (f / 300.0) ** 12), n)[:S]
        x = 0.3 * x / np.abs(x).max()
    elif name == "tone":                           # 150 Hz over a -80 dB noise floor
        t = np.arange(S) / 16000.0
        x = 0.5 * np.sin(2 * math.pi * 150.0 * t + 0.3) + 1e-4 * _noise(S, seed)
    elif name in ("dc", "dc_large"):               # a DC level a thousand times the AC part
        x = 1.0 + 1e-3 * _noise(S, seed + (7 if name == "dc_large" else 0))
    elif name == "click":
        x = np.zeros(S)
        x[(S * 5) // 11 // 10 * 10] = 0.9         # (a multiple of the stride: the frames see every tenth tap from tap 0)
    elif name == "silence":
        x = np.zeros(S)
    else:
        raise KeyError(name)
    return torch.from_numpy(np.asarray(x, dtype=np.float32).copy())


# --------------------------------------------------------------------------- the stages
def wave_stats(x: torch.Tensor, dtype=F64):
    """x (B, S) -> mean (B,), rstd (B,) = 1 / sqrt(biased var + 1e-5)"""
    x = x.to(dtype)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + EPS)


def normalise(x: torch.Tensor, gamma: float, beta: float, dtype=F64) -> torch.Tensor:
    """InstanceNorm1d(1) * gamma + beta, in the kernels' order of operations: ((x - mean) * rstd) * gamma + beta"""
    mean, rstd = wave_stats(x, dtype)
    return ((x.to(dtype) - mean[:, None]) * rstd[:, None]) * gamma + beta


def bank_pool(xn: torch.Tensor, filt: torch.Tensor) -> torch.Tensor:
    """xn (B, S), filt (C, 251) -> (B, C, P0): the bank at stride 10, abs, MaxPool1d(3)"""
    return F.max_pool1d(F.conv1d(xn[:, None, :], filt.to(xn.dtype)[:, None, :], stride=10).abs(), 3, 3)


def stage0(x: torch.Tensor, filt: torch.Tensor, gamma: float, beta: float, dtype=F64) -> torch.Tensor:
    return bank_pool(normalise(x, gamma, beta, dtype), filt)


def stage0_den(x: torch.Tensor, filt: torch.Tensor, gamma: float, beta: float) -> torch.Tensor:
    """what each stage-0 output can resolve: maxpool3(conv1d(|xn|, |filt|, stride 10)), float64"""
    return bank_pool(normalise(x, gamma, beta, F64).abs(), filt.double().abs())


def geometry(S: int):
    """(F0, P0): conv frames and pooled frames of stage 0"""
    F0 = (S - 251) // 10 + 1
    return F0, F0 // 3


def ntile(frames: int, tile_frames: int) -> int:
    return -(-frames // tile_frames)


def tile_partials(y: torch.Tensor, tile_frames: int, conv_frames: int, dtype=F64) -> torch.Tensor:
    """y (B, C, P) pooled -> (B, ntile, C, 2) (sum, sum of squares) over the pooled frames of each tile of
    ``tile_frames`` CONV frames (192: sinc_conv0; 96: the split kernels, conv_pool, gemm_split), ntile =
    ceil(conv_frames / tile_frames) — a ragged last tile may hold no complete pooled frame at all"""
    B, C, P = y.shape
    pt, nt = tile_frames // 3, ntile(conv_frames, tile_frames)
    y = y.to(dtype)
    out = torch.zeros(B, nt, C, 2, dtype=dtype)
    for t in range(nt):
        blk = y[:, :, t * pt: min((t + 1) * pt, P)]
        out[:, t, :, 0] = blk.sum(2)
        out[:, t, :, 1] = (blk * blk).sum(2)
    return out


def finalize_norm(part: torch.Tensor, T: int, gamma: torch.Tensor, beta: torch.Tensor, dtype=F64):
    """part (B, ntile, C, 2), T values per channel -> scale (B, C), shift (B, C): InstanceNorm1d(C, affine), biased
    variance as E[y^2] - mean^2 clamped at 0, eps 1e-5"""
    p = part.to(dtype).sum(1)
    mean = p[..., 0] / T
    var = torch.clamp(p[..., 1] / T - mean * mean, min=0.0)
    sc = gamma.to(dtype)[None, :] / torch.sqrt(var + EPS)
    return sc, beta.to(dtype)[None, :] - mean * sc


def norm_of(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, dtype=F64):
    """(scale, shift) of InstanceNorm1d(C, affine) over y (B, C, T) itself (two-pass variance)"""
    y = y.to(dtype)
    mean = y.mean(2)
    var = ((y - mean[:, :, None]) ** 2).mean(2)
    sc = gamma.to(dtype)[None, :] / torch.sqrt(var + EPS)
    return sc, beta.to(dtype)[None, :] - mean * sc


def activate(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """norm-on-load: LeakyReLU(y * scale + shift), y (B, C, T), scale / shift (B, C)"""
    return F.leaky_relu(y * scale.to(y.dtype)[:, :, None] + shift.to(y.dtype)[:, :, None], SLOPE)


def stage(y: torch.Tensor, scale, shift, w: torch.Tensor, bias: torch.Tensor, dtype=F64) -> torch.Tensor:
    """stages 1 / 2: y (B, Cin, T) -> (B, Cout, (T - 4) // 3)"""
    a = activate(y.to(dtype), scale, shift)
    return F.max_pool1d(F.conv1d(a, w.to(dtype), bias.to(dtype)), 3, 3)


def stage_den(y: torch.Tensor, scale, shift, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    a = activate(y.double(), scale, shift).abs()
    return F.max_pool1d(F.conv1d(a, w.double().abs(), bias.double().abs()), 3, 3)


def chain(x: torch.Tensor, net: str, dtype=F64):
    """the whole front end of network ``net`` on windows x (B, S) in ``dtype`` -> [y0, y1, y2] (each (B, C, P)); the
    normalisation between stages from the tile partials (96-frame tiles) through finalize_norm, as the kernels do"""
    gamma, beta = AFFINE[net]
    y = stage0(x, bank(net), gamma, beta, dtype)
    frames = geometry(x.shape[1])[0]
    out = [y]
    for i in (1, 2):
        w, b, g, bt = conv_weights(net, i)
        sc, sh = finalize_norm(tile_partials(y, 96, frames, dtype), y.shape[2], g, bt, dtype)
        frames = y.shape[2] - 4
        y = stage(y, sc, sh, w, b, dtype)
        out.append(y)
    return out


# --------------------------------------------------------------------------- the measures
def cond_err(got: torch.Tensor, ref: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """element-wise |got - ref| / den in float64"""
    return (got.double() - ref.double()).abs() / den.double()


def part_err(got: torch.Tensor, ref_y: torch.Tensor, den: torch.Tensor, got_y: torch.Tensor = None):
    """tile partials got (B, ntile, C, 2) against the float64 pooled output ref_y (B, C, P) and its denominator ->
    (err of the sums, err of the sums of squares), each (B, C):
    |S got - S ref| / S den   and   |SS got - SS ref| / S den (|ref| + |got_y|)
    With every element within g den of its reference, got^2 - ref^2 = (got - ref)(got + ref) puts both under g.
    ``got_y``: the pooled output the partials were summed from; None: the first-order form 2 S den |ref|, which is the
    same number wherever a channel is resolved and 0 / 0 where its reference lies below what it resolves (silence
    through the odd filters: |ref| ~ 1e-17 den; float32 itself scores 1e+1 there, tests/test_front_ref_host.py)"""
    g = got.double().sum(1)
    ref_y, den = ref_y.double(), den.double()
    mag = 2.0 * ref_y.abs() if got_y is None else ref_y.abs() + got_y.double().abs()
    e1 = (g[..., 0] - ref_y.sum(2)).abs() / den.sum(2)
    e2 = (g[..., 1] - (ref_y * ref_y).sum(2)).abs() / (den * mag).sum(2)
    return e1, e2


def old_rel(got: torch.Tensor, ref: torch.Tensor) -> float:
    """the measure of test_gpu_kernels.py::test_sinc_conv0*: largest error over largest output of the whole tensor"""
    a, b = got.double(), ref.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def gate(e32: float, floor: float = 1e-6) -> float:
    """the one rule of the GPU tests: max(floor, 4 e32) — 22 mantissa bits of the f16x3 operands against float32's 24
    (tests/test_gpu_lstm_f64.py), floor 1e-6 as test_f16x3_dynamic_range_map grants f16x3"""
    return max(floor, 4.0 * e32)


def round_f16(t: torch.Tensor) -> torch.Tensor:
    """an operand that lost its low plane: clamp to +-65504, round to f16"""
    return t.clamp(-65504.0, 65504.0).to(torch.float16).to(t.dtype)


# stage-0 lengths of the GPU test: 4, 96, 97, 192 and 193 conv frames (the tile edges of both kernels), frame counts
# not divisible by 3, S not divisible by 4, and the real window (speech and lowpass only there)
STAGE0_S = (281, 1201, 1211, 2161, 2171, 2661, 2663, 80000)


def stage0_cells():
    """every (net, case, S) of the stage-0 tests"""
    for net in ("seg", "emb"):
        for S in STAGE0_S:
            for case in ALL_CASES:
                if S == 80000 and case not in ("speech", "lowpass"):
                    continue
                yield net, case, S


@functools.lru_cache(maxsize=None)
def stage0_ref(net: str, case: str, S: int):
    """(x (1, S) float32, ref float64, den float64, e32) of one cell — computed once, shared, never modified"""
    gamma, beta = AFFINE[net]
    x = make_case(case, S)[None, :]
    ref = stage0(x, bank(net), gamma, beta, F64)
    den = stage0_den(x, bank(net), gamma, beta)
    e32 = cond_err(stage0(x, bank(net), gamma, beta, F32), ref, den).max().item()
    return x, ref, den, e32
