"""float64 restatement of the band-limited resampler (DESIGN.md "Resampling"): torchaudio's ``sinc_interp_hann``
with ``lowpass_filter_width = 6`` and ``rolloff = 0.99``, written from its definition with numpy only.

    g = gcd(orig, new), o = orig / g, n = new / g, base = 0.99 min(o, n), width = ceil(6 o / base), T = 2 width + o
    t = clamp((-i / n + (k - width) / o) base, -6, 6),  h[i][k] = sinc(pi t) cos(t pi / 12)^2 base / o
    y[j n + i] = sum_k h[i][k] x[j o - width + k]   (x = 0 outside [0, L)),  ceil(n L / o) outputs
"""
from __future__ import annotations

import math

import numpy as np

LOWPASS_WIDTH = 6
ROLLOFF = 0.99


def geometry(orig: int, new: int):
    """-> (o, n, width, T)"""
    g = math.gcd(int(orig), int(new))
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_WIDTH * o / base)
    return o, n, width, 2 * width + o


def out_len(orig: int, new: int, length: int) -> int:
    o, n, _, _ = geometry(orig, new)
    return -(-n * length // o)


def table(orig: int, new: int, dtype=np.float64) -> np.ndarray:
    """(n, T) filter table, computed in ``dtype`` (float64: ``transforms.Resample``'s; float32: what
    ``functional.resample`` builds for a float32 waveform)."""
    o, n, width, T = geometry(orig, new)
    base = min(o, n) * ROLLOFF
    idx = (np.arange(-width, width + o, dtype=dtype) / dtype(o))[None, :]
    t = (np.arange(0, -n, -1, dtype=dtype) / dtype(n))[:, None] + idx
    t = t * dtype(base)
    t = np.clip(t, -LOWPASS_WIDTH, LOWPASS_WIDTH).astype(dtype)
    window = np.cos(t * dtype(math.pi) / dtype(LOWPASS_WIDTH) / dtype(2)) ** 2
    t = t * dtype(math.pi)
    with np.errstate(invalid="ignore", divide="ignore"):
        kern = np.where(t == 0, dtype(1.0), np.sin(t) / t)
    kern = kern * (window * dtype(base / o))
    assert kern.shape == (n, T)
    return kern.astype(dtype)


def resample(x: np.ndarray, orig: int, new: int, h: np.ndarray = None) -> np.ndarray:
    """Resample the last axis of ``x`` in float64 (``h``: a table to use instead of the float64 one, e.g. the
    library's float32 table).  Non-finite samples propagate like a convolution's: to every output whose taps
    cover them."""
    x = np.asarray(x, dtype=np.float64)
    if orig == new:
        return x.copy()
    o, n, width, T = geometry(orig, new)
    h = table(orig, new) if h is None else np.asarray(h, dtype=np.float64)
    L = x.shape[-1]
    M = out_len(orig, new, L)
    nj = -(-M // n)
    lead = x.shape[:-1]
    xf = x.reshape(-1, L)
    pad = np.zeros((xf.shape[0], width + nj * o + T), dtype=np.float64)
    pad[:, width:width + L] = xf
    # frames[r, j, k] = x[j o - width + k]
    frames = np.lib.stride_tricks.sliding_window_view(pad, T, axis=1)[:, ::o][:, :nj]
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.einsum("rjk,ik->rji", frames, h)
    return y.reshape(xf.shape[0], nj * n)[:, :M].reshape(*lead, M)


def nonfinite_reach(x: np.ndarray, orig: int, new: int) -> np.ndarray:
    """Boolean mask of the outputs whose taps cover a non-finite sample of the 1-D signal ``x``."""
    o, n, width, T = geometry(orig, new)
    bad = ~np.isfinite(np.asarray(x, dtype=np.float64))
    L = bad.shape[0]
    M = out_len(orig, new, L)
    m = np.arange(M)
    j = m // n
    start = j * o - width                       # taps cover [start, start + T)
    cum = np.concatenate([[0], np.cumsum(bad)])
    lo = np.clip(start, 0, L)
    hi = np.clip(start + T, 0, L)
    return (cum[hi] - cum[lo]) > 0
