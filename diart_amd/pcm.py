"""The sample formats of raw client audio and their definition in numpy (``include/diart_amd.h``,
``dz_ring_push_rows_pcm``): what the push kernel computes on the GPU, operation for operation in float32, for
host-window mode, custom engines and the file reader.  numpy only: nothing here touches a device.

=========  ==========  =====================================================================================
name       pushed as   float32 sample
=========  ==========  =====================================================================================
``f32``    float32     the value
``s16``    int16       ``float(v) * (1 / 32768)``
``u8``     uint8       ``(float(v) - 128) * (1 / 128)``
``s32``    int32       ``float(v) * 2**-31`` (the conversion rounds to nearest even, the scaling is exact)
``ulaw``   uint8       ``float(L) * (1 / 32768)``, ``L`` the G.711 mu-law expansion of the byte
``alaw``   uint8       ``float(L) * (1 / 32768)``, ``L`` the G.711 A-law expansion of the byte
=========  ==========  =====================================================================================
"""
from __future__ import annotations

import numpy as np

# name -> (DZ_PCM_* constant, dtype of the values clients push; multi-byte values are little-endian)
PCM_FORMATS = {"f32": (0, np.dtype("<f4")), "s16": (1, np.dtype("<i2")), "u8": (2, np.dtype("u1")),
               "s32": (3, np.dtype("<i4")), "ulaw": (4, np.dtype("u1")), "alaw": (5, np.dtype("u1"))}
INPUT_FORMATS = {name: dtype for name, (_, dtype) in PCM_FORMATS.items()}


def ulaw_expand(codes) -> np.ndarray:
    """G.711 mu-law bytes -> 16-bit linear values (int32): 255 distinct values, ``0xFF`` and ``0x7F`` are 0."""
    u = ~np.asarray(codes, dtype=np.int32) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int32)


def alaw_expand(codes) -> np.ndarray:
    """G.711 A-law bytes -> 16-bit linear values (int32): 256 distinct values, none of them 0."""
    a = np.asarray(codes, dtype=np.int32) ^ 0x55
    m = (a & 0x0F) << 4
    s = (a >> 4) & 7
    t = np.where(s == 0, m + 8, (m + 0x108) << np.maximum(s - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int32)


_SCALE15 = np.float32(1.0 / 32768.0)
_TABLES = {"ulaw": ulaw_expand(np.arange(256)).astype(np.float32) * _SCALE15,
           "alaw": alaw_expand(np.arange(256)).astype(np.float32) * _SCALE15}


def pcm_to_float(values: np.ndarray, input_format: str = "f32") -> np.ndarray:
    """Values of ``input_format`` -> float32 samples of the same shape (the table of the module docstring)."""
    if input_format not in INPUT_FORMATS:
        raise ValueError(f"input_format={input_format!r} (expected one of {tuple(INPUT_FORMATS)})")
    x = np.asarray(values)
    if input_format == "f32":
        return x
    if input_format == "s16":
        return x.astype(np.float32) * _SCALE15
    if input_format == "u8":
        return (x.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    if input_format == "s32":
        return x.astype(np.float32) * np.float32(2.0 ** -31)
    return _TABLES[input_format][x]


def pcm_to_mono(values: np.ndarray, input_format: str = "f32", channels: int = 1) -> np.ndarray:
    """Interleaved client audio -> mono float32, the arithmetic of ``dz_ring_push_rows_pcm`` operation for operation
    (all in float32): the format's conversion (``pcm_to_float``; int16 ``v -> float(v) * (1 / 32768)``, exact, what
    ``read_wav`` does), then for several channels ``((c0 + c1) + c2 ...) / channels``.  One float32 channel is
    returned as it is."""
    x = pcm_to_float(np.asarray(values).reshape(-1), input_format)
    if channels == 1:
        return x
    frames = x.reshape(-1, channels)
    total = frames[:, 0].copy()
    for c in range(1, channels):
        total = total + frames[:, c]
    return total / np.float32(channels)
