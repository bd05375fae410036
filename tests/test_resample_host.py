"""The resampler's host half (DESIGN.md "Resampling"): geometry, output lengths and the float32 filter table of
``libdiart_amd.so`` against the float64 restatement (tests/resample_ref.py), the restatement pinned to its
definition, refusals, the ``blocks.Resample`` export and the 24-bit WAV decode.  No GPU."""
import ctypes as C
import sys
import wave
from pathlib import Path

import numpy as np
import pytest

from diart_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_ref as R  # noqa: E402

RATES = [44100, 22050, 11025, 48000, 32000, 8000, 12000, 24000, 88200, 96000]
# (phases, taps) of the issue's geometry table, 16 kHz output
PINNED = {44100: (160, 475), 22050: (320, 459), 11025: (640, 455), 48000: (1, 41), 32000: (1, 28), 8000: (2, 15)}


def _lib_table(orig, new):
    lib = _lib.load()
    p, t = C.c_int(), C.c_int()
    _lib.check(lib.dz_resample_geometry(orig, new, C.byref(p), C.byref(t), None, None), "geometry")
    h = np.empty((p.value, t.value), dtype=np.float32)
    _lib.check(lib.dz_resample_table(orig, new, h.ctypes.data_as(_lib.c_float_p)), "table")
    return h


@pytest.mark.parametrize("orig", RATES)
def test_geometry_and_lengths_match_the_restatement(orig):
    lib = _lib.load()
    p, t, w, o = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.dz_resample_geometry(orig, 16000, C.byref(p), C.byref(t), C.byref(w), C.byref(o)) == 0
    ro, rn, rw, rT = R.geometry(orig, 16000)
    assert (p.value, t.value, w.value, o.value) == (rn, rT, rw, ro)
    if orig in PINNED:
        assert (rn, rT) == PINNED[orig]
    for L in (0, 1, 5, ro - 1, ro, ro + 1, 5 * orig, 5 * orig + 7, 1800 * orig, 2 ** 31 - 1):
        assert lib.dz_resample_out_len(orig, 16000, L) == R.out_len(orig, 16000, L), L
    assert R.out_len(orig, 16000, 5 * orig) == 80000


@pytest.mark.parametrize("orig", RATES)
def test_float32_table_within_one_ulp_of_float64(orig):
    h = _lib_table(orig, 16000)
    h64 = R.table(orig, 16000)
    assert h.shape == h64.shape
    ulp = np.spacing(np.abs(h64).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(h.astype(np.float64) - h64) <= ulp)


def test_restatement_pins():
    # DC gain of every phase
    for orig in RATES:
        dc = R.table(orig, 16000).sum(axis=1)
        assert dc.min() >= 1.00003 and dc.max() <= 1.0009, orig
    # tones from 44.1 kHz: 1 kHz passes, 9 kHz (above the 8 kHz Nyquist) is attenuated
    t = np.arange(2 * 44100) / 44100
    for f, lo, hi in ((1000, 0.9995, 0.9997), (9000, 0.13, 0.15)):
        x = np.sin(2 * np.pi * f * t)
        y = R.resample(x, 44100, 16000)
        gain = np.sqrt((y[2000:-2000] ** 2).mean() / (x[4000:-4000] ** 2).mean())
        assert lo < gain < hi, (f, gain)


def test_float32_built_table_difference():
    """(R) ``functional.resample`` builds the table in the waveform's float32, ``transforms.Resample`` in float64;
    this library rounds the float64 table.  On signals in [-1, 1]: the rounded table stays far inside the GPU gate
    (max 1e-5, relative L2 2e-6) of the float64 definition at every rate.  The float32-built table does too where
    o is small (48 / 32 / 8 kHz), but NOT at the o = 441 ratios: its phases t are rounded to float32 before
    sin(pi t), and over 455 - 475 taps that reaches 9e-6 (44.1 kHz), 2.7e-5 (22.05) and 4.2e-5 (11.025) max,
    relative L2 up to 1.4e-5 (DESIGN.md "Resampling").  These bounds are pinned here."""
    rng = np.random.default_rng(3)
    for orig, tol_max, tol_rel in ((48000, 1e-6, 1e-6), (32000, 1e-6, 1e-6), (8000, 1e-6, 1e-6),
                                   (44100, 1.5e-5, 1e-5), (22050, 4e-5, 1.5e-5), (11025, 6e-5, 2e-5)):
        x = rng.uniform(-1, 1, 2 * orig)
        y64 = R.resample(x, orig, 16000)
        rounded = R.resample(x, orig, 16000, _lib_table(orig, 16000))
        assert np.abs(y64 - rounded).max() < 1e-6
        assert np.linalg.norm(y64 - rounded) / np.linalg.norm(y64) < 1e-7
        y32 = R.resample(x, orig, 16000, R.table(orig, 16000, np.float32))
        d = y64 - y32
        assert np.abs(d).max() < tol_max and np.linalg.norm(d) / np.linalg.norm(y64) < tol_rel, orig


def test_equal_rates_and_refusals():
    lib = _lib.load()
    assert lib.dz_resample_out_len(16000, 16000, 12345) == 12345
    from diart_amd.functional import resample
    x = np.arange(10, dtype=np.float32)
    assert resample(x, 16000, 16000) is x                 # no launch, no GPU needed
    for bad in ((0, 16000), (-44100, 16000), (16000, 0)):
        assert lib.dz_resample_geometry(*bad, None, None, None, None) != 0
        assert lib.dz_resample_out_len(*bad, 100) == -1
    # 16001 -> 16000: 16000 phases x 16015 taps, a ~1 GB table
    assert lib.dz_resample_geometry(16001, 16000, None, None, None, None) == 2
    assert b"filter table" in lib.dz_last_error()
    for ok in (12000, 24000, 88200, 96000):
        assert lib.dz_resample_geometry(ok, 16000, None, None, None, None) == 0


def test_blocks_export_resample():
    from diart_amd.blocks import Resample, resample  # noqa: F401
    import diart_amd.blocks as blocks
    assert "Resample" in blocks.__all__


def _write_pcm(path, sr, width, ints):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(width)
        f.setframerate(sr)
        if width == 3:
            b = np.asarray(ints, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :3]
            f.writeframes(b.tobytes())
        else:
            f.writeframes(np.asarray(ints, dtype="<i4").tobytes())


def test_24bit_wav_decodes_like_32bit(tmp_path):
    from diart_amd.inference import read_wav, read_wav_into
    rng = np.random.default_rng(0)
    s24 = rng.integers(-2 ** 23, 2 ** 23, 4410)
    s24[:4] = [-2 ** 23, 2 ** 23 - 1, 0, -1]
    _write_pcm(tmp_path / "a24.wav", 44100, 3, s24)
    _write_pcm(tmp_path / "a32.wav", 44100, 4, s24 * 256)
    x24, sr24 = read_wav(tmp_path / "a24.wav")
    x32, sr32 = read_wav(tmp_path / "a32.wav")
    assert sr24 == sr32 == 44100 and x24.dtype == np.float32
    assert np.array_equal(x24, x32)
    assert x24[0] == -1.0 and x24[2] == 0.0
    out, sr, pad = read_wav_into(tmp_path / "a24.wav", lambda n: np.full(n, 7, np.float32), lambda d: (0.5, 0.25))
    left = int(np.rint(0.5 * 44100))
    assert np.array_equal(out[left:left + 4410], x32) and not out[:left].any()
