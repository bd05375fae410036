"""G.711, 8-bit and 32-bit client audio, host side: ``pcm_to_mono`` against the definition, the windows a custom
engine receives, the argument checks, the websocket decoding and the WAV reader.  No GPU.

The definition (``include/diart_amd.h``, ``dz_ring_push_rows_pcm``) is restated here from the integer formulas in
int64 and float32 operations in the stated order, independently of ``diart_amd.pcm``."""
import base64
import struct
import wave

import numpy as np
import pytest

from diart_amd.inference import read_wav, read_wav_into, wav_duration
from diart_amd.serve import INPUT_FORMATS, StreamServer, pcm_to_mono
from diart_amd.ws import decode_audio

STEP, WINDOW = 8000, 80000
NEW = ("u8", "s32", "ulaw", "alaw")
DTYPES = {"u8": np.uint8, "s32": np.dtype("<i4"), "ulaw": np.uint8, "alaw": np.uint8}


def ulaw_linear(b):
    u = ~np.asarray(b).astype(np.int64) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where((u & 0x80) != 0, 0x84 - t, t - 0x84)


def alaw_linear(b):
    a = np.asarray(b).astype(np.int64) ^ 0x55
    m = (a & 0x0F) << 4
    s = (a >> 4) & 7
    t = np.where(s == 0, m + 8, (m + 0x108) << np.where(s == 0, 0, s - 1))
    return np.where((a & 0x80) != 0, t, -t)


def to_float(v, fmt):
    """One value of ``fmt`` -> its float32 sample, every operation rounded to float32."""
    v = np.asarray(v)
    if fmt == "f32":
        return v.astype(np.float32)
    if fmt == "s16":
        return np.multiply(v.astype(np.float32), np.float32(2.0 ** -15), dtype=np.float32)
    if fmt == "u8":
        return np.multiply(np.subtract(v.astype(np.float32), np.float32(128.0), dtype=np.float32),
                           np.float32(2.0 ** -7), dtype=np.float32)
    if fmt == "s32":
        # int64 -> float32 rounds to nearest even, as the int32 -> float32 conversion does
        return np.multiply(v.astype(np.int64).astype(np.float32), np.float32(2.0 ** -31), dtype=np.float32)
    lin = ulaw_linear(v) if fmt == "ulaw" else alaw_linear(v)
    return np.multiply(lin.astype(np.float32), np.float32(2.0 ** -15), dtype=np.float32)


def restate(values, fmt, channels):
    """float32 mono of interleaved ``values``: ((c0 + c1) + c2 ...) / channels of the formats' samples."""
    v = to_float(np.asarray(values).reshape(-1, channels), fmt)
    assert v.dtype == np.float32
    if channels == 1:
        return v[:, 0]
    acc = v[:, 0]
    for c in range(1, channels):
        acc = np.add(acc, v[:, c], dtype=np.float32)
    return np.divide(acc, np.float32(channels), dtype=np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def make_audio(rng, fmt, channels, frames):
    if fmt == "s32":
        a = rng.integers(-2 ** 31, 2 ** 31, size=(frames, channels), dtype=np.int64).astype("<i4")
        a[3], a[4] = -2 ** 31, 2 ** 31 - 1
        a[5, 0], a[5, -1] = 0x7fffffc0, 0x7fffffbf            # rounds up to 1.0f / stays below
        a[STEP - 1], a[STEP] = 2 ** 31 - 1, -2 ** 31
        return a
    a = rng.integers(0, 256, size=(frames, channels), dtype=np.uint8)
    a[3], a[4], a[5, 0], a[5, -1] = 0x00, 0xFF, 0x80, 0x7F
    a[STEP - 1], a[STEP] = 0x7F, 0x80
    return a


# ------------------------------------------------------------------------------------------- the definition
def test_g711_pins_and_value_sets():
    pins_u = {0x00: -32124, 0x80: 32124, 0x7F: 0, 0xFF: 0, 0x01: -31100, 0x8F: 16764}
    pins_a = {0xD5: 8, 0x55: -8, 0xAA: 32256, 0x2A: -32256, 0x00: -5504, 0x80: 5504}
    codes = np.arange(256, dtype=np.uint8)
    for fmt, pins, lin in (("ulaw", pins_u, ulaw_linear), ("alaw", pins_a, alaw_linear)):
        assert all(int(lin(b)) == L for b, L in pins.items())
        got = pcm_to_mono(codes, fmt)
        assert got.dtype == np.float32
        assert np.array_equal(bits(got), bits(lin(codes).astype(np.float32) / np.float32(32768.0)))
        for b, L in pins.items():
            assert got[b] == np.float32(L) / np.float32(32768.0)
    u, a = pcm_to_mono(codes, "ulaw"), pcm_to_mono(codes, "alaw")
    assert len(set(u.tolist())) == 255 and len(set(a.tolist())) == 256
    assert u[0xFF] == 0 and u[0x7F] == 0 and not (a == 0).any() and np.abs(a).min() == np.float32(8 / 32768)
    assert np.array_equal(np.sort(u), -np.sort(u)[::-1]) and np.array_equal(np.sort(a), -np.sort(a)[::-1])


def test_s32_rounds_once_and_u8_is_exact():
    v = np.array([0x7fffffc0, 0x7fffffbf, -2 ** 31, 2 ** 31 - 1, 0, 1, -1, 0x01000001], dtype="<i4")
    got = pcm_to_mono(v, "s32")
    assert got[0] == np.float32(1.0) and got[1] < 1.0 and got[2] == -1.0 and got[3] == 1.0
    assert got[5] == np.float32(2.0 ** -31) and got[7] == np.float32(2.0 ** -7)          # 0x01000001 rounds to 2^24
    assert np.array_equal(bits(got), bits(restate(v, "s32", 1)))
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(pcm_to_mono(u, "u8").astype(np.float64), (u.astype(np.float64) - 128) / 128)


@pytest.mark.parametrize("fmt", NEW)
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_pcm_to_mono_equals_the_restatement(fmt, channels):
    rng = np.random.default_rng(channels)
    a = make_audio(rng, fmt, channels, 2 * STEP)
    if fmt in ("ulaw", "alaw", "u8"):
        a[100:356] = np.arange(256, dtype=np.uint8)[:, None]           # every code, in every channel at once
        a[400:656, 0] = np.arange(256, dtype=np.uint8)                 # and against random partners
    got = pcm_to_mono(a.reshape(-1), fmt, channels)
    assert got.dtype == np.float32 and got.shape == (2 * STEP,)
    assert np.array_equal(bits(got), bits(restate(a, fmt, channels)))


# ------------------------------------------------------------------------------------------------ the server
class Recorder:
    def __init__(self):
        self.windows = {}

    def __call__(self, windows, starts, slots):
        assert windows.dtype == np.float32
        for w, t, s in zip(windows, starts, slots):
            self.windows.setdefault(s, []).append((float(t), w.copy()))
        return [np.zeros((0, 3)) for _ in slots]


@pytest.mark.parametrize("fmt,channels", [("ulaw", 1), ("ulaw", 2), ("alaw", 2), ("alaw", 3), ("u8", 1), ("u8", 8),
                                          ("s32", 1), ("s32", 2)])
def test_windows_equal_the_definition_bit_for_bit(fmt, channels):
    rng = np.random.default_rng(channels * 10 + len(fmt))
    rec = Recorder()
    srv = StreamServer(None, None, max_streams=3, engine=rec, input_format=fmt, input_channels=channels)
    assert srv.rings is None and srv._in_dtype == INPUT_FORMATS[fmt] == np.dtype(DTYPES[fmt])
    frames = {"a": WINDOW + 3 * STEP + 123, "b": WINDOW + 2 * STEP, "c": WINDOW + STEP + 7999}
    audio = {k: make_audio(rng, fmt, channels, n) for k, n in frames.items()}
    for k in audio:
        srv.open(k)
    # "a": 1-D pushes of odd numbers of VALUES (frames are cut across calls when channels > 1 and buffered until whole);
    # "b": 2-D (n, channels) pushes; "c": one 1-D push
    flat = audio["a"].reshape(-1)
    lo = 0
    while lo < flat.size:
        n = int(rng.integers(1, 3 * STEP * channels)) | 1
        srv.push("a", flat[lo:lo + n])
        assert srv._streams["a"].buffer.size == min(lo + n, flat.size) % (STEP * channels)
        lo += n
        if rng.random() < 0.3:
            srv.step()
    lo = 0
    while lo < frames["b"]:
        n = int(rng.integers(1, 2 * STEP))
        srv.push("b", audio["b"][lo:lo + n])
        lo += n
    srv.push("c", audio["c"].reshape(-1))
    srv.drain()
    slots = {k: srv._streams[k].slot for k in audio}
    for k, a in audio.items():
        mono = restate(a, fmt, channels)
        assert np.array_equal(bits(mono), bits(pcm_to_mono(a.reshape(-1), fmt, channels)))
        got = rec.windows[slots[k]]
        assert len(got) == (frames[k] - WINDOW) // STEP + 1
        for i, (t, w) in enumerate(got):
            assert abs(t - 0.5 * i) < 1e-9
            assert np.array_equal(bits(w), bits(mono[i * STEP:i * STEP + WINDOW])), (k, i)


def test_a_wrong_dtype_raises_and_old_names_stay_refused():
    eng = Recorder()
    wrong = {"u8": np.int8, "ulaw": np.int16, "alaw": np.float32, "s32": np.int64}
    for fmt in NEW:
        srv = StreamServer(None, None, max_streams=1, engine=eng, input_format=fmt, input_channels=2)
        srv.open(0)
        with pytest.raises(ValueError):
            srv.push(0, np.zeros(10, dtype=wrong[fmt]))
        with pytest.raises(ValueError):
            srv.push(0, np.zeros(10, dtype=np.float32))
        with pytest.raises(ValueError):
            srv.push(0, np.zeros((10, 3), dtype=DTYPES[fmt]))         # not (n, 2)
        assert srv.push(0, np.zeros((10, 2), dtype=DTYPES[fmt])) == 0
    f32 = StreamServer(None, None, max_streams=1, engine=eng)
    f32.open(0)
    with pytest.raises(ValueError):
        f32.push(0, np.zeros(10, dtype=np.uint8))
    for bad in ("s24", "mulaw", "int16", None):
        with pytest.raises(ValueError):
            StreamServer(None, None, engine=eng, input_format=bad)
    assert {k: v for k, v in INPUT_FORMATS.items()} == {
        "f32": np.dtype("<f4"), "s16": np.dtype("<i2"), "u8": np.dtype(np.uint8), "s32": np.dtype("<i4"),
        "ulaw": np.dtype(np.uint8), "alaw": np.dtype(np.uint8)}


def test_decode_audio_in_the_new_formats():
    x = np.array([[0x00, 0xFF], [0x80, 0x7F], [0x55, 0xD5]], dtype=np.uint8)
    raw = x.tobytes()
    for fmt in ("u8", "ulaw", "alaw"):
        for msg in (raw, base64.b64encode(raw).decode()):
            got = decode_audio(msg, fmt, 2)
            assert got.dtype == np.uint8 and np.array_equal(got, x.reshape(-1))
            assert np.array_equal(decode_audio(msg, fmt), x.reshape(-1))
        for msg in (raw[:-1], base64.b64encode(raw[:-1]).decode()):       # half a stereo frame
            with pytest.raises(ValueError):
                decode_audio(msg, fmt, 2)
            decode_audio(msg, fmt, 1)
        with pytest.raises(ValueError):
            decode_audio(raw[:4], fmt, 3)
    y = np.array([[-2 ** 31, 2 ** 31 - 1], [1, -1]], dtype="<i4")
    raw = y.tobytes()
    for msg in (raw, base64.b64encode(raw).decode()):
        got = decode_audio(msg, "s32", 2)
        assert got.dtype == np.dtype("<i4") and np.array_equal(got, y.reshape(-1))
    for cut in (1, 2, 3):
        with pytest.raises(ValueError):
            decode_audio(raw[:-cut], "s32")                                # not whole values
    with pytest.raises(ValueError):
        decode_audio(raw[:-4], "s32", 2)                                   # half a stereo frame
    with pytest.raises(KeyError):
        decode_audio(raw, "mulaw")


# ------------------------------------------------------------------------------------------------- WAV files
def write_riff(path, tag, channels, rate, bits, data, extra=b"", before=(), extensible=False):
    """A RIFF/WAVE file: ``fmt `` (``extensible``: tag 0xFFFE around sub-format ``tag``), the chunks of ``before``
    (id, body), then ``data``; an odd-sized chunk is padded with one byte."""
    def chunk(cid, body):
        return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits) + extra
    if extensible:
        fmt += struct.pack("<HHIH", 22, bits, 0, tag) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + chunk(b"fmt ", fmt) + b"".join(chunk(c, b) for c, b in before) + chunk(b"data", data)
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def check_file(path, want, rate):
    got, sr = read_wav(path)
    assert sr == rate and got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert wav_duration(path) == len(want) / rate
    out, sr2, pad = read_wav_into(path, lambda n: np.full(n, 7.0, dtype=np.float32), lambda d: (0.25, 0.1), 0.5)
    left = int(np.rint(0.25 * rate))
    assert sr2 == rate and pad == (0.25, 0.1) and len(out) % (rate // 2) == 0
    assert np.array_equal(bits(out[left:left + len(want)]), bits(want))
    assert not out[:left].any() and not out[left + len(want):].any()


@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("channels", [1, 2])
def test_read_wav_g711(tmp_path, law, tag, channels):
    rng = np.random.default_rng(tag + channels)
    a = rng.integers(0, 256, size=(8000 + 77, channels), dtype=np.uint8)
    a[:256, 0] = np.arange(256)
    p = write_riff(tmp_path / "g.wav", tag, channels, 8000, 8, a.tobytes(), extra=struct.pack("<H", 0))
    check_file(p, restate(a, law, channels), 8000)


def test_read_wav_float_extensible_list_and_odd_chunks(tmp_path):
    rng = np.random.default_rng(5)
    f = rng.uniform(-1.5, 1.5, size=(4001, 2)).astype("<f4")
    check_file(write_riff(tmp_path / "f32.wav", 3, 2, 16000, 32, f.tobytes()), restate(f, "f32", 2), 16000)
    d = rng.uniform(-1, 1, size=4001).astype("<f8")
    check_file(write_riff(tmp_path / "f64.wav", 3, 1, 16000, 64, d.tobytes()), d.astype(np.float32), 16000)
    s = rng.integers(-32768, 32768, size=(3999, 2), dtype=np.int16).astype("<i2")
    check_file(write_riff(tmp_path / "ext.wav", 1, 2, 44100, 16, s.tobytes(), extensible=True),
               restate(s, "s16", 2), 44100)
    u = rng.integers(0, 256, size=8001, dtype=np.uint8)
    check_file(write_riff(tmp_path / "extu.wav", 7, 1, 8000, 8, u.tobytes(), extensible=True),
               restate(u, "ulaw", 1), 8000)
    # a LIST chunk and an odd-sized chunk (with its pad byte) before the data, and an odd-sized data chunk
    mono = s[:, 0].copy()
    p = write_riff(tmp_path / "list.wav", 1, 1, 16000, 16, mono.tobytes(),
                   before=[(b"LIST", b"INFOISFT\x05\0\0\0abcd\0\0"), (b"odd ", b"data!"), (b"fact", struct.pack("<I", 3999))])
    check_file(p, restate(mono, "s16", 1), 16000)
    p = write_riff(tmp_path / "oddu.wav", 7, 1, 8000, 8, u[:4001].tobytes(), before=[(b"junk", b"x")])
    check_file(p, restate(u[:4001], "ulaw", 1), 8000)


def _wave_module_decode(path):
    """What ``read_wav`` gave while it stood on the ``wave`` module: that module's frames, and the arithmetic."""
    with wave.open(str(path), "rb") as f:
        sr, nch, width, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
        raw = f.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3)
        w = np.zeros((b.shape[0], 4), dtype=np.uint8)
        w[:, 1:] = b
        x = w.view("<i4")[:, 0].astype(np.float32) / 2147483648.0
    x = x.reshape(-1, nch)
    return (x.mean(axis=1) if nch > 1 else x[:, 0]).astype(np.float32), sr


@pytest.mark.parametrize("width,channels", [(2, 1), (2, 2), (3, 2), (1, 1), (1, 3)])
def test_integer_pcm_files_decode_as_before(tmp_path, width, channels):
    rng = np.random.default_rng(width * 10 + channels)
    raw = rng.integers(0, 256, size=5003 * channels * width, dtype=np.uint8).tobytes()
    p = tmp_path / "pcm.wav"
    with wave.open(str(p), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(22050)
        f.writeframes(raw)
    want, sr = _wave_module_decode(p)
    assert sr == 22050 and len(want) == 5003
    check_file(p, want, 22050)
    if channels == 1:
        fmt = {2: "s16", 1: "u8"}[width]
        assert np.array_equal(bits(want), bits(restate(np.frombuffer(raw, INPUT_FORMATS[fmt]), fmt, 1)))


def test_an_unknown_tag_is_refused_by_name(tmp_path):
    p = write_riff(tmp_path / "gsm.wav", 0x31, 1, 8000, 8, bytes(100))
    for fn in (read_wav, wav_duration):
        with pytest.raises(ValueError) as e:
            fn(p)
        assert "gsm.wav" in str(e.value) and "49" in str(e.value) and "0x0031" in str(e.value)
    p = write_riff(tmp_path / "ext.wav", 0x55, 2, 44100, 16, bytes(100), extensible=True)      # MP3 in an extensible header
    with pytest.raises(ValueError, match="0x0055"):
        read_wav(p)
    (tmp_path / "not.wav").write_bytes(b"RIFF\x04\0\0\0AVI ")
    with pytest.raises(ValueError, match="not.wav"):
        read_wav(tmp_path / "not.wav")
    p = write_riff(tmp_path / "f16.wav", 3, 1, 8000, 16, bytes(100))
    with pytest.raises(ValueError, match="16-bit"):
        read_wav(p)
