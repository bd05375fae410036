"""``StreamServer`` ingest of 16-bit, multi-channel audio, host side: windows that reach a custom engine, the argument
checks, the websocket decoding.  No GPU: the server runs on ``engine=callable`` as in ``test_serve.py``.

The sample a server hands its models is defined in ``include/diart_amd.h`` (``dz_ring_push_rows_pcm``) and restated
here in numpy, independently of ``diart_amd.serve.pcm_to_mono``."""
import base64

import numpy as np
import pytest

from diart_amd.serve import StreamServer
from diart_amd.ws import decode_audio

STEP, WINDOW = 8000, 80000


def restate(values, fmt, channels):
    """float32 mono of interleaved ``values``: s16 -> float(v) * (1 / 32768); several channels ->
    ((c0 + c1) + c2 ...) / channels, every operation rounded to float32."""
    v = np.asarray(values).reshape(-1, channels)
    if fmt == "s16":
        v = v.astype(np.float32) * np.float32(2.0 ** -15)
    assert v.dtype == np.float32
    if channels == 1:
        return v[:, 0]
    acc = v[:, 0]
    for c in range(1, channels):
        acc = np.add(acc, v[:, c], dtype=np.float32)
    return np.divide(acc, np.float32(channels), dtype=np.float32)


def bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x.view(np.uint32)


def make_audio(rng, fmt, channels, frames):
    if fmt == "s16":
        a = rng.integers(-32768, 32768, size=(frames, channels), dtype=np.int16)
        a[3], a[4] = -32768, 32767                        # whole frames of the extremes
        a[5, 0], a[5, -1] = -32768, 32767
        a[STEP - 1], a[STEP] = 32767, -32768              # across a block boundary
        return a
    a = rng.uniform(-1, 1, size=(frames, channels)).astype(np.float32)
    a[7, channels - 1] = np.nan                           # a NaN in one channel makes that frame NaN
    a[WINDOW + 11, 0] = np.nan
    return a


class Recorder:
    def __init__(self):
        self.windows = {}

    def __call__(self, windows, starts, slots):
        assert windows.dtype == np.float32
        for w, t, s in zip(windows, starts, slots):
            self.windows.setdefault(s, []).append((float(t), w.copy()))
        return [np.zeros((0, 3)) for _ in slots]


@pytest.mark.parametrize("fmt,channels", [("s16", 1), ("s16", 2), ("f32", 2), ("f32", 5)])
def test_windows_equal_the_definition_bit_for_bit(fmt, channels):
    rng = np.random.default_rng(channels * 10 + (fmt == "s16"))
    rec = Recorder()
    srv = StreamServer(None, None, max_streams=3, engine=rec, input_format=fmt, input_channels=channels)
    frames = {"a": WINDOW + 5 * STEP + 123, "b": WINDOW + 2 * STEP, "c": WINDOW + 3 * STEP + 7999}
    audio = {k: make_audio(rng, fmt, channels, n) for k, n in frames.items()}
    for k in audio:
        srv.open(k)
    # "a": 1-D pushes of irregular numbers of VALUES (so frames are split across calls when channels > 1);
    # "b": 2-D (n, channels) pushes; "c": one 1-D push
    flat = audio["a"].reshape(-1)
    lo = 0
    while lo < flat.size:
        n = int(rng.integers(1, 3 * STEP * channels)) | 1       # odd: splits a stereo frame
        srv.push("a", flat[lo:lo + n])
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
        got = rec.windows[slots[k]]
        assert len(got) == (frames[k] - WINDOW) // STEP + 1
        for i, (t, w) in enumerate(got):
            assert abs(t - 0.5 * i) < 1e-9
            assert np.array_equal(bits(w), bits(mono[i * STEP:i * STEP + WINDOW])), (k, i)
    if fmt == "f32":
        assert np.isnan(rec.windows[slots["a"]][0][1][7])


def test_dtype_mismatch_and_bad_arguments_raise():
    eng = Recorder()
    f32 = StreamServer(None, None, max_streams=1, engine=eng)
    f32.open(0)
    with pytest.raises(ValueError):
        f32.push(0, np.zeros(10, dtype=np.int16))
    s16 = StreamServer(None, None, max_streams=1, engine=eng, input_format="s16", input_channels=2)
    s16.open(0)
    with pytest.raises(ValueError):
        s16.push(0, np.zeros(10, dtype=np.float32))
    with pytest.raises(ValueError):
        s16.push(0, np.zeros((10, 3), dtype=np.int16))           # not (n, 2)
    assert s16.push(0, np.zeros((10, 2), dtype=np.int16)) == 0
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            StreamServer(None, None, engine=eng, input_channels=bad)
    for bad in ("s24", "mulaw", "int16", None):
        with pytest.raises(ValueError):
            StreamServer(None, None, engine=eng, input_format=bad)
    with pytest.raises(ValueError):
        StreamServer(None, None, engine=eng, device_rings="some")


def test_defaults_are_untouched():
    srv = StreamServer(None, None, max_streams=2, engine=Recorder())
    assert (srv.input_format, srv.input_channels, srv.rings) == ("f32", 1, None)
    # float64 and lists of floats are cast as before
    srv.open(0)
    srv.push(0, [0.25] * 10)
    srv.push(0, np.full(10, 0.5))
    assert srv._streams[0].buffer.dtype == np.float32 and srv._streams[0].buffer.size == 20


def test_44100_hz_stays_in_host_window_mode_without_a_gpu_engine():
    rec = Recorder()
    srv = StreamServer(None, None, max_streams=1, engine=rec, sample_rate=44100, input_sample_rate=44100)
    assert srv.rings is None and srv.step_samples == 22050 and srv.chunk_samples == 220500
    srv.open("x")
    x = np.random.default_rng(0).uniform(-1, 1, 220500 + 22050).astype(np.float32)
    srv.push("x", x)
    srv.drain()
    (t0, w0), (t1, w1) = rec.windows[0]
    assert np.array_equal(w0, x[:220500]) and np.array_equal(w1, x[22050:]) and (t0, t1) == (0.0, 0.5)


def test_decode_audio_s16():
    x = np.array([[-32768, 32767], [1, -1], [0, 12345]], dtype="<i2")
    raw = x.tobytes()
    for msg in (raw, base64.b64encode(raw).decode()):
        assert np.array_equal(decode_audio(msg, "s16", 2), x.reshape(-1))
        assert np.array_equal(decode_audio(msg, "s16"), x.reshape(-1))
        assert decode_audio(msg, "s16", 2).dtype == np.int16
    for msg in (raw[:-1], base64.b64encode(raw[:-1]).decode()):       # an odd number of bytes
        with pytest.raises(ValueError):
            decode_audio(msg, "s16")
    for msg in (raw[:-2], base64.b64encode(raw[:-2]).decode()):       # half a stereo frame
        with pytest.raises(ValueError):
            decode_audio(msg, "s16", 2)
        decode_audio(msg, "s16", 1)
    f = np.arange(6, dtype="<f4")
    assert np.array_equal(decode_audio(f.tobytes(), "f32", 2), f)
    with pytest.raises(ValueError):
        decode_audio(f.tobytes()[:-4], "f32", 2)                      # half a stereo float frame
    assert np.array_equal(decode_audio(f.tobytes()), f)               # defaults: the reference's wire format
