"""G.711, 8-bit and 32-bit client audio on the GPU: the push kernel's new instances (``dz_ring_push_rows_pcm``),
``dz_pcm_decode`` / ``functional.decode_pcm``, and ``StreamServer`` / ``WebSocketFrontEnd`` on top of them.

The sample is defined in ``include/diart_amd.h`` and restated here from the integer formulas (int64, then float32
operations in the stated order); the GPU must produce those bits whichever path of the kernel a frame takes."""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.functional import decode_pcm
from diart_amd.pipeline import AudioRing
from diart_amd.serve import INPUT_FORMATS, StreamServer, pcm_to_mono
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_streams

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NEW = ("u8", "s32", "ulaw", "alaw")


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
    v = np.asarray(v)
    if fmt == "f32":
        return v.astype(np.float32)
    if fmt == "s16":
        return np.multiply(v.astype(np.float32), np.float32(2.0 ** -15), dtype=np.float32)
    if fmt == "u8":
        return np.multiply(np.subtract(v.astype(np.float32), np.float32(128.0), dtype=np.float32),
                           np.float32(2.0 ** -7), dtype=np.float32)
    if fmt == "s32":
        return np.multiply(v.astype(np.int64).astype(np.float32), np.float32(2.0 ** -31), dtype=np.float32)
    lin = ulaw_linear(v) if fmt == "ulaw" else alaw_linear(v)
    return np.multiply(lin.astype(np.float32), np.float32(2.0 ** -15), dtype=np.float32)


def restate(values, fmt, channels):
    """float32 mono of ``values`` (..., frames, channels): ((c0 + c1) + c2 ...) / channels of the formats' samples,
    every operation rounded to float32."""
    v = to_float(values, fmt)
    if channels == 1:
        return v[..., 0]
    acc = v[..., 0]
    for c in range(1, channels):
        acc = np.add(acc, v[..., c], dtype=np.float32)
    return np.divide(acc, np.float32(channels), dtype=np.float32)


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    want = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32))
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.view(torch.int32))


def raw_blocks(rng, fmt, channels, pushes, k, hop):
    """(pushes, k, hop, channels) random values; the first and last frame of every row and the frames either side of
    every 16-frame boundary (a lane's span in the 1-byte kernels) carry the extreme codes."""
    edge = np.unique(np.concatenate([[0, hop - 1], np.arange(16, hop, 16) - 1, np.arange(16, hop, 16)]))
    if fmt == "s32":
        a = rng.integers(-2 ** 31, 2 ** 31, size=(pushes, k, hop, channels), dtype=np.int64).astype("<i4")
        ext = np.array([-2 ** 31, 2 ** 31 - 1, 0x7fffffc0, 0x7fffffbf], dtype="<i4")
    else:
        a = rng.integers(0, 256, size=(pushes, k, hop, channels), dtype=np.uint8)
        ext = np.array([0x00, 0x80, 0x7F, 0xFF], dtype=np.uint8)
    a[:, :, edge, :] = ext[(np.arange(len(edge))[:, None] + np.arange(channels)[None, :]) % 4]
    a[:, :, edge[::3], :] = ext[(np.arange(len(edge[::3])) % 4)][:, None]            # whole frames of one extreme
    return a


@pytest.mark.parametrize("fmt", NEW)
@pytest.mark.parametrize("hop", [4000, 4112, 22050])
def test_ring_push_of_the_new_formats_equals_the_definition(gpu, hop, fmt):
    """hop 4 000: the telephone block, no multiple of a kernel block; 4 112 = 257 x 16: one lane past a wave's 1 024
    frames and 16 frames for it; 22 050: every other ring position is off the 16-byte boundary (single-frame path).
    1 / 2 / 3 / 8 channels; pageable, pinned and device blocks; rows 16-byte aligned and one value off; 12 pushes into
    a ring of 10 blocks (row 1 joins one push late, so the rows sit at different positions)."""
    n, W, pushes = 3, 10 * hop, 12
    rng = np.random.default_rng(hop + len(fmt))
    dtype = INPUT_FORMATS[fmt]
    per16 = 16 // dtype.itemsize
    out = torch.empty(n, W, device=gpu)
    for channels in (1, 2, 3, 8):
        a = raw_blocks(rng, fmt, channels, pushes, n, hop)
        mono = restate(a, fmt, channels)                                     # (pushes, n, hop), shared by the variants
        rows_of = [[2, 0] if t == 0 else [2, 0, 1] for t in range(pushes)]
        want = np.stack([np.concatenate([mono[t, rows_of[t].index(r)] for t in range(pushes) if r in rows_of[t]])[-W:]
                         for r in range(n)])
        values = hop * channels
        for where in ("pageable", "pinned", "device"):
            for off_by in (0, 1):
                stride = -(-values // per16) * per16 + off_by
                back = torch.zeros((pushes, n, stride), dtype=torch.from_numpy(np.zeros(0, dtype)).dtype)
                back[:, :, :values] = torch.from_numpy(a.reshape(pushes, n, values))
                back = back.pin_memory() if where == "pinned" else back.to(gpu) if where == "device" else back
                ring = AudioRing(n, W, hop, slack_blocks=0, device=gpu)
                for t in range(pushes):
                    blk = back[t, :len(rows_of[t]), :values]
                    assert blk.stride(0) == stride
                    if fmt == "s32" and t % 2:
                        ring.push_rows(blk, rows_of[t], channels=channels)                  # inferred from int32
                    elif t % 3 == 2:
                        ring.push_rows(blk.view(len(rows_of[t]), hop, channels) if off_by == 0 and stride == values
                                       else blk, rows_of[t], channels=channels, format=fmt)
                    else:
                        ring.push_rows(blk, rows_of[t], channels=channels, format=fmt)
                assert [ring.filled_row(r) for r in range(n)] == [W] * n
                got = ring.gather([1, 2, 0], out)
                assert same_bits(got, want[[1, 2, 0]]), (fmt, channels, where, off_by)     # (.cpu() waits for the GPU)
                del ring


def test_push_rows_format_argument(gpu):
    hop = 4000
    ring = AudioRing(2, 10 * hop, hop, slack_blocks=0, device=gpu)
    u8 = torch.zeros(1, hop, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ring.push_rows(u8, [0])                                   # bytes mean nothing without a format
    with pytest.raises(TypeError):
        ring.push_rows(u8, [0], format="s16")
    with pytest.raises(TypeError):
        ring.push_rows(torch.zeros(1, hop, dtype=torch.int16), [0], format="ulaw")
    with pytest.raises(ValueError):
        ring.push_rows(u8, [0], format="mulaw")
    with pytest.raises(TypeError):
        ring.push_rows(torch.zeros(1, hop, dtype=torch.float64), [0])
    assert ring.filled_row(0) == 0
    arr = (C.c_int * 1)(0)
    for bad in (-1, 6, 99):
        rc = ring._lib.dz_ring_push_rows_pcm(ring._h, u8.data_ptr(), hop, bad, 1, 0, arr, 1,
                                             torch.cuda.current_stream(gpu).cuda_stream)
        assert rc != 0 and b"unknown format" in ring._lib.dz_last_error()
    assert ring.filled_row(0) == 0


def test_decode_pcm_of_every_code(gpu):
    frames = 4099
    i = np.arange(frames)
    for fmt in ("u8", "ulaw", "alaw"):
        mono = (i % 256).astype(np.uint8)[:, None]
        stereo = np.stack([i % 256, (i * 7 + i // 256 * 37 + 3) % 256], axis=1).astype(np.uint8)
        for a in (mono, stereo):
            ch = a.shape[1]
            want = restate(a, fmt, ch)
            assert same_bits(decode_pcm(a.reshape(-1), fmt, ch, device=gpu), want)
            assert same_bits(decode_pcm(a.tobytes(), fmt, ch, device=gpu), want)
            dev = torch.from_numpy(a).to(gpu)
            got = decode_pcm(dev, fmt, ch)
            assert got.device == dev.device and got.dtype == torch.float32 and same_bits(got, want)
            # a view one frame in: the source is not 16-byte aligned, every frame takes the single-frame path
            assert same_bits(decode_pcm(dev[1:], fmt, ch), want[1:])
    rng = np.random.default_rng(0)
    # the lane body the decode shares with the push: a lane's F = 16 / itemsize frames, one short, one over, one alone,
    # and 256 F + 3 (a second block whose only lane holds a ragged end), against the host definition
    for fmt, dtype in INPUT_FORMATS.items():
        F = 16 // dtype.itemsize
        for ch in (1, 3):
            for n_frames in (1, F - 1, F, F + 1, 256 * F + 3):
                v = rng.integers(0, 2 ** (8 * dtype.itemsize), size=n_frames * ch, dtype=np.uint64)
                v = v.astype(f"<u{dtype.itemsize}").view(dtype)
                if fmt == "f32" and ch > 1:
                    v = rng.uniform(-1, 1, size=n_frames * ch).astype(np.float32)     # (a sum of NaNs has no one payload)
                assert same_bits(decode_pcm(v, fmt, ch, device=gpu), pcm_to_mono(v, fmt, ch)), (fmt, ch, n_frames)
    s32 = raw_blocks(rng, "s32", 2, 1, 1, frames)[0, 0]
    assert same_bits(decode_pcm(s32, "s32", 2, device=gpu), restate(s32, "s32", 2))
    assert same_bits(decode_pcm(s32[:, :1].copy(), "s32", 1, device=gpu), restate(s32[:, :1], "s32", 1))
    s16 = rng.integers(-32768, 32768, size=(frames, 3), dtype=np.int16)
    s16[0], s16[-1] = -32768, 32767
    assert same_bits(decode_pcm(s16, "s16", 3, device=gpu), pcm_to_mono(s16.reshape(-1), "s16", 3))
    f32 = rng.integers(0, 2 ** 32, size=frames, dtype=np.uint32).view(np.float32)        # any bits: mono is a copy
    assert same_bits(decode_pcm(f32, "f32", device=gpu), pcm_to_mono(f32, "f32", 1))
    f2 = rng.uniform(-1, 1, size=(frames, 2)).astype(np.float32)
    assert same_bits(decode_pcm(f2, "f32", 2, device=gpu), pcm_to_mono(f2.reshape(-1), "f32", 2))
    for bad in (lambda: decode_pcm(s16, "ulaw", 1, device=gpu), lambda: decode_pcm(bytes(5), "ulaw", 2, device=gpu),
                lambda: decode_pcm(bytes(6), "s32", 1, device=gpu), lambda: decode_pcm(bytes(8), "mulaw", device=gpu),
                lambda: decode_pcm(b"", "u8", device=gpu), lambda: decode_pcm(bytes(8), "u8", 9, device=gpu)):
        with pytest.raises(ValueError):
            bad()


def test_s16_and_plain_float_pushes_write_what_they_wrote(gpu):
    """The paths from before the new formats: an s16 stereo push gives the bits of ``pcm_to_mono``, a mono float push
    through the PCM entry the bits of ``dz_ring_push_rows`` (any bits)."""
    n, hop = 2, 8000
    W = 10 * hop
    rng = np.random.default_rng(7)
    s16, plain, pcm = (AudioRing(n, W, hop, slack_blocks=0, device=gpu) for _ in range(3))
    hist = np.zeros((n, 0), dtype=np.float32)
    fhist = np.zeros((n, 0), dtype=np.float32)
    for t in range(11):
        a = rng.integers(-32768, 32768, size=(n, hop, 2), dtype=np.int16)
        a[0, 0], a[1, -1] = -32768, 32767
        blk = torch.from_numpy(a.reshape(n, -1))
        s16.push_rows(blk.to(gpu) if t % 2 else blk, [1, 0], channels=2)
        hist = np.concatenate([hist, np.stack([pcm_to_mono(a[1].reshape(-1), "s16", 2),
                                               pcm_to_mono(a[0].reshape(-1), "s16", 2)])], axis=1)[:, -W:]
        bits = rng.integers(0, 2 ** 32, size=(n, hop), dtype=np.uint32).view(np.float32)
        fhist = np.concatenate([fhist, bits], axis=1)[:, -W:]
        f = torch.from_numpy(bits)
        f = f.to(gpu) if t % 2 else f
        plain.push_rows(f, [0, 1])
        arr = (C.c_int * n)(0, 1)
        assert pcm._lib.dz_ring_push_rows_pcm(pcm._h, f.data_ptr(), f.stride(0) * 4, 0, 1, int(f.is_cuda), arr, n,
                                              torch.cuda.current_stream(gpu).cuda_stream) == 0
    out = torch.empty(n, W, device=gpu)
    assert same_bits(s16.gather([0, 1], out), hist)          # (block row 0 went to ring row 1)
    a = plain.gather([0, 1], out).clone()
    assert torch.equal(a.view(torch.int32), pcm.gather([0, 1], out).view(torch.int32))
    assert same_bits(a, fhist)                               # the two entry points share their push path: numpy too


# ---------------------------------------------------------------------------------------------- StreamServer
def encode_nearest(x, linear):
    """Quantise ``x`` (float, full scale 1.0) to the code of ``linear`` (the 256 decoded values) nearest to it."""
    order = np.argsort(linear, kind="stable")
    levels = linear[order].astype(np.float64)
    v = np.clip(np.asarray(x, dtype=np.float64) * 32768.0, levels[0], levels[-1])
    hi = np.clip(np.searchsorted(levels, v), 1, 255)
    pick = np.where(v - levels[hi - 1] <= levels[hi] - v, hi - 1, hi)
    return order[pick].astype(np.uint8)


@pytest.fixture(scope="module")
def telephone():
    """Two streams of synthetic speech at 8 kHz, 11.5 s: 14 windows each."""
    out = {}
    for i, k in enumerate(("ann", "ben")):
        x = synth_streams(1, 11.5, seed0=900 + i)[0]
        out[k] = R.resample(x, 16000, 8000).astype(np.float32)[:92000]
    return out


def _server(gpu, pipeline="diarization", **kw):
    seg = M.HipSegmentation(synth_segmentation_state(), max_batch=2)
    emb = M.HipEmbedding(synth_embedding_state(), max_batch=2) if pipeline == "diarization" else None
    extra = {"tau_active": 0.5} if pipeline == "vad" else {}
    return StreamServer(seg, emb, max_streams=2, device=gpu, pipeline=pipeline, input_sample_rate=8000, **extra, **kw)


def _serve(srv, audio, frame_values=1):
    """Both streams push irregular numbers of whole frames, one step per round; returns each stream's RTTM."""
    rng = np.random.default_rng(4)
    pos = {k: 0 for k in audio}
    for k in audio:
        srv.open(k)
    steps = 0
    while any(pos[k] < len(audio[k]) for k in audio):
        for k in audio:
            m = int(rng.integers(1000, 9000)) * frame_values
            srv.push(k, audio[k][pos[k]:pos[k] + m])
            pos[k] += m
        steps += bool(srv.step())
    steps += srv.drain()
    assert not srv.step_errors and steps >= 14
    assert all(st.emitted == 14 for st in srv._streams.values())
    return {k: srv.close(k).to_rttm() for k in audio}


@pytest.mark.parametrize("pipeline,rings", [("diarization", True), ("diarization", False), ("vad", True)])
def test_ulaw_stereo_server_equals_a_float_server_fed_the_decoded_audio(gpu, telephone, pipeline, rings):
    rng = np.random.default_rng(11)
    lin = ulaw_linear(np.arange(256))
    raw = {k: np.stack([encode_nearest(0.9 * x + 0.01 * rng.standard_normal(len(x)), lin),
                        encode_nearest(0.6 * x + 0.01 * rng.standard_normal(len(x)), lin)], axis=1)
           for k, x in telephone.items()}
    mono = {k: pcm_to_mono(a.reshape(-1), "ulaw", 2) for k, a in raw.items()}
    assert all(np.array_equal(mono[k].view(np.uint32), restate(a, "ulaw", 2).view(np.uint32)) for k, a in raw.items())
    ulaw = _server(gpu, pipeline, input_format="ulaw", input_channels=2, device_rings=rings)
    f32 = _server(gpu, pipeline)
    assert (ulaw.rings is not None) == rings and f32.rings is not None and ulaw.step_samples == 4000
    got = _serve(ulaw, {k: a.reshape(-1) for k, a in raw.items()}, frame_values=2)
    want = _serve(f32, mono)
    assert got == want and any(want.values())


def test_websocket_binary_alaw_frames(gpu, telephone):
    """``WebSocketFrontEnd`` on a real socket in front of an A-law mono server at 8 kHz: binary messages of raw G.711
    bytes; the RTTM lines that come back are those of a float server stepped directly on the decoded audio."""
    from test_ws import Client
    from diart_amd.ws import WebSocketFrontEnd
    lin = alaw_linear(np.arange(256))
    raw = {k: encode_nearest(x[:72000], lin) for k, x in telephone.items()}           # 9 s: 9 windows per stream

    direct, want = _server(gpu), {k: [] for k in raw}
    for k in raw:
        direct.open(k)
        direct.push(k, pcm_to_mono(raw[k], "alaw", 1))
    while True:
        out = direct.step()
        if not out:
            break
        for k, ann in out.items():
            want[k] += [l for l in ann.to_rttm().splitlines() if l]
    assert all(want.values())

    srv = _server(gpu, input_format="alaw")
    fe = WebSocketFrontEnd(srv, port=0).start()
    try:
        clients = {k: Client(fe.port, k) for k in raw}
        for k, c in clients.items():
            for pos in range(0, len(raw[k]), 8000):
                c.send(0x2, raw[k][pos:pos + 8000].tobytes())
        deadline = time.time() + 30
        while time.time() < deadline and sum(s.emitted for s in list(srv._streams.values())) < 18:
            time.sleep(0.05)
        assert sum(s.emitted for s in srv._streams.values()) == 18
        time.sleep(0.3)
        got = {k: [] for k in raw}
        for k, c in clients.items():
            c.s.settimeout(0.5)
            try:
                while True:
                    op, data = c.recv()
                    assert op == 0x1
                    got[k] += [l for l in data.decode().splitlines() if l]
            except (TimeoutError, OSError):
                pass
        assert not fe.errors
        assert got == want
    finally:
        fe.stop()
