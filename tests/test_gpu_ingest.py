"""Raw client audio on the GPU: ``dz_ring_push_rows_pcm`` (16-bit PCM and interleaved channels converted and averaged
by the push kernel), rings whose block is not a multiple of 4 samples (44.1 kHz, 22.05 kHz), and ``StreamServer`` /
``WebSocketFrontEnd`` on top of them.

The sample the ring holds is defined in ``include/diart_amd.h`` and restated here in numpy; the ring must hold those
bits.  For the server the gate is identity: ring mode and host-window mode hand the resampler the same float32
windows, and the resampler and the engines are batch-invariant by their own tests."""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.pipeline import AudioRing
from diart_amd.serve import StreamServer
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_streams

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


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


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    want = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32))
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.view(torch.int32))


def raw_block(rng, fmt, channels, k, hop):
    if fmt == "s16":
        a = rng.integers(-32768, 32768, size=(k, hop, channels), dtype=np.int16)
        a[0, 0], a[0, 1], a[0, hop - 1, 0], a[-1, hop - 1] = -32768, 32767, -32768, 32767
        return a
    a = rng.uniform(-1, 1, size=(k, hop, channels)).astype(np.float32)
    a[0, 5, channels - 1] = np.nan             # one channel: the frame is NaN
    a[-1, hop - 1, 0] = np.inf
    return a


def place(a: np.ndarray, where: str, flat: bool, gpu):
    """The block as a pageable / pinned host tensor or a device tensor, (k, hop * C) or (k, hop, C)."""
    t = torch.from_numpy(a.reshape(a.shape[0], -1) if flat else a)
    if where == "pinned":
        return t.pin_memory()
    return t.to(gpu) if where == "device" else t


@pytest.mark.parametrize("hop", [22050, 11025, 8000])
def test_push_rows_of_raw_blocks_equals_the_definition(gpu, hop):
    """f32 / s16, 1 / 2 / 5 channels, from pageable, pinned and device memory, rows scrambled, streams at different
    fill levels, more than three wrap-arounds of the ring: every complete window, bit for bit."""
    n, W = 5, 10 * hop
    ring = AudioRing(n, W, hop, slack_blocks=0, device=gpu)
    rng = np.random.default_rng(hop)
    hist = [np.zeros(0, dtype=np.float32) for _ in range(n)]
    out = torch.empty(n, W, device=gpu)
    combos = [(f, c) for f in ("f32", "s16") for c in (1, 2, 5)]
    places = ("pageable", "pinned", "device")
    checked = 0
    for it in range(54):
        fmt, ch = combos[it % 6]
        where = places[(it // 6) % 3]
        rows = rng.permutation(n)[:int(rng.integers(2, n + 1))].tolist()        # scrambled order
        if it < 4:
            rows = [r for r in rows if r != 3] or [0]                          # row 3 joins late
        a = raw_block(rng, fmt, ch, len(rows), hop)
        blk = place(a, where, flat=bool((it // 18) % 2), gpu=gpu)
        ring.push_rows(blk, rows, channels=ch)
        for j, r in enumerate(rows):
            hist[r] = np.concatenate([hist[r], restate(a[j], fmt, ch)])[-W:]
        assert all(ring.filled_row(r) == len(hist[r]) for r in range(n))
        full = [r for r in range(n) if len(hist[r]) == W]
        if full:
            full = rng.permutation(full).tolist()
            assert same_bits(ring.gather(full, out), np.stack([hist[r] for r in full])), (it, fmt, ch, where)
            checked += 1
        torch.cuda.synchronize()               # the zero-copy read of a pinned block is over
    assert checked > 30 and min(ring.filled_row(r) for r in range(n)) == W
    # a gather into rows that are not 16-byte aligned (a view one float in)
    if hop % 4:
        wide = torch.empty(n, W + 3, device=gpu)
        assert same_bits(ring.gather([1, 0], wide[:, 1:W + 1]), np.stack([hist[1], hist[0]]))
        with pytest.raises(RuntimeError, match="16-byte"):
            ring.raw()                          # no in-place window: dz_ring_window says why


@pytest.mark.parametrize("hop", [22050, 11025])
def test_lock_step_push_and_snapshot_on_an_unaligned_ring(gpu, hop):
    n, W = 3, 10 * hop
    ring = AudioRing(n, W, hop, slack_blocks=2, device=gpu)
    rng = np.random.default_rng(1)
    hist = np.zeros((n, 0), dtype=np.float32)
    for t in range(27):
        blk = rng.standard_normal((n, hop)).astype(np.float32)
        full = ring.push(torch.from_numpy(blk).to(gpu) if t % 2 else blk)
        hist = np.concatenate([hist, blk], axis=1)[:, -W:]
        assert full == (hist.shape[1] == W)
        if full:
            assert same_bits(ring.snapshot(), hist)
    ring.push_rows(torch.from_numpy(hist[:1, :hop].copy()), [1])      # plain float rows on such a ring
    want = np.concatenate([hist[1], hist[0, :hop]])[-W:]
    assert same_bits(ring.gather([1], torch.empty(1, W, device=gpu)), want[None])


def test_mono_float_equals_the_plain_push_on_an_aligned_ring(gpu):
    """``dz_ring_push_rows_pcm`` with one float32 channel writes the bits ``dz_ring_push_rows`` writes — any bits:
    the block is random 32-bit patterns (NaNs with payloads, denormals).  The two entry points share their push path,
    so both rings are also held against the block history in numpy."""
    n, hop = 4, 8000
    W = 10 * hop
    plain, pcm = AudioRing(n, W, hop, slack_blocks=0, device=gpu), AudioRing(n, W, hop, slack_blocks=0, device=gpu)
    rng = np.random.default_rng(2)
    out = torch.empty(n, W, device=gpu)
    hist = [np.zeros(0, dtype=np.float32) for _ in range(n)]
    for it in range(23):
        rows = rng.permutation(n)[:int(rng.integers(1, n + 1))].tolist()
        bits = rng.integers(0, 2 ** 32, size=(len(rows), hop), dtype=np.uint32).view(np.float32)
        for j, r in enumerate(rows):
            hist[r] = np.concatenate([hist[r], bits[j]])[-W:]
        blk = torch.from_numpy(bits)
        blk = blk.to(gpu) if it % 2 else blk
        plain.push_rows(blk, rows)
        arr = (C.c_int * len(rows))(*rows)
        rc = pcm._lib.dz_ring_push_rows_pcm(pcm._h, blk.data_ptr(), blk.stride(0) * 4, 0, 1, int(blk.is_cuda), arr,
                                            len(rows), torch.cuda.current_stream(gpu).cuda_stream)
        assert rc == 0
        full = [r for r in range(n) if plain.filled_row(r) == W]
        assert [r for r in range(n) if pcm.filled_row(r) == W] == full
        if full:
            a = plain.gather(full, out).clone()
            assert torch.equal(a.view(torch.int32), pcm.gather(full, out).view(torch.int32))
            assert same_bits(a, np.stack([hist[r] for r in full]))          # and both hold the blocks' bits
    assert full


def test_a_reopened_row_keeps_nothing_of_its_previous_occupant(gpu):
    hop, n = 22050, 2
    W = 10 * hop
    ring = AudioRing(n, W, hop, slack_blocks=0, device=gpu)
    for _ in range(13):                                        # the first occupant: 13 blocks of 7.0 (write position 3)
        ring.push_rows(torch.full((n, hop), 7.0), [0, 1])
    ring.reset_row(0)
    assert ring.filled_row(0) == 0 and ring.filled_row(1) == W
    rng = np.random.default_rng(3)
    new = rng.integers(-32768, 32768, size=(10, hop, 2), dtype=np.int16)
    for t in range(10):
        with pytest.raises(RuntimeError):
            ring.gather([0], torch.empty(1, W, device=gpu))    # incomplete: refused
        ring.push_rows(torch.from_numpy(new[t:t + 1]), [0], channels=2)
    got = ring.gather([0, 1], torch.empty(2, W, device=gpu))
    assert same_bits(got[0], restate(new, "s16", 2)) and bool((got[1] == 7.0).all())


# ---------------------------------------------------------------------------------------------- StreamServer
def _speech(rate, seed0, lengths=(11.0, 8.5, 7.0)):
    out = {}
    for i, (k, v) in enumerate(zip(("ann", "ben", "cy"), lengths)):
        x = synth_streams(1, v, seed0=seed0 + i)[0]
        out[k] = x if rate == 16000 else R.resample(x, 16000, rate).astype(np.float32)
    return out


def _server(gpu, pipeline="diarization", **kw):
    seg = M.HipSegmentation(synth_segmentation_state(), max_batch=4)
    emb = M.HipEmbedding(synth_embedding_state(), max_batch=4) if pipeline == "diarization" else None
    extra = {"tau_active": 0.5} if pipeline == "vad" else {}
    return StreamServer(seg, emb, max_streams=4, device=gpu, pipeline=pipeline, **extra, **kw)


def _serve(srv, audio, frame_values=1, seed=4):
    """Three streams join late and push irregular amounts (whole frames); returns each stream's RTTM."""
    rng = np.random.default_rng(seed)
    rate = srv.input_sample_rate
    pos = {k: 0 for k in audio}
    join_at = dict(zip(audio, (0, 2, 5)))
    tick = 0
    while any(pos[k] < len(audio[k]) for k in audio):
        for k in audio:
            if tick == join_at[k]:
                srv.open(k)
            if tick >= join_at[k] and pos[k] < len(audio[k]):
                m = int(rng.integers(rate // 8, rate * 2)) * frame_values
                srv.push(k, audio[k][pos[k]:pos[k] + m])
                pos[k] += m
        srv.step()
        tick += 1
    srv.drain()
    assert not srv.step_errors
    return {k: srv.close(k).to_rttm() for k in audio}


@pytest.mark.parametrize("rate,pipeline", [(44100, "diarization"), (44100, "vad"), (22050, "diarization")])
def test_rings_at_44100_hz_equal_host_window_mode(gpu, rate, pipeline):
    audio = _speech(rate, 80)
    ring = _server(gpu, pipeline, input_sample_rate=rate, device_rings="all")
    host = _server(gpu, pipeline, input_sample_rate=rate, device_rings=False)
    assert ring.rings is not None and host.rings is None and ring.step_samples == rate // 2
    got, want = _serve(ring, audio), _serve(host, audio)
    assert got == want and any(want.values())


def _stereo_s16(x, seed):
    """Two microphones' worth of a mono stream: different gains and a little noise each, 16-bit."""
    rng = np.random.default_rng(seed)
    ch = np.stack([0.9 * x + 0.01 * rng.standard_normal(len(x)), 0.6 * x + 0.01 * rng.standard_normal(len(x))], axis=1)
    return np.clip(np.round(ch * 32768.0), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("rings", [True, False])
def test_s16_stereo_server_equals_a_float_server_fed_the_converted_audio(gpu, rings):
    raw = {k: _stereo_s16(x, i) for i, (k, x) in enumerate(_speech(48000, 60).items())}
    mono = {k: restate(a, "s16", 2) for k, a in raw.items()}
    s16 = _server(gpu, input_format="s16", input_channels=2, input_sample_rate=48000, device_rings=rings)
    f32 = _server(gpu, input_sample_rate=48000)
    assert (s16.rings is not None) == rings and f32.rings is not None
    got = _serve(s16, {k: a.reshape(-1) for k, a in raw.items()}, frame_values=2)
    want = _serve(f32, mono)
    assert got == want and any(want.values())
    # (n, 2) pushes and 1-D pushes that end inside a frame: the same stream
    again = _server(gpu, input_format="s16", input_channels=2, input_sample_rate=48000, device_rings=rings)
    again.open("ann")
    flat = raw["ann"].reshape(-1)
    again.push("ann", raw["ann"][:30001])
    again.push("ann", flat[60002:90003])
    again.push("ann", flat[90003:])
    again.drain()
    assert again.close("ann").to_rttm() == want["ann"]


def test_s16_stereo_at_44100_hz_on_rings(gpu):
    """Everything at once: 16-bit stereo, a block of 22 050 frames, rings against host-window mode."""
    raw = {k: _stereo_s16(x, i).reshape(-1) for i, (k, x) in enumerate(_speech(44100, 40).items())}
    kw = dict(input_format="s16", input_channels=2, input_sample_rate=44100)
    ring, host = _server(gpu, device_rings="all", **kw), _server(gpu, device_rings=False, **kw)
    assert ring.rings is not None and host.rings is None
    got, want = _serve(ring, raw, frame_values=2), _serve(host, raw, frame_values=2)
    assert got == want and any(want.values())


def test_a_reopened_slot_of_a_44100_hz_server(gpu):
    """One slot, two occupants with different amounts of audio: the second one's RTTM is that of a fresh server."""
    audio = _speech(44100, 20, lengths=(7.3, 9.0))
    srv = _server(gpu, "vad", input_sample_rate=44100, device_rings="all")
    srv.open("first")
    assert srv._streams["first"].slot == 0
    srv.push("first", audio["ann"])
    srv.drain()
    srv.close("first")
    srv.open("second")
    assert srv._streams["second"].slot == 0
    srv.push("second", audio["ben"])
    srv.drain()
    fresh = _server(gpu, "vad", input_sample_rate=44100, device_rings="all")
    fresh.open("second")
    fresh.push("second", audio["ben"])
    fresh.drain()
    got, want = srv.close("second").to_rttm(), fresh.close("second").to_rttm()
    assert got == want and want


def test_websocket_binary_s16_stereo_frames(gpu):
    """``WebSocketFrontEnd`` on a real socket in front of an s16 stereo server: binary messages of raw 16-bit
    frames; the RTTM lines that come back are those of an identical server stepped directly."""
    from test_ws import Client
    from diart_amd.ws import WebSocketFrontEnd
    raw = {k: _stereo_s16(synth_streams(1, 9.0, seed0=700 + i)[0], i) for i, k in enumerate(("ann", "ben"))}

    def make():
        return StreamServer(M.HipSegmentation(synth_segmentation_state(), max_batch=3),
                            M.HipEmbedding(synth_embedding_state(), max_batch=3), max_streams=3, device=gpu,
                            input_format="s16", input_channels=2)

    direct, want = make(), {k: [] for k in raw}
    for k in raw:
        direct.open(k)
        direct.push(k, raw[k])
    while True:
        out = direct.step()
        if not out:
            break
        for k, ann in out.items():
            want[k] += [l for l in ann.to_rttm().splitlines() if l]
    assert all(want.values())

    srv = make()
    fe = WebSocketFrontEnd(srv, port=0).start()
    try:
        clients = {k: Client(fe.port, k) for k in raw}
        for k, c in clients.items():
            for pos in range(0, len(raw[k]), 16000):
                c.send(0x2, raw[k][pos:pos + 16000].astype("<i2").tobytes())
        deadline = time.time() + 30
        while time.time() < deadline and sum(s.emitted for s in list(srv._streams.values())) < 18:
            time.sleep(0.05)
        assert sum(s.emitted for s in srv._streams.values()) == 18      # 9 s = 9 windows per stream
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
        # half a stereo frame: the connection is dropped with an error, the server lives on
        bad = Client(fe.port, "odd")
        bad.send(0x2, b"\x00\x00")
        deadline = time.time() + 10
        while time.time() < deadline and not fe.errors:
            time.sleep(0.05)
        assert fe.errors and "whole number" in fe.errors[-1][1]
    finally:
        fe.stop()
