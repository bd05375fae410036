"""VoiceActivityDetection on the N-stream engine: the speech track written by the segmentation head
(``dz_seg_forward_vad``), ``VadBatch`` and ``StreamServer(pipeline="vad")``.  Per stream the engine must produce what
that stream's own ``VoiceActivityDetection`` produces at batch 1 (reference blocks/vad.py:136-191)."""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.blocks import VoiceActivityDetection, VoiceActivityDetectionConfig
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.features import SlidingWindow, SlidingWindowFeature
from diart_amd.pipeline import AudioRing, VadBatch
from diart_amd.synth import synth_segmentation_state, synth_streams

pytestmark = pytest.mark.gpu

W, SR = 80000, 16000
TAU = 0.5


@pytest.fixture(scope="module")
def states():
    return {False: synth_segmentation_state(seed=31), True: synth_segmentation_state(seed=77, powerset=True)}


def bits(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().contiguous().view(torch.int32).numpy()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equal, every NaN counted equal to a NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and np.array_equal(bits(a)[~na.numpy()], bits(b)[~nb.numpy()])


def tracks(ann):
    return sorted((s.start, s.end, str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("powerset", [False, True])
def test_forward_vad_is_the_max_over_speakers_bit_for_bit(gpu, states, precision, powerset):
    """The track equals torch.max(dz_seg_forward(...), -1) bit for bit and the scores beside it equal dz_seg_forward's,
    at batches 1, 3 and 64, in both precisions (f16x3: the fused MLP head; f32: seg_head_kernel, the other head)."""
    seg = M.HipSegmentation(states[powerset], max_batch=64, powerset=powerset, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(64, 5.0, seed0=500)).to(gpu)
    for b in (1, 3, 64):
        want = seg(x[:b])
        track, scores = seg.forward_vad(x[:b], return_scores=True)
        assert track.shape == (b, want.shape[1], 1) and track.is_cuda
        assert same_bits(scores, want), (precision, powerset, b)
        assert same_bits(track, torch.max(want, dim=-1, keepdim=True)[0]), (precision, powerset, b)
        assert not torch.isnan(track).any()
        if powerset:
            assert set(torch.unique(track).tolist()) <= {0.0, 1.0}
    assert torch.equal(seg.forward_vad(x[:3]), track[:3])          # (without the scores: same track)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("powerset", [False, True])
def test_forward_vad_of_a_nan_window(gpu, states, precision, powerset):
    """A window with a NaN sample: its track row is NaN wherever its score row has a NaN (torch.max propagates NaN;
    on the f16x3 path the whole row is NaN, like the reference), and the other rows are those of a batch without it."""
    seg = M.HipSegmentation(states[powerset], max_batch=4, powerset=powerset, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(4, 5.0, seed0=510)).to(gpu)
    clean, _ = seg.forward_vad(x, return_scores=True)
    x[1, 12345] = float("nan")
    want = seg(x)
    track, scores = seg.forward_vad(x, return_scores=True)
    assert same_bits(scores, want)
    assert same_bits(track, torch.max(want, dim=-1, keepdim=True)[0])
    nan_rows = torch.isnan(want).any(dim=-1)
    assert torch.equal(torch.isnan(track[..., 0]), nan_rows)
    if precision == "f16x3":
        assert bool(torch.isnan(track[1]).all())
    for i in (0, 2, 3):
        assert same_bits(track[i], clean[i])


# ---------------------------------------------------------------------------------------------------- the engine
def blocks_vad(states, powerset, precision, step, latency, gpu):
    cfg = VoiceActivityDetectionConfig(
        segmentation=M.SegmentationModel.from_state(states[powerset], max_batch=1, powerset=powerset,
                                                    precision=precision),
        step=step, latency=latency, tau_active=TAU, device=gpu)
    return VoiceActivityDetection(cfg)


def chunk(x, t, hop, step):
    return SlidingWindowFeature(x[t * hop:t * hop + W, None], SlidingWindow(start=t * step, duration=1 / SR,
                                                                            step=1 / SR))


def vad_engine(states, powerset, precision, n, gpu, step=0.5, latency=None, **kw):
    return VadBatch(M.HipSegmentation(states[powerset], max_batch=n, powerset=powerset, precision=precision), n,
                    tau_active=TAU, step=step, latency=latency, device=gpu, **kw)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("powerset", [False, True])
@pytest.mark.parametrize("step", [0.5, 0.25])
@pytest.mark.parametrize("latency", ["step", "duration"])
def test_engine_equals_per_stream_pipelines(gpu, states, precision, powerset, step, latency):
    """3 streams x 10 steps on 2 lanes: every step's speech turns (VadBatch.detect) equal those of the stream's own
    VoiceActivityDetection at batch 1; the step 0.25 engine reads its windows from a device ring (hop 4000)."""
    n, steps, hop = 3, 10, int(step * SR)
    lat = step if latency == "step" else 5.0
    audio = synth_streams(n, (W + (steps - 1) * hop) / SR, seed0=600 + int(powerset))
    pipe = vad_engine(states, powerset, precision, n, gpu, step, lat, lanes=2)
    assert pipe.depth == 2 and not pipe.throughput
    dev = torch.from_numpy(audio).to(gpu)
    ring = AudioRing(n, W, hop, device=gpu) if step == 0.25 else None
    got = []
    for t in range(steps):
        if ring is not None:
            if t == 0:
                for j in range(W // hop):
                    ring.push(dev[:, j * hop:(j + 1) * hop].contiguous())
            else:
                ring.push(dev[:, W + (t - 1) * hop:W + t * hop].contiguous())
            got.append(pipe.detect(ring))
        else:
            got.append(pipe.detect(dev[:, t * hop:t * hop + W]))
    spoken = 0
    for i in range(n):
        ref = blocks_vad(states, powerset, precision, step, lat, gpu)
        for t in range(steps):
            (want, _), = ref([chunk(audio[i], t, hop, step)])
            assert tracks(got[t][i]) == tracks(want), (i, t)
            assert all(lab == "speech" for lab in got[t][i].labels())
            spoken += len(tracks(want))
    assert spoken > 0, "no speech turn anywhere: the comparison shows nothing"


def test_partial_steps_and_resets_leave_other_streams_alone(gpu, states):
    """Steps over a subset of slots, and reset(slot), change nothing for the other streams; a reset stream restarts
    like a fresh pipeline (window start times from 0)."""
    n, steps, hop, step = 3, 10, 8000, 0.5
    audio = synth_streams(n, (W + (steps - 1) * hop) / SR, seed0=640)
    dev = torch.from_numpy(audio).to(gpu)
    full = vad_engine(states, False, "f16x3", n, gpu)
    part = vad_engine(states, False, "f16x3", n, gpu)
    fresh = vad_engine(states, False, "f16x3", n, gpu)
    restart = 5
    for t in range(steps):
        x = dev[:, t * hop:t * hop + W]
        want = full.detect(x)
        if t == 4:                      # stream 1 has no window this step, then starts over
            ticket = part.launch(x[[0, 2]].contiguous(), slots=[0, 2])
            part.finish(ticket)
            turns, nturns = ticket["tail"][4], ticket["tail"][5]
            got = {0: BatchedOutputTail.annotation(turns[0], int(nturns[0]), label="speech"),
                   2: BatchedOutputTail.annotation(turns[1], int(nturns[1]), label="speech")}
            part.reset(1)
        else:
            got = dict(enumerate(part.detect(x)))
        for i in (0, 2):
            assert tracks(got[i]) == tracks(want[i]), (t, i)
        if t >= restart:                # stream 1 after its reset: a fresh engine fed from window `restart` on
            again = fresh.detect(torch.stack([dev[1, t * hop:t * hop + W]] * n))
            assert tracks(got[1]) == tracks(again[1]), t


def test_launch_does_not_wait_for_the_gpu(gpu, states):
    """After its warm-up, VadBatch.launch returns while work queued before it is pending, and the step's track equals
    that of an engine that never waited."""
    n, hop = 4, 8000
    audio = torch.from_numpy(synth_streams(n, (W + 2 * hop) / SR, seed0=995)).to(gpu)
    pipe, ref = vad_engine(states, False, "f16x3", n, gpu), vad_engine(states, False, "f16x3", n, gpu)
    for p in (pipe, ref):
        p.finish(p.launch(audio[:, :W]))
    want = ref.finish(ref.launch(audio[:, hop:hop + W])).copy()
    cyc = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cyc)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    torch.cuda._sleep(int(cyc * 300.0 / max(ms, 1e-3)))       # ~0.3 s
    ev = torch.cuda.Event()
    ev.record()
    ticket = pipe.launch(audio[:, hop:hop + W])
    pending = not ev.query()
    got = pipe.finish(ticket)
    assert pending, "VadBatch.launch waited for work queued before it"
    assert np.array_equal(got, want)


def test_vad_engine_refuses_what_it_cannot_do(gpu, states):
    seg = M.HipSegmentation(states[False], max_batch=4)
    with pytest.raises(ValueError):
        VadBatch(seg, 4, step=0.5, latency=0.25, device=gpu)
    with pytest.raises(ValueError):
        VadBatch(seg, 4, step=0.5, latency=6.0, device=gpu)
    with pytest.raises(ValueError):
        VadBatch(seg, 4, device=gpu, serial=True)
    big = VadBatch(M.HipSegmentation(states[False], max_batch=64), 64, device=gpu, warmup=0)
    assert big.throughput and big.depth == 6 and big.max_inflight == 8
    small = VadBatch(M.HipSegmentation(states[False], max_batch=64, precision="f32"), 64, device=gpu, warmup=0)
    assert not small.throughput and small.depth == 2 and small.max_inflight == 3


def test_throughput_form_of_64_streams_against_the_blocks_path(gpu, states):
    """64 streams on the throughput engine (matrix-core recurrence, six lanes, steps in flight): the detection error
    rate of each stream's stitched output against its own VoiceActivityDetection is at most 0.5 %."""
    from diart_amd.inference import PredictionAccumulator
    from diart_amd.metrics import DetectionErrorRate
    n, steps, hop = 64, 14, 8000
    audio = synth_streams(n, (W + (steps - 1) * hop) / SR, seed0=700)
    dev = torch.from_numpy(audio).to(gpu)
    pipe = vad_engine(states, False, "f16x3", n, gpu)
    assert pipe.throughput and pipe.recurrence not in (None, "valu")
    hyp = [None] * n
    inflight = []

    def take(ticket):
        pipe.finish(ticket)
        turns, nturns = ticket["tail"][4], ticket["tail"][5]
        for i in range(n):
            ann = BatchedOutputTail.annotation(turns[i], int(nturns[i]), uri=str(i), label="speech")
            hyp[i] = ann if hyp[i] is None else hyp[i].update(ann)
    for t in range(steps):
        inflight.append(pipe.launch(dev[:, t * hop:t * hop + W]))
        if len(inflight) >= pipe.max_inflight:
            take(inflight.pop(0))
    while inflight:
        take(inflight.pop(0))
    metric = DetectionErrorRate()
    total = 0.0
    for i in range(n):
        ref, acc = blocks_vad(states, False, "f16x3", 0.5, 0.5, gpu), PredictionAccumulator(str(i))
        for t in range(steps):
            for out in ref([chunk(audio[i], t, hop, 0.5)]):
                acc.on_next(out)
        want = acc.get_prediction()
        d = metric(want, hyp[i].support(0.05), detailed=True)
        total += d["total"]
    assert total > 30.0
    assert abs(metric) <= 0.005, abs(metric)


# ---------------------------------------------------------------------------------------------------- serving
@pytest.mark.parametrize("rate,rings", [(16000, True), (48000, True), (16000, False), (44100, False)])
def test_stream_server_vad_equals_dedicated_pipelines(gpu, states, rate, rings):
    """StreamServer(pipeline="vad"): streams join late and push irregular amounts; each stream's stitched output
    equals that of its own VoiceActivityDetection fed the same windows (through blocks.Resample at another rate),
    on device rings and in host-window mode."""
    from diart_amd.blocks import Resample
    from diart_amd.inference import PredictionAccumulator, rolling_windows
    from diart_amd.serve import StreamServer
    sys_path_resample()
    import resample_ref as R
    lengths = {"ann": 11.0, "ben": 8.5, "cy": 7.0}
    audio = {}
    for i, (k, v) in enumerate(lengths.items()):
        x = synth_streams(1, v, seed0=820 + i)[0]
        audio[k] = x if rate == SR else R.resample(x, SR, rate).astype(np.float32)
    srv = StreamServer(M.HipSegmentation(states[False], max_batch=4), None, max_streams=4, device=gpu,
                       input_sample_rate=rate, device_rings=rings, tau_active=TAU, pipeline="vad")
    assert isinstance(srv.batch, VadBatch) and (srv.rings is not None) == rings
    rng = np.random.default_rng(5)
    pos = {k: 0 for k in audio}
    join_at = {"ann": 0, "ben": 2, "cy": 5}
    tick, widths = 0, []
    while any(pos[k] < len(audio[k]) for k in audio):
        for k in audio:
            if tick == join_at[k]:
                srv.open(k)
            if tick >= join_at[k] and pos[k] < len(audio[k]):
                m = int(rng.integers(rate // 8, rate * 2))
                srv.push(k, audio[k][pos[k]:pos[k] + m])
                pos[k] += m
        out = srv.step()
        widths.append(len(out))
        assert all(lab == "speech" for ann in out.values() for lab in ann.labels())
        tick += 1
    srv.drain()
    assert max(widths) >= 2, "windows of different streams were never batched together"
    blk = Resample(rate, SR, gpu) if rate != SR else None
    spoken = 0
    for k in audio:
        got = srv.close(k)
        cfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel.from_state(states[False], max_batch=1),
                                           tau_active=TAU, device=gpu)
        pipe, acc = VoiceActivityDetection(cfg), PredictionAccumulator(k)
        hop = rate // 2
        usable = len(audio[k]) // hop * hop
        blocks = (audio[k][None, i:i + hop] for i in range(0, usable, hop))
        for w in rolling_windows(blocks, 5.0, 0.5, rate):
            for out in pipe([blk(w) if blk is not None else w]):
                acc.on_next(out)
        want = acc.get_prediction()
        assert want is not None and got.to_rttm() == want.to_rttm(), k
        spoken += len(got)
    assert spoken > 0


def sys_path_resample():
    import sys
    from pathlib import Path
    here = str(Path(__file__).resolve().parent)
    if here not in sys.path:
        sys.path.insert(0, here)


def test_websocket_round_trip_sends_speech_rttm(gpu, states):
    """WebSocketFrontEnd on a StreamServer(pipeline="vad") over a real socket: the RTTM lines the client gets back are
    those of the same server stepped directly, and they carry the label "speech"."""
    import time
    sys_path_resample()
    from test_ws import Client
    from diart_amd.serve import StreamServer
    from diart_amd.ws import WebSocketFrontEnd
    audio = synth_streams(1, 8.0, seed0=880)[0]

    def make():
        return StreamServer(M.HipSegmentation(states[False], max_batch=1), None, max_streams=1, device=gpu,
                            tau_active=TAU, pipeline="vad")

    direct, want = make(), []
    direct.open("vad")
    direct.push("vad", audio)
    while True:
        out = direct.step()
        if not out:
            break
        want += [l for l in out["vad"].to_rttm().splitlines() if l]
    assert want and all(l.split()[7] == "speech" for l in want)
    srv = make()
    fe = WebSocketFrontEnd(srv, port=0).start()
    try:
        c = Client(fe.port, "vad")
        for p in range(0, len(audio), 16000):
            c.send_audio(audio[p:p + 16000])
        deadline = time.time() + 30
        while time.time() < deadline and sum(s.emitted for s in list(srv._streams.values())) < 7:
            time.sleep(0.05)
        assert sum(s.emitted for s in srv._streams.values()) == 7      # 8 s = 7 windows of 5 s every 0.5 s
        time.sleep(0.3)
        got = []
        c.s.settimeout(0.5)
        try:
            while True:
                op, data = c.recv()
                assert op == 0x1
                got += [l for l in data.decode().splitlines() if l]
        except (TimeoutError, OSError):
            pass
        assert not fe.errors
        assert got == want
    finally:
        fe.stop()
