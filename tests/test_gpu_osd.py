"""OverlappedSpeechDetection on the GPU: the stand-alone overlap kernel on crafted rows, the track the two segmentation
heads write (``dz_seg_forward_track``), ``OverlapBatch``, ``StreamServer(pipeline="osd")`` and ``FileBatch(pipeline=
"osd")``.  The yardstick of the track is torch on the CPU, ``torch.sort(scores, -1, descending=True).values[..., 1:2]``
of scores copied to the host; per stream the engines must produce what that stream's own ``OverlappedSpeechDetection``
produces at batch 1."""
import gc

import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.blocks import OverlappedSpeechDetection, OverlappedSpeechDetectionConfig
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.features import SlidingWindow, SlidingWindowFeature
from diart_amd.functional import overlap_track
from diart_amd.pipeline import AudioRing, FileBatch, OverlapBatch, VadBatch
from diart_amd.synth import synth_segmentation_state, synth_stream, synth_streams

pytestmark = pytest.mark.gpu

W, SR = 80000, 16000
# tau_active per model (False: multilabel state, seed 31; True: powerset state, seed 77), chosen from the reference alone:
# the CPU restatement of the segmentation (oracle/models_ref.py, PyanNetRef with the same state; powerset_to_multilabel
# for the powerset model) was run on this file's audio, its scores reduced by the defining torch statement, and the share
# of frames whose overlap track lies above tau counted.  The synthetic multilabel model scores high (the track's median
# is 0.86 - 0.92): at pyannote's 0.5 the share is 0.86 - 0.91 and the reference has NO step without a turn on the engine,
# server and file audio, so the multilabel tests use 0.95.  The powerset scores are hard 0 / 1 decisions: 0.5.  The audio
# (seeds below) was picked, again with the reference alone, so that the steps without a turn are not a single one.
#
#   share of frames above tau; steps of the reference's own pipeline with / without a turn (latency = step)
#                                        multilabel, tau 0.95        powerset, tau 0.5
#     engine audio, step 0.5             0.411   26 / 4              0.606   28 / 2      (latency 5: 19 / 11, 28 / 2)
#     engine audio, step 0.25            0.393   27 / 3              0.597   27 / 3      (latency 5: 15 / 15, 25 / 5)
#     server audio                       0.394   15 / 11             0.560   24 / 2
#     server audio as mu-law at 8 kHz    0.363   17 / 9              (not run)
#     file audio                         0.379   22 / 8              0.601   26 / 4
TAU = {False: 0.95, True: 0.5}
ENGINE_SEEDS = (601, 610, 621)                                                       # one synth_stream per stream
SERVER_STREAMS = {False: {"ann": (825, 11.0), "ben": (828, 8.5), "cy": (830, 7.0)},  # name: (seed, seconds)
                  True: {"ann": (831, 11.0), "ben": (827, 8.5), "cy": (824, 7.0)}}
FILES = (("a", 47, 7.0), ("b", 52, 9.5), ("c", 43, 7.0), ("d", 42, 9.5))             # name, seed, seconds


def engine_audio(steps: int, hop: int) -> np.ndarray:
    return np.stack([synth_stream(s, (W + (steps - 1) * hop) / SR) for s in ENGINE_SEEDS])


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


def cpu_track(scores: torch.Tensor) -> torch.Tensor:
    """The definition, evaluated by torch on the CPU from scores copied to the host."""
    return torch.sort(scores.detach().cpu(), dim=-1, descending=True).values[..., 1:2]


def tracks(ann):
    return sorted((s.start, s.end, str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


# ---------------------------------------------------------------------------------------------------- the kernel
def crafted_rows(K: int, rows: int = 1000) -> torch.Tensor:
    """Random rows, then classes of special rows cycling through the row index: all-equal, exact ties of the two largest,
    +inf / -inf, one NaN, two NaNs (a NaN at every position in turn)."""
    g = torch.Generator().manual_seed(100 + K)
    x = torch.rand(rows, K, generator=g) * 2 - 0.5
    for r in range(rows):
        kind, a, b = r % 8, r % K, (r // 8 + 1 + r % K) % K
        if a == b:
            b = (a + 1) % K
        if kind == 1:
            x[r] = x[r, 0]
        elif kind == 2:
            x[r, b] = x[r, a] = x[r].max() + 0.25                # the two largest tie exactly
        elif kind == 3:
            x[r, a] = float("inf")
        elif kind == 4:
            x[r, a], x[r, b] = float("inf"), float("-inf")
        elif kind == 5:
            x[r, a] = float("nan")
        elif kind == 6:
            x[r, a] = x[r, b] = float("nan")
        elif kind == 7:
            x[r, a], x[r, b] = float("inf"), float("inf")
    return x


@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_overlap_kernel_on_crafted_rows_is_the_cpu_statement_bit_for_bit(gpu, K):
    """(1000, K): four workgroups of 256 rows, the last one ragged; packed rows go through the whole-wave loads, the
    strided view (rows 12 floats apart) through the per-row loads."""
    x = crafted_rows(K)
    want = cpu_track(x)
    assert torch.isnan(want).any() and torch.isinf(want).any() and (want == want).any()
    got = overlap_track(x.to(gpu))
    assert got.is_cuda and got.shape == (1000, 1) and same_bits(got, want)
    wide = torch.full((1000, 12), -7.0)
    wide[:, :K] = x
    view = wide.to(gpu)[:, :K]
    assert view.stride() == (12, 1)
    assert same_bits(overlap_track(view), want)
    one = overlap_track(x[5:6].to(gpu))                            # a single row
    assert same_bits(one, want[5:6])
    lead = overlap_track(x[:996].reshape(3, 332, K).to(gpu))       # leading axes are kept
    assert lead.shape == (3, 332, 1) and same_bits(lead.reshape(996, 1), want[:996])
    with pytest.raises(ValueError):
        overlap_track(torch.rand(4, 1, device=gpu))
    with pytest.raises(ValueError):
        overlap_track(torch.rand(4, 9, device=gpu))


# ---------------------------------------------------------------------------------------------------- the heads
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("powerset", [False, True])
def test_forward_overlap_is_the_cpu_statement_on_the_scores_bit_for_bit(gpu, states, precision, powerset):
    """Batches 1 and 3 (one chunk is 293 rows: three 128-row tiles of the fused head, the last one ragged), both heads
    (f16x3: mlp_head_kernel; f32: seg_head_kernel): the scores are dz_seg_forward's, the track is the CPU statement on
    them, and forward_vad on the same handle afterwards is still torch.max: the selector does not stick."""
    seg = M.HipSegmentation(states[powerset], max_batch=3, powerset=powerset, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(3, 5.0, seed0=500)).to(gpu)
    seen = set()
    for b in (1, 3):
        want = seg(x[:b])
        track, scores = seg.forward_overlap(x[:b], return_scores=True)
        assert track.shape == (b, want.shape[1], 1) and track.is_cuda
        assert same_bits(scores, want), (precision, powerset, b)
        assert same_bits(track, cpu_track(want)), (precision, powerset, b)
        assert not torch.isnan(track).any()
        if powerset:                           # hard decisions: 1 exactly where a two-speaker class wins
            assert set(torch.unique(track).tolist()) <= {0.0, 1.0}
            seen |= set(torch.unique(track).tolist())
        vad, scores = seg.forward_vad(x[:b], return_scores=True)
        assert same_bits(scores, want)
        assert same_bits(vad, torch.max(want, dim=-1, keepdim=True)[0]), (precision, powerset, b)
        assert not torch.equal(vad, track)
    assert torch.equal(seg.forward_overlap(x[:3]), track[:3])         # (without the scores: same track)
    assert not powerset or seen == {0.0, 1.0}


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("powerset", [False, True])
def test_forward_overlap_of_a_nan_window(gpu, states, precision, powerset):
    """A window with a NaN sample: its track row is NaN wherever its score row is (on the f16x3 path the whole window,
    like the reference; the exact-f32 path lets the NaN through its arithmetic, and the track follows the scores it
    writes), and the other rows are those of a batch without it."""
    seg = M.HipSegmentation(states[powerset], max_batch=4, powerset=powerset, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(4, 5.0, seed0=510)).to(gpu)
    clean = seg.forward_overlap(x)
    x[1, 12345] = float("nan")
    want = seg(x)
    track, scores = seg.forward_overlap(x, return_scores=True)
    assert same_bits(scores, want)
    assert same_bits(track, cpu_track(want))
    nan_rows = torch.isnan(want).all(dim=-1)              # (two NaN scores are enough: NaN is ordered above numbers)
    assert bool(torch.isnan(track[..., 0])[nan_rows].all())
    assert torch.equal(torch.isnan(track[..., 0]), torch.isnan(want).sum(dim=-1) >= 2)
    if precision == "f16x3":                              # the whole window's rows are NaN, like the reference's
        assert bool(nan_rows[1].all()) and bool(torch.isnan(track[1]).all())
    for i in (0, 2, 3):
        assert same_bits(track[i], clean[i]) and not torch.isnan(track[i]).any()


def _call_track(seg, x, batch, track):
    """dz_seg_forward_track through the library on the handle ``seg`` holds for these windows -> (rc, scores, track)."""
    from diart_amd import _lib
    lib = _lib.load()
    B, S = x.shape
    h = seg._need(S, B)
    F = seg.num_frames(S)
    rows = max(batch, B)
    scores = torch.full((rows, F, seg.num_speakers), -7.0, device=x.device)
    trk = torch.full((rows, F, 1), -7.0, device=x.device)
    rc = lib.dz_seg_forward_track(h, x.data_ptr(), x.stride(0) if B > 1 else S, batch, scores.data_ptr(), trk.data_ptr(),
                                  track, torch.cuda.current_stream(x.device).cuda_stream)
    return rc, scores, trk


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_track_speech_is_forward_vad_and_a_batch_above_the_handles_is_refused(gpu, states, precision):
    """DZ_TRACK_SPEECH through dz_seg_forward_track on a real handle: scores and track are dz_seg_forward_vad's bit for
    bit.  A batch above the handle's max_batch is refused by name and nothing is written."""
    from diart_amd import _lib
    seg = M.HipSegmentation(states[False], max_batch=3, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(3, 5.0, seed0=500)).to(gpu)
    want_track, want_scores = seg.forward_vad(x, return_scores=True)
    rc, scores, trk = _call_track(seg, x, 3, _lib.TRACK_SPEECH)
    assert rc == 0, _lib.load().dz_last_error()
    assert same_bits(scores, want_scores) and same_bits(trk, want_track)
    rc, scores, trk = _call_track(seg, x, 4, _lib.TRACK_OVERLAP)
    assert rc != 0
    assert _lib.load().dz_last_error().decode() == "dz_seg_forward_track: batch 4 outside [1, 3]"
    torch.cuda.synchronize(gpu)
    assert bool((scores == -7.0).all()) and bool((trk == -7.0).all())


def test_a_one_speaker_model_is_refused_by_name_on_every_layer(gpu):
    """K < 2 has no overlap: the C entry point refuses the handle (and still gives it its speech track), and
    forward_overlap, OverlapBatch and OverlappedSpeechDetection refuse the model at the call / at construction."""
    from diart_amd import _lib
    state = synth_segmentation_state(seed=31, num_speakers=1)
    seg = M.HipSegmentation(state, max_batch=2).to(gpu)
    assert seg.num_speakers == 1
    x = torch.from_numpy(synth_streams(2, 5.0, seed0=500)).to(gpu)
    rc, scores, trk = _call_track(seg, x, 2, _lib.TRACK_OVERLAP)
    assert rc != 0
    assert _lib.load().dz_last_error().decode() == \
        "dz_seg_forward_track: the overlap track needs 2 <= speakers <= 8 (got 1)"
    torch.cuda.synchronize(gpu)
    assert bool((scores == -7.0).all()) and bool((trk == -7.0).all())
    rc, scores, trk = _call_track(seg, x, 2, _lib.TRACK_SPEECH)
    assert rc == 0 and same_bits(trk, seg(x))                  # one speaker: the speech track is the scores
    with pytest.raises(ValueError, match="forward_overlap.*1 speaker"):
        seg.forward_overlap(x)
    with pytest.raises(ValueError, match="forward_overlap.*1 speaker"):
        M.HipSegmentation(state, max_batch=2).forward_overlap(x)          # a model not yet on the device
    with pytest.raises(ValueError, match="OverlapBatch.*1 speaker"):
        OverlapBatch(M.HipSegmentation(state, max_batch=2), 2, device=gpu)
    with pytest.raises(ValueError, match="OverlappedSpeechDetection.*1 speaker"):
        OverlappedSpeechDetection(OverlappedSpeechDetectionConfig(
            segmentation=M.SegmentationModel.from_state(state, max_batch=1), device=gpu))
    with pytest.raises(ValueError, match="float32"):
        overlap_track(torch.rand(4, 3, device=gpu).double())
    with pytest.raises(ValueError, match="empty"):
        overlap_track(torch.rand(0, 3, device=gpu))
    with pytest.raises(ValueError, match="empty"):
        overlap_track(torch.rand(0, 3))


# ---------------------------------------------------------------------------------------------------- the engine
def blocks_osd(states, powerset, precision, step, latency, gpu):
    cfg = OverlappedSpeechDetectionConfig(
        segmentation=M.SegmentationModel.from_state(states[powerset], max_batch=1, powerset=powerset,
                                                    precision=precision),
        step=step, latency=latency, tau_active=TAU[powerset], device=gpu)
    return OverlappedSpeechDetection(cfg)


def chunk(x, t, hop, step):
    return SlidingWindowFeature(x[t * hop:t * hop + W, None], SlidingWindow(start=t * step, duration=1 / SR,
                                                                            step=1 / SR))


def osd_engine(states, powerset, precision, n, gpu, step=0.5, latency=None, **kw):
    return OverlapBatch(M.HipSegmentation(states[powerset], max_batch=n, powerset=powerset, precision=precision), n,
                        tau_active=TAU[powerset], step=step, latency=latency, device=gpu, **kw)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("powerset", [False, True])
@pytest.mark.parametrize("step", [0.5, 0.25])
@pytest.mark.parametrize("latency", ["step", "duration"])
def test_engine_equals_per_stream_pipelines(gpu, states, precision, powerset, step, latency):
    """3 streams x 10 steps on 2 lanes: every step's overlap turns (OverlapBatch.detect) equal those of the stream's own
    OverlappedSpeechDetection at batch 1; the step 0.25 engine reads its windows from a device ring (hop 4000)."""
    n, steps, hop = 3, 10, int(step * SR)
    lat = step if latency == "step" else 5.0
    audio = engine_audio(steps, hop)
    pipe = osd_engine(states, powerset, precision, n, gpu, step, lat, lanes=2)
    assert isinstance(pipe, VadBatch) and pipe.depth == 2 and not pipe.throughput
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
    with_turns, without = 0, 0
    for i in range(n):
        ref = blocks_osd(states, powerset, precision, step, lat, gpu)
        for t in range(steps):
            (want, _), = ref([chunk(audio[i], t, hop, step)])
            assert tracks(got[t][i]) == tracks(want), (i, t)
            assert all(lab == "overlap" for lab in got[t][i].labels())
            with_turns += len(tracks(want)) > 0
            without += len(tracks(want)) == 0
    assert with_turns > 0, "no overlap turn anywhere: the comparison shows nothing"
    assert without > 0, "every step of every stream has an overlap turn: a track stuck high would pass"


def test_partial_steps_and_resets_leave_other_streams_alone(gpu, states):
    """A step over a subset of slots, and reset(slot), change nothing for the other streams; a reset stream restarts
    like a fresh engine (window start times from 0)."""
    n, steps, hop = 3, 10, 8000
    audio = engine_audio(steps, hop)
    dev = torch.from_numpy(audio).to(gpu)
    full, part, fresh = (osd_engine(states, False, "f16x3", n, gpu) for _ in range(3))
    restart, some = 5, 0
    for t in range(steps):
        x = dev[:, t * hop:t * hop + W]
        want = full.detect(x)
        if t == 4:                      # stream 1 has no window this step, then starts over
            ticket = part.launch(x[[0, 2]].contiguous(), slots=[0, 2])
            part.finish(ticket)
            turns, nturns = ticket["tail"][4], ticket["tail"][5]
            got = {0: BatchedOutputTail.annotation(turns[0], int(nturns[0]), label="overlap"),
                   2: BatchedOutputTail.annotation(turns[1], int(nturns[1]), label="overlap")}
            part.reset(1)
        else:
            got = dict(enumerate(part.detect(x)))
        for i in (0, 2):
            assert tracks(got[i]) == tracks(want[i]), (t, i)
            some += len(tracks(want[i]))
        if t >= restart:                # stream 1 after its reset: a fresh engine fed from window `restart` on
            again = fresh.detect(torch.stack([dev[1, t * hop:t * hop + W]] * n))
            assert tracks(got[1]) == tracks(again[1]), t
    assert some > 0


def test_engine_refuses_what_it_cannot_do(gpu, states):
    seg = M.HipSegmentation(states[False], max_batch=4)
    with pytest.raises(ValueError):
        OverlapBatch(seg, 4, step=0.5, latency=0.25, device=gpu)
    with pytest.raises(ValueError):
        OverlapBatch(seg, 4, device=gpu, serial=True)
    big = OverlapBatch(M.HipSegmentation(states[False], max_batch=64), 64, device=gpu, warmup=0)
    assert big.throughput and big.depth == 6 and big.max_inflight == 8          # VadBatch's engine choices
    assert big.tau_active == 0.5


# ---------------------------------------------------------------------------------------------------- serving
def sys_path_tests():
    import sys
    from pathlib import Path
    here = str(Path(__file__).resolve().parent)
    if here not in sys.path:
        sys.path.insert(0, here)


@pytest.mark.parametrize("rate,fmt,rings,powerset", [(16000, "f32", True, False), (16000, "f32", False, False),
                                                     (8000, "ulaw", True, False), (16000, "f32", True, True),
                                                     (16000, "f32", False, True)])
def test_stream_server_osd_equals_dedicated_pipelines(gpu, states, rate, fmt, rings, powerset):
    """StreamServer(pipeline="osd"): streams join late and push irregular amounts; each stream's stitched output equals
    that of its own OverlappedSpeechDetection fed the same windows (decoded, and through blocks.Resample at 8 kHz), on
    device rings and in host-window mode, once as G.711 mu-law at 8 kHz."""
    from diart_amd.blocks import Resample
    from diart_amd.inference import PredictionAccumulator, rolling_windows
    from diart_amd.pcm import pcm_to_mono
    from diart_amd.serve import StreamServer
    sys_path_tests()
    import resample_ref as R
    raw, audio = {}, {}
    for k, (seed, seconds) in SERVER_STREAMS[powerset].items():
        x = synth_streams(1, seconds, seed0=seed)[0]
        x = x if rate == SR else R.resample(x, SR, rate).astype(np.float32)
        if fmt == "ulaw":
            from test_gpu_ingest_formats import encode_nearest, ulaw_linear
            raw[k] = encode_nearest(x, ulaw_linear(np.arange(256)))
            audio[k] = pcm_to_mono(raw[k], "ulaw", 1)
        else:
            raw[k] = audio[k] = x
    srv = StreamServer(M.HipSegmentation(states[powerset], max_batch=4, powerset=powerset), None, max_streams=4,
                       device=gpu, input_sample_rate=rate, input_format=fmt, device_rings=rings,
                       tau_active=TAU[powerset], pipeline="osd")
    assert isinstance(srv.batch, OverlapBatch) and (srv.rings is not None) == rings
    rng = np.random.default_rng(5)
    pos = {k: 0 for k in raw}
    join_at = {"ann": 0, "ben": 2, "cy": 5}
    tick, widths, with_turns, without = 0, [], 0, 0

    def count(out):
        nonlocal with_turns, without
        assert all(lab == "overlap" for ann in out.values() for lab in ann.labels())
        with_turns += sum(len(ann) > 0 for ann in out.values())
        without += sum(len(ann) == 0 for ann in out.values())
    while any(pos[k] < len(raw[k]) for k in raw):
        for k in raw:
            if tick == join_at[k]:
                srv.open(k)
            if tick >= join_at[k] and pos[k] < len(raw[k]):
                m = int(rng.integers(rate // 8, rate * 2))
                srv.push(k, raw[k][pos[k]:pos[k] + m])
                pos[k] += m
        out = srv.step()
        widths.append(len(out))
        count(out)
        tick += 1
    while True:
        out = srv.step()
        if not out:
            break
        count(out)
    assert not srv.step_errors
    assert max(widths) >= 2, "windows of different streams were never batched together"
    blk = Resample(rate, SR, gpu) if rate != SR else None
    for k in audio:
        got = srv.close(k)
        cfg = OverlappedSpeechDetectionConfig(
            segmentation=M.SegmentationModel.from_state(states[powerset], max_batch=1, powerset=powerset),
            tau_active=TAU[powerset], device=gpu)
        pipe, acc = OverlappedSpeechDetection(cfg), PredictionAccumulator(k)
        hop = rate // 2
        usable = len(audio[k]) // hop * hop
        blocks = (audio[k][None, i:i + hop] for i in range(0, usable, hop))
        for w in rolling_windows(blocks, 5.0, 0.5, rate):
            for out in pipe([blk(w) if blk is not None else w]):
                acc.on_next(out)
        want = acc.get_prediction()
        assert want is not None and got.to_rttm() == want.to_rttm(), k
    assert with_turns > 0, "no overlap turn anywhere: the comparison shows nothing"
    assert without > 0, "every step of every stream has an overlap turn: a track stuck high would pass"


def test_websocket_round_trip_sends_overlap_rttm(gpu, states):
    """WebSocketFrontEnd on a StreamServer(pipeline="osd") over a real socket: the RTTM lines the client gets back are
    those of the same server stepped directly, and they carry the label "overlap"."""
    import time
    sys_path_tests()
    from test_ws import Client
    from diart_amd.serve import StreamServer
    from diart_amd.ws import WebSocketFrontEnd
    audio = synth_streams(1, 8.0, seed0=880)[0]

    def make():
        return StreamServer(M.HipSegmentation(states[False], max_batch=1), None, max_streams=1, device=gpu,
                            tau_active=TAU[False], pipeline="osd")

    direct, want = make(), []
    direct.open("osd")
    direct.push("osd", audio)
    while True:
        out = direct.step()
        if not out:
            break
        want += [l for l in out["osd"].to_rttm().splitlines() if l]
    assert want and all(l.split()[7] == "overlap" for l in want)
    srv = make()
    fe = WebSocketFrontEnd(srv, port=0).start()
    try:
        c = Client(fe.port, "osd")
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


# ---------------------------------------------------------------------------------------------------- files
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from diart_amd.inference import write_wav
    root = tmp_path_factory.mktemp("osd_files")
    speech = root / "wav"
    speech.mkdir()
    for name, seed, dur in FILES:
        write_wav(speech / f"{name}.wav", synth_stream(seed, dur), SR)
    return root, speech


def _benchmark(speech, out, cfg, k):
    from diart_amd.inference import Benchmark
    b = Benchmark(speech, None, out, show_report=False, batch_size=32, concurrent_files=k)
    b(OverlappedSpeechDetection, cfg)
    path = b.last_path
    del b
    gc.collect()
    return path, {p.name: p.read_text() for p in sorted(out.iterdir())}


def _uncovered(rttm_text: str, duration: float, step: float) -> bool:
    """Is there a stretch of at least one step inside [0, duration] that no turn of the file covers?  (A file's steps
    are not visible behind ``Benchmark``; a step without a turn shows as such a stretch.)"""
    spans = sorted((float(l.split()[3]), float(l.split()[3]) + float(l.split()[4]))
                   for l in rttm_text.splitlines() if l.strip())
    t = 0.0
    for s, e in spans:
        if s - t >= step:
            return True
        t = max(t, e)
    return duration - t >= step


@pytest.mark.parametrize("powerset", [False, True])
def test_files_batched_together_give_the_rttm_files_of_the_loop(gpu, states, corpus, powerset):
    """Benchmark(OverlappedSpeechDetection) on both paths: concurrent_files=0 runs the one-file-at-a-time loop, 4 takes
    the file batch (FileBatch(pipeline="osd") on an OverlapBatch), and the RTTM files are the same byte for byte."""
    root, speech = corpus
    cfg = OverlappedSpeechDetectionConfig(
        segmentation=M.SegmentationModel.from_state(states[powerset], max_batch=32, powerset=powerset),
        tau_active=TAU[powerset], device=gpu)
    path, want = _benchmark(speech, root / f"loop-{powerset}", cfg, 0)
    assert path == "one_file_at_a_time" and sorted(want) == [f"{n}.rttm" for n, *_ in FILES]
    path, got = _benchmark(speech, root / f"batch-{powerset}", cfg, 4)
    assert path == "file_batch"
    assert got == want, "RTTM files differ from the one-file-at-a-time loop"
    labels = {l.split()[7] for t in got.values() for l in t.splitlines() if l.strip()}
    assert labels == {"overlap"}, "no overlap turn in any file: the comparison shows nothing"
    assert any(_uncovered(want[f"{n}.rttm"], dur, cfg.step) for n, _, dur in FILES), \
        "overlap turns cover every file end to end: a track stuck high would pass"
    # Benchmark hides a file's steps: the pipeline driven directly over each file's windows shows them
    from diart_amd.inference import rolling_windows
    with_turns, without = 0, 0
    hop = int(cfg.step * SR)
    for _, seed, dur in FILES:
        x = synth_stream(seed, dur)
        pipe = OverlappedSpeechDetection(cfg)
        for w in rolling_windows((x[None, i:i + hop] for i in range(0, len(x) // hop * hop, hop)), 5.0, cfg.step, SR):
            (ann, _), = pipe([w])
            assert all(lab == "overlap" for lab in ann.labels())
            with_turns += len(ann) > 0
            without += len(ann) == 0
    assert with_turns > 0, "no step of any file has an overlap turn"
    assert without > 0, "every step of every file has an overlap turn: a track stuck high would pass"


def test_file_batch_form(gpu, states):
    fb = FileBatch(M.HipSegmentation(states[False], max_batch=8), None, pipeline="osd", rows=8, max_files=4,
                   tau_active=TAU[False], device=gpu)
    assert fb.kind == "osd" and isinstance(fb.engine, OverlapBatch) and fb.G == 1 and fb.gather
    x = synth_stream(FILES[0][1], FILES[0][2])
    got = fb.run([("a", x, 0.0), ("b", x, 0.0)])
    assert sorted(got) == ["a", "b"] and got["a"].to_rttm().replace(" a ", " b ") == got["b"].to_rttm()
    assert set(got["a"].labels()) == {"overlap"}
