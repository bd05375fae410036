"""The WeSpeaker ResNet34 embedding on the N-stream engine: the two halves of its forward (``dz_wsp_trunk`` /
``dz_wsp_pool``), ``WeSpeakerBatch`` and ``StreamServer`` with a ``HipWeSpeakerEmbedding``.  Per stream the engine must
produce what that stream's own ``SpeakerDiarization`` produces at batch 1.  Every comparison is an equality (bits,
assignments, RTTM text): a row of the WeSpeaker forward and of the segmentation does not depend on the batch it is in."""
import gc
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import _lib
from diart_amd import models as M
from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.blocks.clustering import OnlineSpeakerClustering
from diart_amd.features import SlidingWindow, SlidingWindowFeature
from diart_amd.pipeline import AudioRing, WeSpeakerBatch
from diart_amd.synth import synth_segmentation_state, synth_streams, synth_wespeaker_state

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16x3", "f32")
W, HOP, SR = 80000, 8000, 16000
TAU = 0.5
MB = 1 << 20


@pytest.fixture(scope="module")
def states():
    return {False: synth_segmentation_state(seed=31), True: synth_segmentation_state(seed=77, powerset=True),
            "emb": synth_wespeaker_state()}


def same_bits(a, b) -> bool:
    """Bit-for-bit equal, every NaN counted equal to a NaN."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a).view(np.int32)[~na],
                                                          np.ascontiguousarray(b).view(np.int32)[~nb]))


def tracks(ann):
    return sorted((s.start, s.end, str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


def chunk(x, t):
    return SlidingWindowFeature(x[t * HOP:t * HOP + W, None], SlidingWindow(start=t * 0.5, duration=1 / SR, step=1 / SR))


def engine(states, n, precision, gpu, powerset=False, norm_w=False, **kw):
    return WeSpeakerBatch(M.HipSegmentation(states[powerset], max_batch=n, powerset=powerset, precision=precision),
                          M.HipWeSpeakerEmbedding(states["emb"], max_batch=n, precision=precision), n, tau_active=TAU,
                          normalize_embedding_weights=norm_w, device=gpu, **kw)


def own_pipeline(states, precision, gpu, powerset=False, norm_w=False, seg_model=None, emb_model=None):
    """One stream's own pipeline: the blocks API at batch 1 with the same models."""
    cfg = SpeakerDiarizationConfig(
        segmentation=seg_model or M.SegmentationModel.from_state(states[powerset], max_batch=1, powerset=powerset,
                                                                 precision=precision),
        embedding=emb_model or M.EmbeddingModel.from_state(states["emb"], max_batch=1, precision=precision),
        latency=0.5, tau_active=TAU, normalize_embedding_weights=norm_w, device=gpu)
    return SpeakerDiarization(cfg)


class OwnStream:
    """A stream's own SpeakerDiarization stepped one chunk at a time, with a second clustering state fed the same
    segmentation / embeddings, which tells the assignments (the pipeline keeps them to itself)."""

    def __init__(self, pipe):
        self.pipe = pipe
        self.clu = OnlineSpeakerClustering(TAU, 0.3, 1.0, "cosine", 20)
        self.total = None

    def step(self, c):
        batch = torch.from_numpy(c.data)[None]
        seg = self.pipe.segmentation(batch)
        emb = self.pipe.embedding(batch, seg)
        ann = self.pipe.finalise([c], seg, emb)[0][0]
        assign = self.clu.identify(SlidingWindowFeature(seg[0].numpy(), c.sliding_window), emb[0]).assignment
        self.total = ann if self.total is None else self.total.update(ann)
        return ann, np.asarray(assign)


def rttm(ann, uri="s"):
    if ann is None:
        return ""
    ann.uri = uri
    return ann.support(0.05).to_rttm()


# ------------------------------------------------------------------------------------------------ the two halves
@pytest.mark.parametrize("precision", PRECISIONS)
def test_halves_equal_the_whole_bit_for_bit(gpu, states, precision):
    """dz_wsp_trunk + dz_wsp_pool == dz_wsp_forward_multi bit for bit (NaN == NaN) at batches 1, 3 and 64, K = 1 and
    3, with and without the L2 normalisation, with both halves on one HIP stream and on two joined by an event; a pool
    whose batch is not the last trunk's is an error that launches nothing; dz_wsp_peek works after either half."""
    hip = M.HipWeSpeakerEmbedding(states["emb"], max_batch=64, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(64, 5.0, seed0=300)).to(gpu)
    x[2, 4321] = float("nan")                       # a flagged row: the handle carries the flag between the halves
    g = torch.Generator().manual_seed(9)
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    checked = 0
    for b in (1, 3, 64):
        for K in (1, 3):
            w = torch.rand(b, K, 293, generator=g).to(gpu)
            for normalize in (False, True):
                want = hip.forward_multi(x[:b, None], w, normalize=normalize)
                handle = hip._need(W, b)
                stride = x.stride(0) if b > 1 else W
                # one stream
                out = torch.full((b, K, 256), 7.0, device=gpu)
                cur = torch.cuda.current_stream(gpu).cuda_stream
                hip.trunk_launch(handle, x.data_ptr(), stride, b, cur)
                hip.pool_launch(handle, w.data_ptr(), b, K, 293, normalize, out.data_ptr(), cur)
                assert same_bits(out, want), (precision, b, K, normalize, "one stream")
                # two streams joined by an event
                out2 = torch.full((b, K, 256), 7.0, device=gpu)
                ev = torch.cuda.Event()
                s1.wait_stream(torch.cuda.current_stream(gpu))
                hip.trunk_launch(handle, x.data_ptr(), stride, b, s1.cuda_stream)
                ev.record(s1)
                s2.wait_event(ev)
                hip.pool_launch(handle, w.data_ptr(), b, K, 293, normalize, out2.data_ptr(), s2.cuda_stream)
                torch.cuda.current_stream(gpu).wait_stream(s2)
                assert same_bits(out2, want), (precision, b, K, normalize, "two streams")
                if b >= 3:
                    assert bool(torch.isnan(want[2]).all()) and not bool(torch.isnan(want[:2]).any())
                checked += 1
    assert checked == 12
    # the wrong batch: refused, nothing launched (the output keeps its fill), and the right pool still works
    b, K = 3, 3
    w = torch.rand(b, K, 293, generator=g).to(gpu)
    want = hip.forward_multi(x[:b, None], w, normalize=True)
    layer4 = hip.peek(W, 5)[0].clone()
    handle = hip._need(W, b)
    cur = torch.cuda.current_stream(gpu).cuda_stream
    hip.trunk_launch(handle, x.data_ptr(), x.stride(0), b, cur)
    assert same_bits(hip.peek_handle(handle, 5)[0], layer4)          # peek after the first half
    out = torch.full((b + 1, K, 256), 7.0, device=gpu)
    for wrong in (b + 1, b - 1, 0):
        with pytest.raises(_lib.DiartAmdError, match="dz_wsp_pool"):
            hip.pool_launch(handle, w.data_ptr(), wrong, K, 293, True, out.data_ptr(), cur)
    torch.cuda.synchronize(gpu)
    assert bool((out == 7.0).all())
    hip.pool_launch(handle, w.data_ptr(), b, K, 293, True, out.data_ptr(), cur)
    assert same_bits(out[:b], want)
    assert hip.peek_handle(handle, 6)[0].numel() == b * K * 5120      # peek after the second half


# ------------------------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("powerset", [False, True], ids=["multilabel", "powerset"])
@pytest.mark.parametrize("norm_w", [False, True], ids=["raw-weights", "normalized-weights"])
def test_engine_equals_per_stream_pipelines(gpu, states, precision, powerset, norm_w):
    """5 streams x 20 steps on 2 lanes.  Every step: the engine's embeddings equal forward_multi on the same windows
    and the engine's own weights bit for bit; per stream, the speaker assignments and the step's speech turns equal
    those of the stream's own SpeakerDiarization at batch 1; at the end each stream's RTTM, taken through diarize() on
    a second engine, equals the RTTM of its own pipeline."""
    n, steps = 5, 20
    audio = synth_streams(n, (W + HOP * (steps - 1)) / SR, seed0=1300 + int(powerset))
    dev = torch.from_numpy(audio).to(gpu)
    pipe = engine(states, n, precision, gpu, powerset, norm_w, tail=True)
    dia = engine(states, n, precision, gpu, powerset, norm_w, tail=True)
    assert pipe.depth == 2 and pipe.max_inflight == 3 and not pipe.throughput and pipe.num_hip_streams == 4
    hip = M.HipWeSpeakerEmbedding(states["emb"], max_batch=n, precision=precision).to(gpu)
    own = [OwnStream(own_pipeline(states, precision, gpu, powerset, norm_w)) for _ in range(n)]
    said = [None] * n
    assigned = turns_seen = 0
    for t in range(steps):
        x = dev[:, t * HOP:t * HOP + W]
        ticket = pipe.launch(x)
        seg, emb, _, assign = pipe.finish(ticket, want_scores=False)
        emb, assign = emb.copy(), np.asarray(assign).copy()
        _, _, _, _, turns, nturns = ticket["tail"]
        want_emb = hip.forward_multi(x[:, None], ticket["w"][:n], normalize=True)
        assert same_bits(emb, want_emb), (precision, powerset, norm_w, t)
        anns = dia.diarize(x)
        for i in range(n):
            want, want_assign = own[i].step(chunk(audio[i], t))
            assert np.array_equal(assign[i], want_assign), (precision, powerset, norm_w, t, i, assign[i], want_assign)
            got = BatchedOutputTail.annotation(turns[i], int(nturns[i]))
            assert tracks(got) == tracks(want), (precision, powerset, norm_w, t, i)
            assert tracks(anns[i]) == tracks(want), (precision, powerset, norm_w, t, i, "diarize")
            said[i] = anns[i] if said[i] is None else said[i].update(anns[i])
            assigned += int((want_assign >= 0).sum())
            turns_seen += len(tracks(want))
    for i in range(n):
        assert rttm(said[i]) == rttm(own[i].total), (precision, powerset, norm_w, i)
    assert assigned > 0 and turns_seen > 0, "no speaker anywhere: the comparison shows nothing"


def test_64_streams_on_the_throughput_recurrence_and_both_lanes(gpu, states):
    """64 streams x 8 steps, steps kept in flight on both lanes, the matrix-core recurrence StreamBatch would pick:
    each stream's assignments at every step and its RTTM equal those of its own SpeakerDiarization at batch 1.

    The streams' own pipelines run the recurrence kernel the engine runs (``HipSegmentation(recurrence=)``): the
    matrix-core and the one-chain-per-CU recurrence agree to ~1e-6, not to the bit, and a score within that of
    tau_active would move a turn boundary; with the same kernel a row does not depend on its batch and the
    comparison is an equality.  The 64 pipelines share one pair of model objects (the models hold no stream state)."""
    n, steps = 64, 8
    audio = synth_streams(n, (W + HOP * (steps - 1)) / SR, seed0=1400)
    dev = torch.from_numpy(audio).to(gpu)
    pipe = engine(states, n, "f16x3", gpu, tail=True)
    assert pipe.throughput and pipe.recurrence not in (None, "valu")
    assert pipe.depth == 2 and pipe.max_inflight == 3 and pipe.num_hip_streams == 4
    got_assign = np.empty((steps, n, 3), dtype=np.int64)
    said = [None] * n
    inflight = []

    def take(t, ticket):
        _, _, _, assign = pipe.finish(ticket, want_scores=False)
        got_assign[t] = np.asarray(assign)
        _, _, _, _, turns, nturns = ticket["tail"]
        for i in range(n):
            ann = BatchedOutputTail.annotation(turns[i], int(nturns[i]))
            said[i] = ann if said[i] is None else said[i].update(ann)

    for t in range(steps):
        inflight.append((t, pipe.launch(dev[:, t * HOP:t * HOP + W])))
        if len(inflight) >= pipe.max_inflight:
            take(*inflight.pop(0))
    while inflight:
        take(*inflight.pop(0))
    rec = pipe.recurrence
    seg_model = M.SegmentationModel(lambda: M.HipSegmentation(states[False], max_batch=1, precision="f16x3",
                                                              recurrence=rec))
    emb_model = M.EmbeddingModel.from_state(states["emb"], max_batch=1, precision="f16x3")
    bad_assign, bad_rttm, assigned = [], [], 0
    for i in range(n):
        own = OwnStream(own_pipeline(states, "f16x3", gpu, seg_model=seg_model, emb_model=emb_model))
        for t in range(steps):
            _, want_assign = own.step(chunk(audio[i], t))
            assigned += int((want_assign >= 0).sum())
            if not np.array_equal(got_assign[t, i], want_assign):
                bad_assign.append((i, t, got_assign[t, i].tolist(), want_assign.tolist()))
        if rttm(said[i]) != rttm(own.total):
            bad_rttm.append(i)
    print(f"64 streams, recurrence {rec}: {len(bad_assign)} assignment rows and {len(bad_rttm)} RTTMs differ; "
          f"{assigned} speakers assigned")
    assert assigned > 0
    assert not bad_assign, bad_assign[:5]
    assert not bad_rttm, bad_rttm


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_nan_window_gets_no_speaker_and_leaves_its_neighbours_alone(gpu, states, precision):
    n, steps, poisoned = 4, 4, 2
    audio = torch.from_numpy(synth_streams(n, (W + HOP * (steps - 1)) / SR, seed0=1500)).to(gpu)
    clean, dirty = engine(states, n, precision, gpu), engine(states, n, precision, gpu)
    for t in range(steps):
        x = audio[:, t * HOP:t * HOP + W]
        want_seg, want_emb, want_scores, want_assign = [np.array(v) for v in clean(x)]
        y = x.clone()
        if t == poisoned:
            y[1, 12345] = float("nan")
        seg, emb, scores, assign = dirty(y)
        for i in range(n):
            if i == 1 and t == poisoned:
                continue
            assert same_bits(seg[i], want_seg[i]) and same_bits(emb[i], want_emb[i]), (precision, t, i)
            if i != 1 or t < poisoned:      # (afterwards stream 1 is a stream that skipped a window: its own history)
                assert np.array_equal(scores[i], want_scores[i]) and np.array_equal(assign[i], want_assign[i]), (t, i)
        if t == poisoned:
            assert bool(np.isnan(emb[1]).all()), "the embeddings of a NaN window are NaN rows"
            assert bool((np.asarray(assign[1]) < 0).all()), assign[1]
        if t == poisoned - 1:
            assert bool((np.asarray(assign) >= 0).any()), "nobody speaks: the comparison shows nothing"


def test_partial_steps_resets_and_ring_input(gpu, states):
    """``slots=`` steps (some streams only) and ``reset(slot)`` give every stream what a full-step engine computes for it
    from that point on (embeddings bitwise, scores, assignments); windows read in place from an ``AudioRing`` give
    what the same windows give as a tensor."""
    n, steps = 4, 8
    audio = synth_streams(n, (W + HOP * steps) / SR, seed0=1600)
    dev = torch.from_numpy(audio).to(gpu)
    full, ringed = engine(states, n, "f16x3", gpu), engine(states, n, "f16x3", gpu)
    ring = AudioRing(n, W, HOP, device=gpu)
    for j in range(W // HOP - 1):
        ring.push(dev[:, j * HOP:(j + 1) * HOP].contiguous())
    want = [[None] * steps for _ in range(n)]
    for t in range(steps):
        seg, emb, scores, assign = full(dev[:, t * HOP:t * HOP + W])
        assert ring.push(dev[:, W + (t - 1) * HOP:W + t * HOP].contiguous())
        rseg, remb, rscores, rassign = ringed(ring)
        assert same_bits(rseg, seg) and same_bits(remb, emb), t
        assert np.array_equal(rscores, scores) and np.array_equal(rassign, assign), t
        for i in range(n):
            want[i][t] = (emb[i].copy(), scores[i].copy(), np.asarray(assign[i]).copy())
    part = engine(states, n, "f16x3", gpu)
    pos = [0] * n
    pattern = [[0, 1, 2, 3], [0, 2], [1, 3], [3], [0, 1, 2], "reset2", [2, 3], [0, 1, 2, 3], [2], [1, 2], [0, 2, 3]]
    checked = 0
    for sel in pattern:
        if sel == "reset2":
            part.reset(2)
            pos[2] = 0
            continue
        sel = [i for i in sel if pos[i] < steps]
        rows = torch.stack([dev[i, pos[i] * HOP:pos[i] * HOP + W] for i in sel])
        _, emb, scores, assign = part.finish(part.launch(rows, slots=sel))
        for j, i in enumerate(sel):
            we, ws, wa = want[i][pos[i]]
            assert same_bits(emb[j], we), (sel, i)
            assert np.array_equal(scores[j], ws) and np.array_equal(np.asarray(assign[j]), wa), (sel, i)
            pos[i] += 1
            checked += 1
    assert checked >= 20


def test_launch_does_not_wait_for_the_gpu(gpu, states):
    """After its warm-up, WeSpeakerBatch.launch returns while work queued before it is pending, and the step's
    results equal those of an engine that never waited."""
    n = 4
    audio = torch.from_numpy(synth_streams(n, (W + 2 * HOP) / SR, seed0=995)).to(gpu)
    pipe, ref = engine(states, n, "f16x3", gpu), engine(states, n, "f16x3", gpu)
    for p in (pipe, ref):
        p.finish(p.launch(audio[:, :W]))
    want = [x.copy() for x in ref.finish(ref.launch(audio[:, HOP:HOP + W]))[:2]]
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
    ticket = pipe.launch(audio[:, HOP:HOP + W])
    pending = not ev.query()
    seg, emb, _, _ = pipe.finish(ticket)
    assert pending, "WeSpeakerBatch.launch waited for work queued before it"
    assert same_bits(seg, want[0]) and same_bits(emb, want[1])


def test_engine_choices(gpu, states):
    """lanes stay at 2 whatever the stream count; the recurrence is StreamBatch's choice; nothing is allocated for a
    window size before its first launch."""
    big = engine(states, 64, "f16x3", gpu, warmup=0)
    assert big.throughput and big.depth == 2 and big.max_inflight == 3 and big.recurrence not in (None, "valu")
    exact = engine(states, 64, "f32", gpu, warmup=0)
    assert not exact.throughput and exact.depth == 2 and exact.recurrence is None
    asked = engine(states, 64, "f16x3", gpu, warmup=0, recurrence="valu", lanes=1, inflight=4)
    assert not asked.throughput and asked.recurrence == "valu" and asked.depth == 1 and asked.max_inflight == 4
    assert not big._sub and not exact._sub and not asked._sub


# ------------------------------------------------------------------------------------------------ serving
def _tests_on_path():
    here = str(Path(__file__).resolve().parent)
    if here not in sys.path:
        sys.path.insert(0, here)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("rate,rings", [(16000, True), (16000, False), (48000, True)])
def test_stream_server_equals_dedicated_pipelines(gpu, states, precision, rate, rings):
    """StreamServer with the WeSpeaker model builds a WeSpeakerBatch: streams join late and push irregular amounts,
    on device rings and in host-window mode, and at 48 kHz through the device resampler; each stream's RTTM equals
    that of its own SpeakerDiarization fed the same windows (through blocks.Resample at the other rate)."""
    from diart_amd.blocks import Resample
    from diart_amd.inference import PredictionAccumulator, rolling_windows
    from diart_amd.serve import StreamServer
    _tests_on_path()
    import resample_ref as R
    lengths = {"ann": 9.0, "ben": 7.5, "cy": 8.0}
    audio = {}
    for i, (k, v) in enumerate(lengths.items()):
        x = synth_streams(1, v, seed0=1700 + i)[0]
        audio[k] = x if rate == SR else R.resample(x, SR, rate).astype(np.float32)
    srv = StreamServer(M.HipSegmentation(states[False], max_batch=4, precision=precision),
                       M.HipWeSpeakerEmbedding(states["emb"], max_batch=4, precision=precision), max_streams=4,
                       device=gpu, input_sample_rate=rate, device_rings=rings, tau_active=TAU)
    assert isinstance(srv.batch, WeSpeakerBatch) and (srv.rings is not None) == rings
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
        widths.append(len(srv.step()))
        tick += 1
    srv.drain()
    assert max(widths) >= 2, "windows of different streams were never batched together"
    blk = Resample(rate, SR, gpu) if rate != SR else None
    spoken = 0
    for k in audio:
        got = srv.close(k)
        pipe, acc = own_pipeline(states, precision, gpu), PredictionAccumulator(k)
        hop = rate // 2
        usable = len(audio[k]) // hop * hop
        blocks = (audio[k][None, i:i + hop] for i in range(0, usable, hop))
        for w in rolling_windows(blocks, 5.0, 0.5, rate):
            for out in pipe([blk(w) if blk is not None else w]):
                acc.on_next(out)
        want = acc.get_prediction()
        assert want is not None and got.to_rttm() == want.to_rttm(), (precision, rate, rings, k)
        spoken += len(got)
    assert spoken > 0


# ------------------------------------------------------------------------------------------------ lifecycle
def test_engines_release_their_device_memory(gpu, states):
    """Create, run and drop an 8-stream engine ten times (two lanes: two segmentation handles and two dz_wsp arenas of
    ~270 MB, pinned slots, HIP streams).  As in tests/test_gpu_lifecycle.py the first few engines fill pools the HIP
    runtime keeps; from the fifth to the tenth the free device memory does not move."""
    audio = torch.from_numpy(synth_streams(8, 6.0, seed0=77)).to(gpu)
    x = torch.zeros(64, device=gpu)
    for i in range(80):                       # torch's stream pools, so that their growth is not counted against the engines
        with torch.cuda.stream(torch.cuda.Stream(gpu, priority=-1 if i % 2 else 0)):
            x.add_(1)
    after = []
    for k in range(10):
        pipe = engine(states, 8, "f16x3", gpu, tail=True, warmup=3)
        for t in range(3):
            pipe(audio[:, t * HOP: t * HOP + W])
        del pipe
        gc.collect()
        torch.cuda.synchronize(gpu)
        torch.cuda.empty_cache()
        after.append(torch.cuda.mem_get_info(gpu)[0])
    print("free device memory after each engine, MB:", [round(a / MB) for a in after])
    assert max(after[5:]) - min(after[5:]) < 8 * MB, [round(a / MB) for a in after]
    assert after[0] - after[-1] < 512 * MB, [round(a / MB) for a in after]
