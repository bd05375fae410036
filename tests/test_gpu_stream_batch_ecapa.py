"""Config 3 (powerset segmentation + ECAPA-TDNN) on the N-stream engine: ``StreamBatch`` and ``StreamServer`` with a
``HipEcapaEmbedding``.  Per stream the engine must produce what that stream's own pipeline produces
(``SpeakerDiarization`` at batch 1, the live reference's ``StreamingInference``): each stream's K speaker rows are
embedded with their own batch geometry, whatever the other streams hold, and ``launch`` does not wait for the GPU."""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.pipeline import GroupsBatch, StreamBatch
from diart_amd.synth import synth_ecapa_state, synth_segmentation_state, synth_streams

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16x3", "f32")
W, HOP = 80000, 8000


@pytest.fixture(scope="module")
def states():
    return synth_segmentation_state(seed=77, powerset=True), synth_ecapa_state()


def engine(states, n, precision, gpu, **kw):
    seg_sd, emb_sd = states
    return StreamBatch(M.HipSegmentation(seg_sd, max_batch=n, powerset=True, precision=precision),
                       M.HipEcapaEmbedding(emb_sd, precision=precision), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu, **kw)


def config3(states, precision, gpu):
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    seg_sd, emb_sd = states
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=1, powerset=True, precision=precision),
        embedding=M.EmbeddingModel.from_state(emb_sd, max_batch=3, precision=precision),
        latency=0.5, tau_active=0.5, normalize_embedding_weights=True, device=gpu)
    return SpeakerDiarization(cfg)


def chunk(x, t):
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    return SlidingWindowFeature(x[t * HOP:t * HOP + W, None], SlidingWindow(start=t * 0.5, duration=1 / 16000,
                                                                            step=1 / 16000))


def tracks(ann):
    return sorted((s.start, s.end, str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


def same_with_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_engine_equals_per_stream_pipelines(gpu, states, precision):
    """3 streams x 9 steps, 2 lanes: every step's speech turns (StreamBatch.diarize) equal those of the stream's own
    SpeakerDiarization at batch 1, and its embeddings (the blocks' embedding stage of that chunk alone) agree
    within 1e-6, NaN rows (too-short speakers) included."""
    n, steps = 3, 9
    audio = synth_streams(n, (W + HOP * steps) / 16000.0, seed0=950)
    d_audio = torch.from_numpy(audio).to(gpu)
    pipe = engine(states, n, precision, gpu, tail=True)
    assert pipe.depth == 2 and isinstance(pipe, GroupsBatch)
    refs = [config3(states, precision, gpu) for _ in range(n)]
    nan_seen = 0
    for t in range(steps):
        ticket = pipe.launch(d_audio[:, t * HOP:t * HOP + W])
        seg, emb, _, _ = pipe.finish(ticket, want_scores=False)
        emb = emb.copy()
        _, _, _, _, turns, nturns = ticket["tail"]
        from diart_amd.blocks.aggregation import BatchedOutputTail
        for i in range(n):
            c = chunk(audio[i], t)
            batch = torch.from_numpy(c.data)[None]
            rseg = refs[i].segmentation(batch)
            remb = refs[i].embedding(batch, rseg)
            want = refs[i].finalise([c], rseg, remb)[0][0]
            r = remb.reshape(-1, 192).numpy()
            assert same_with_nan(emb[i], r), (precision, t, i)
            ok = ~np.isnan(r).any(axis=1)
            assert np.abs(emb[i][ok] - r[ok]).max(initial=0.0) <= 1e-6, (precision, t, i)
            nan_seen += int((~ok).sum())
            assert np.abs(seg[i] - rseg.reshape(seg[i].shape).numpy()).max() <= 1e-6, (precision, t, i)
            got = BatchedOutputTail.annotation(turns[i], int(nturns[i]))
            assert tracks(got) == tracks(want), (precision, t, i)
    print(f"{precision}: {nan_seen} NaN embedding rows over {n * steps * 3}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stream_server_equals_dedicated_pipelines(gpu, states, precision):
    """StreamServer with a config-3 model pair: 3 streams of different lengths that join at different times and
    push odd block sizes; every stream's RTTM equals its own StreamingInference(SpeakerDiarization, batch 1)."""
    from diart_amd.inference import StreamingInference
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = states
    lengths = {"ana": 9.0, "ben": 7.5, "cy": 8.0}
    audio = {k: synth_streams(1, v, seed0=970 + i)[0] for i, (k, v) in enumerate(lengths.items())}
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=3, powerset=True, precision=precision),
                       M.HipEcapaEmbedding(emb_sd, precision=precision), max_streams=3, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu)
    assert isinstance(srv.batch, GroupsBatch)
    rng = np.random.default_rng(5)
    pos = {k: 0 for k in audio}
    join_at = {"ana": 0, "ben": 2, "cy": 5}
    tick, widths = 0, []
    while any(pos[k] < len(audio[k]) for k in audio):
        for k in audio:
            if tick == join_at[k]:
                srv.open(k)
            if tick >= join_at[k] and pos[k] < len(audio[k]):
                m = int(rng.integers(2000, 30000))
                srv.push(k, audio[k][pos[k]:pos[k] + m])
                pos[k] += m
        widths.append(len(srv.step()))
        tick += 1
    srv.drain()
    assert max(widths) >= 2, "windows of different streams were never batched together"
    for k in audio:
        got = srv.close(k)
        usable = len(audio[k]) // HOP * HOP
        want = StreamingInference(config3(states, precision, gpu), audio[k][:usable], 16000, k, (0, 0), 1)()
        assert want is not None and got.to_rttm() == want.to_rttm(), (precision, k)


def test_partial_steps_and_resets(gpu, states):
    """``slots=`` steps (some streams only) and ``reset(slot)`` give every stream the outputs a full-step engine
    computes for it: embeddings bitwise (each stream's rows are a group of their own), scores and assignments."""
    n, steps = 4, 8
    audio = synth_streams(n, (W + HOP * steps) / 16000.0, seed0=990)
    d_audio = torch.from_numpy(audio).to(gpu)
    full = engine(states, n, "f16x3", gpu)
    want = [[None] * steps for _ in range(n)]
    for t in range(steps):
        seg, emb, scores, assign = full(d_audio[:, t * HOP:t * HOP + W])
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
        rows = torch.stack([d_audio[i, pos[i] * HOP:pos[i] * HOP + W] for i in sel])
        _, emb, scores, assign = part.finish(part.launch(rows, slots=sel))
        for j, i in enumerate(sel):
            we, ws, wa = want[i][pos[i]]
            assert same_with_nan(emb[j], we) and np.array_equal(np.nan_to_num(emb[j]), np.nan_to_num(we)), (sel, i)
            assert np.array_equal(scores[j], ws) and np.array_equal(np.asarray(assign[j]), wa), (sel, i)
            pos[i] += 1
            checked += 1
    assert checked >= 20


def test_launch_does_not_wait_for_the_gpu(gpu, states):
    """After its warm-up, StreamBatch.launch in the ECAPA form returns while work queued before it is pending (the
    embedding geometry is derived on the device), and the step's results equal an engine that never waited."""
    n = 4
    audio = torch.from_numpy(synth_streams(n, (W + 2 * HOP) / 16000.0, seed0=995)).to(gpu)
    pipe, ref = engine(states, n, "f16x3", gpu), engine(states, n, "f16x3", gpu)
    for p in (pipe, ref):
        p.finish(p.launch(audio[:, :W]))
    want = [x.copy() for x in ref.finish(ref.launch(audio[:, HOP:HOP + W]))[:2]]
    cyc, ms = 20_000_000, 0.0
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
    assert pending, "StreamBatch.launch waited for work queued before it"
    assert np.array_equal(seg, want[0]) and same_with_nan(emb, want[1])
    assert np.array_equal(np.nan_to_num(emb), np.nan_to_num(want[1]))


def test_ecapa_form_refuses_what_it_cannot_do(gpu, states):
    with pytest.raises(ValueError):
        engine(states, 4, "f16x3", gpu, emb_split=2)
    pipe = engine(states, 64, "f16x3", gpu, warmup=0)
    assert pipe.depth == 2 and pipe.max_inflight == 3
    serial = engine(states, 2, "f16x3", gpu, lanes=1, serial=True, warmup=0)
    x = torch.from_numpy(synth_streams(2, 5.0, seed0=997)).to(gpu)
    _, emb, _, _ = serial(x)
    assert emb.shape == (2, 3, 192)
