"""NeMo TitaNet-L on the N-stream engine: ``StreamBatch`` and ``StreamServer`` with a ``HipTitaNetEmbedding``, in the
groups form ECAPA-TDNN runs in (tests/test_gpu_stream_batch_ecapa.py makes the same assertions for config 3).  Per
stream the engine must produce what that stream's own pipeline produces (``SpeakerDiarization`` at batch 1, the live
reference's ``StreamingInference``) — which also shows that the blocks API takes the model with
``normalize_embedding_weights=True``."""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.pipeline import GroupsBatch, StreamBatch
from diart_amd.synth import synth_titanet_state, synth_segmentation_state, synth_streams

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16x3", "f32")
W, HOP = 80000, 8000


@pytest.fixture(scope="module")
def states():
    return synth_segmentation_state(seed=77, powerset=True), synth_titanet_state()


def engine(states, n, precision, gpu, **kw):
    seg_sd, emb_sd = states
    return StreamBatch(M.HipSegmentation(seg_sd, max_batch=n, powerset=True, precision=precision),
                       M.HipTitaNetEmbedding(emb_sd, precision=precision), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu, **kw)


def blocks_pipeline(states, precision, gpu):
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
    within 1e-6; NaN rows (too-short speakers) must sit at the same places when the stream produces any (the count
    is printed; tests/test_gpu_titanet.py covers the NaN rules themselves)."""
    n, steps = 3, 9
    audio = synth_streams(n, (W + HOP * steps) / 16000.0, seed0=950)
    d_audio = torch.from_numpy(audio).to(gpu)
    pipe = engine(states, n, precision, gpu, tail=True)
    assert pipe.depth == 2 and isinstance(pipe, GroupsBatch)
    refs = [blocks_pipeline(states, precision, gpu) for _ in range(n)]
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
    """StreamServer with a powerset segmentation + TitaNet pair: 3 streams of different lengths that join at different times and
    push odd block sizes; every stream's RTTM equals its own StreamingInference(SpeakerDiarization, batch 1)."""
    from diart_amd.inference import StreamingInference
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = states
    lengths = {"ana": 9.0, "ben": 7.5, "cy": 8.0}
    audio = {k: synth_streams(1, v, seed0=970 + i)[0] for i, (k, v) in enumerate(lengths.items())}
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=3, powerset=True, precision=precision),
                       M.HipTitaNetEmbedding(emb_sd, precision=precision), max_streams=3, tau_active=0.5,
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
        want = StreamingInference(blocks_pipeline(states, precision, gpu), audio[k][:usable], 16000, k, (0, 0), 1)()
        assert want is not None and got.to_rttm() == want.to_rttm(), (precision, k)
