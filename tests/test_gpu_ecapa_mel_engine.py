"""The mel-spectrogram ECAPA-TDNN through the blocks API and on the N-stream engine.

Blocks: ``SpeakerDiarization`` (either segmentation model, ``normalize_embedding_weights=True``) over the five 5 s
windows of a 7 s synthetic stream assigns the speakers that the reference-shaped CPU pipeline of tests/titanet_chain.py
assigns when it is fed the float64 restatement's embeddings (tests/ecapa_mel_ref.py) rounded to float32, on the
segmentation the GPU produced.  A step at which that reference alone flips under the rounding proves nothing and would be
excluded with the steps after it; the stream's seed is chosen so that none is (checked on the CPU with the oracle's
segmentation for both models: 3 speakers, no flip).

Engine: ``StreamBatch(seg, emb, 2)`` is a ``GroupsBatch`` with 2 lanes and reproduces each stream's own batch-1 pipeline
over 6 steps; one ``StreamServer`` step accepts the pair."""
import numpy as np
import pytest
import torch

import ecapa_mel_ref as R
import titanet_chain as chain
from diart_amd import models as M
from diart_amd.pipeline import GroupsBatch, StreamBatch
from diart_amd.synth import synth_ecapa_state, synth_segmentation_state, synth_stream, synth_streams

pytestmark = pytest.mark.gpu

W, HOP = 80000, 8000
STREAM_SEED, STREAM_SECONDS = 33, 7.0


@pytest.fixture(scope="module")
def states():
    return synth_segmentation_state(seed=77, powerset=True), synth_ecapa_state()


@pytest.mark.parametrize("powerset", [True, False], ids=["segmentation-3.0", "segmentation"])
def test_blocks_match_the_reference_shaped_cpu_pipeline(gpu, powerset):
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    from test_gpu_der import rolling_chunks
    emb_sd = synth_ecapa_state()
    seg_sd = synth_segmentation_state(seed=77, powerset=True) if powerset else synth_segmentation_state()
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=chain.BATCH, powerset=powerset),
        embedding=M.EmbeddingModel.from_state(emb_sd, max_batch=chain.BATCH * chain.SPEAKERS, arch="ecapa-mel"),
        latency=0.5, tau_active=0.5, normalize_embedding_weights=True, device=gpu)
    pipe = SpeakerDiarization(cfg)
    chunks = rolling_chunks(synth_stream(STREAM_SEED, STREAM_SECONDS))
    steps = len(chunks)
    assert steps == 5 <= chain.BATCH
    outs = pipe(chunks)
    x = torch.from_numpy(np.stack([c.data[:, 0] for c in chunks]))[:, None, :]
    seg = cfg.segmentation(x.to(gpu)).cpu()
    assert type(cfg.embedding.model) is M.HipEcapaMelEmbedding
    got = [chain.annotation_tracks(ann) for ann, _ in outs]
    emb = chain.embed(R.MelSpecEmbeddingRef(emb_sd).embed, chunks, seg)
    want, want64 = chain.tracks(seg, emb, rounded=True), chain.tracks(seg, emb, rounded=False)
    first_flip = next((i for i in range(steps) if want[i] != want64[i]), steps)
    speakers = sorted({s for st in want for *_, s in st})
    print(f"ecapa-mel blocks ({'powerset' if powerset else 'multilabel'}): {steps} steps, {steps - first_flip} excluded, "
          f"{sum(map(len, want))} turns of speakers {speakers}")
    assert first_flip == steps, f"the reference flips under float32 rounding at step {first_flip}: choose another seed"
    assert sum(map(len, want)) >= steps and len(speakers) >= 2, "the stream does not exercise the clustering"
    for i in range(steps):
        assert got[i] == want[i], (i, got[i], want[i])


def blocks_pipeline(states, gpu):
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    seg_sd, emb_sd = states
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=1, powerset=True),
        embedding=M.EmbeddingModel.from_state(emb_sd, max_batch=3, arch="ecapa-mel"),
        latency=0.5, tau_active=0.5, normalize_embedding_weights=True, device=gpu)
    return SpeakerDiarization(cfg)


def test_stream_batch_reproduces_each_streams_pipeline(gpu, states):
    """2 streams x 6 steps on 2 lanes: every stream's accumulated turns, written as RTTM, equal those of its own
    SpeakerDiarization at batch 1."""
    from diart_amd.blocks.aggregation import BatchedOutputTail
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    from test_gpu_der import accumulate
    seg_sd, emb_sd = states
    n, steps = 2, 6
    audio = synth_streams(n, (W + HOP * steps) / 16000.0, seed0=950)
    d_audio = torch.from_numpy(audio).to(gpu)
    pipe = StreamBatch(M.HipSegmentation(seg_sd, max_batch=n, powerset=True), M.HipEcapaMelEmbedding(emb_sd), n,
                       tau_active=0.5, normalize_embedding_weights=True, device=gpu, tail=True)
    assert isinstance(pipe, GroupsBatch) and pipe.depth == 2
    refs = [blocks_pipeline(states, gpu) for _ in range(n)]
    got, want = [[] for _ in range(n)], [[] for _ in range(n)]
    for t in range(steps):
        ticket = pipe.launch(d_audio[:, t * HOP:t * HOP + W])
        pipe.finish(ticket, want_scores=False)
        turns, nturns = ticket["tail"][4], ticket["tail"][5]
        for i in range(n):
            c = SlidingWindowFeature(audio[i][t * HOP:t * HOP + W, None],
                                     SlidingWindow(start=t * 0.5, duration=1 / 16000, step=1 / 16000))
            want[i] += refs[i]([c])
            got[i].append((BatchedOutputTail.annotation(turns[i], int(nturns[i])), None))
    for i in range(n):
        a, b = accumulate(got[i], f"s{i}").to_rttm(), accumulate(want[i], f"s{i}").to_rttm()
        assert b and a == b, i


def test_stream_server_takes_the_pair(gpu, states):
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = states
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=2, powerset=True), M.HipEcapaMelEmbedding(emb_sd),
                       max_streams=2, tau_active=0.5, normalize_embedding_weights=True, device=gpu)
    assert isinstance(srv.batch, GroupsBatch)
    audio = synth_streams(2, 5.5, seed0=970)
    for i, k in enumerate(("ana", "ben")):
        srv.open(k)
        srv.push(k, audio[i])
    assert len(srv.step()) == 2
    srv.drain()
    for k in ("ana", "ben"):
        assert srv.close(k) is not None
