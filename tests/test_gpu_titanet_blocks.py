"""Blocks API: ``SpeakerDiarization`` with the NeMo TitaNet-L embedding (and either segmentation model,
``normalize_embedding_weights=True``) against the reference-shaped CPU pipeline of tests/titanet_chain.py — the oracle's
clustering and tail fed with the float64 restatement's embeddings rounded to float32 — over a synthetic stream: every
step's speech turns carry the same global speakers at the same times.

The CPU pipeline runs on the segmentation the GPU produced (its parity has its own tests), so only the embedding and
what follows it are compared.  A step at which the reference alone flips under the float32 rounding of its embeddings
(its "f64" and "f32" pipelines disagree) proves nothing and is excluded, together with the steps after it (the
clustering state has diverged); the test fails if that excludes more than 1 % of the steps.  The stream's seed is
chosen so that no step is excluded (tests/test_titanet_host.py checks that on the CPU with the oracle's segmentation)."""
import numpy as np
import pytest
import torch

import titanet_chain as chain
from diart_amd import models as M
from diart_amd.synth import synth_segmentation_state, synth_stream, synth_titanet_state
from titanet_ref import TitaNetRef

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("powerset", [True, False], ids=["segmentation-3.0", "segmentation"])
def test_blocks_match_the_reference_shaped_cpu_pipeline(gpu, powerset):
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    from test_gpu_der import rolling_chunks
    emb_sd = synth_titanet_state()
    seg_sd = synth_segmentation_state(seed=77, powerset=True) if powerset else synth_segmentation_state()
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=chain.BATCH, powerset=powerset),
        embedding=M.EmbeddingModel.from_state(emb_sd, max_batch=chain.BATCH * chain.SPEAKERS), latency=0.5, tau_active=0.5,
        normalize_embedding_weights=True, device=gpu)
    pipe = SpeakerDiarization(cfg)
    chunks = rolling_chunks(synth_stream(chain.STREAM_SEED, chain.STREAM_SECONDS))
    outs, segs = [], []
    for i in range(0, len(chunks), chain.BATCH):
        batch = chunks[i:i + chain.BATCH]
        outs += pipe(batch)
        x = torch.from_numpy(np.stack([c.data[:, 0] for c in batch]))[:, None, :]
        segs.append(cfg.segmentation(x.to(gpu)).cpu())
    assert type(cfg.embedding.model) is M.HipTitaNetEmbedding
    seg = torch.cat(segs)
    got = [chain.annotation_tracks(ann) for ann, _ in outs]
    emb = chain.embed(TitaNetRef(emb_sd), chunks, seg)
    want, want64 = chain.tracks(seg, emb, rounded=True), chain.tracks(seg, emb, rounded=False)
    steps = len(chunks)
    first_flip = next((i for i in range(steps) if want[i] != want64[i]), steps)
    excluded = steps - first_flip
    nan_rows = int(torch.isnan(emb).any(dim=-1).sum())
    speakers = sorted({s for st in want for *_, s in st})
    print(f"titanet blocks ({'powerset' if powerset else 'multilabel'}): {steps} steps, {excluded} excluded, "
          f"{sum(map(len, want))} turns of speakers {speakers}, {nan_rows} NaN embedding rows of {emb.shape[0] * emb.shape[1]}")
    assert excluded <= 0.01 * steps, f"the reference flips under float32 rounding at step {first_flip}: choose another seed"
    assert sum(map(len, want)) >= steps and len(speakers) >= 2, "the stream does not exercise the clustering"
    for i in range(first_flip):
        assert got[i] == want[i], (i, got[i], want[i])
