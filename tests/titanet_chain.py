"""The reference-shaped CPU pipeline around the float64 TitaNet restatement (tests/titanet_ref.py), for the blocks-API
test and its CPU seed check: OverlappedSpeechPenalty with min-max normalisation -> the wrapper call over the batch's
(chunk, speaker) rows -> EmbeddingNormalization -> the oracle's OnlineSpeakerClustering -> DelayedAggregation and
Binarize (oracle.tail_ref), chunk by chunk.  ``embed`` computes the float64 embeddings once; ``tracks`` runs the
clustering and tail on them either unrounded ("f64") or rounded to float32 first ("f32", what the reference's float32
models hand to its clustering)."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

SPEAKERS, BATCH = 3, 8
STREAM_SEED, STREAM_SECONDS = 31, 12.0       # (chosen so that the "f64" and "f32" pipelines agree on every step)


def embed(ref, chunks, seg: torch.Tensor) -> torch.Tensor:
    """chunks: SlidingWindowFeature list; seg (n, F, K) float32 -> raw float64 embeddings (n, K, 192), NaN rows kept.
    Rows are embedded in the batches of ``BATCH`` chunks the blocks API is driven with (one wrapper call each)."""
    from oracle.functional_ref import overlapped_speech_penalty_ref
    out = []
    for i0 in range(0, len(chunks), BATCH):
        x = torch.from_numpy(np.stack([c.data[:, 0] for c in chunks[i0:i0 + BATCH]]))[:, None, :]
        w = overlapped_speech_penalty_ref(seg[i0:i0 + BATCH], normalize=True)
        B, K = x.shape[0], w.shape[2]
        rows = x.repeat(1, K, 1).reshape(B * K, 1, -1)
        out.append(ref(rows, w.permute(0, 2, 1).reshape(B * K, -1)).view(B, K, -1))
    return torch.cat(out)


def tracks(seg: torch.Tensor, emb: torch.Tensor, rounded: bool, tau=0.5, rho=0.3, delta=1.0, latency=0.5) -> List[list]:
    """Per step: sorted [(start, end, global speaker)] of the turns the tail emits, times rounded to 1 us."""
    from oracle.clustering_ref import OnlineSpeakerClusteringRef
    from oracle.functional_ref import normalize_embeddings_ref
    from oracle.pyannote_stub import SlidingWindow as SW, SlidingWindowFeature as SWF
    from oracle.tail_ref import TailRef
    clu, tail = OnlineSpeakerClusteringRef(tau, rho, delta, "cosine", 20), TailRef(tau, 0.5, latency)
    e = normalize_embeddings_ref(emb.float() if rounded else emb).numpy()
    F, out = seg.shape[1], []
    for i in range(seg.shape[0]):
        scores, _ = clu(seg[i].numpy(), e[i])
        _, turns = tail(SWF(scores, SW(start=i * 0.5, duration=5 / F, step=5 / F)))
        out.append(sorted((round(a, 6), round(b, 6), int(spk)) for a, b, spk in turns))
    return out


def annotation_tracks(ann) -> list:
    """The same form from an Annotation whose labels are ``speaker<g>`` (the blocks API's output)."""
    return sorted((round(s.start, 6), round(s.end, 6), int(str(lab).replace("speaker", "")))
                  for s, _, lab in ann.itertracks(yield_label=True))
