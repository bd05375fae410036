"""SpeakerDiarization / VoiceActivityDetection vs the REFERENCE'S OWN pipeline classes.

``tests/golden/pipeline_toy.npz`` holds what ``/root/reference/src/diart/blocks/diarization.py`` and
``blocks/vad.py`` (loaded by path, unmodified, around the toy models of ``golden/scenarios.py``)
returned chunk by chunk for three (latency, batch size, timestamp shift, thresholds) cases, plus the
segmentation / embeddings their blocks handed to the clustering (``make_golden.py::pipelines``).

* CPU (here): the HOST half of this package's pipelines (``finalise``: C++ clustering +
  aggregation + binarisation in one call, timestamps, buffers, shift) fed with the reference blocks'
  own segmentation / embeddings must return the reference's speech turns EXACTLY.
* GPU (``-m gpu``): the whole pipeline — blocks around the same toy models, OSP / normalisation as
  HIP kernels — must give those turns again (boundaries to 1e-9: nothing in between is discretised
  differently unless an OSP weight moves an embedding across a clustering threshold).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLD))
import scenarios  # noqa: E402

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks import (SpeakerDiarization, SpeakerDiarizationConfig, VoiceActivityDetection,  # noqa: E402
                              VoiceActivityDetectionConfig)
from diart_amd.features import SlidingWindow, SlidingWindowFeature  # noqa: E402


def _chunks():
    stream = scenarios.pipeline_stream()
    S, H = 80000, 8000
    return [SlidingWindowFeature(stream[i * H:i * H + S, None], SlidingWindow(start=i * 0.5, duration=1 / 16000, step=1 / 16000))
            for i in range((len(stream) - S) // H + 1)]


def _table(outputs):
    rows = []
    for i, (ann, _) in enumerate(outputs):
        for seg, _, label in ann.itertracks(yield_label=True):
            rows.append([i, seg.start, seg.end, float(label[len("speaker"):]) if label.startswith("speaker") else 0.0])
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def _digest(outputs):
    return np.array([[w.data.shape[0], w.sliding_window.start, w.sliding_window.step,
                      float(np.asarray(w.data, dtype=np.float64).sum()), w.data[0, 0], w.data[-1, 0]]
                     for _, w in outputs], dtype=np.float64)


def _pipelines(name, device):
    latency, bs, shift, tau, rho, delta = scenarios.PIPE_CASES[name]
    cfg = SpeakerDiarizationConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                   embedding=M.EmbeddingModel(lambda: scenarios.ToyEmbedding()), latency=latency,
                                   tau_active=tau, rho_update=rho, delta_new=delta, device=device)
    vcfg = VoiceActivityDetectionConfig(segmentation=M.SegmentationModel(lambda: scenarios.ToySegmentation()),
                                        latency=latency, tau_active=tau, device=device)
    dia, vad = SpeakerDiarization(cfg), VoiceActivityDetection(vcfg)
    dia.set_timestamp_shift(shift)
    vad.set_timestamp_shift(shift)
    return dia, vad, bs


def test_toy_models_have_the_surface_of_the_hip_models():
    """The stand-ins are driven through the same methods the reference's LazyModel uses on
    HipSegmentation / HipEmbedding: same call signatures, ``to`` returns the model, no nn.Module."""
    import inspect
    for toy, hip in ((scenarios.ToySegmentation, M.HipSegmentation), (scenarios.ToyEmbedding, M.HipEmbedding)):
        a, b = inspect.signature(toy.__call__), inspect.signature(hip.__call__)
        assert [p.name for p in a.parameters.values()][:2] == [p.name for p in b.parameters.values()][:2]
        assert len(a.parameters) == len(b.parameters)
        assert not issubclass(toy, torch.nn.Module) and not issubclass(hip, torch.nn.Module)
        assert list(inspect.signature(toy.to).parameters) == list(inspect.signature(hip.to).parameters)


@pytest.mark.parametrize("name", list(scenarios.PIPE_CASES))
def test_host_half_reproduces_the_reference_pipelines_outputs(name):
    z = np.load(GOLD / "pipeline_toy.npz")
    chunks = _chunks()
    assert len(chunks) == int(z["num_chunks"])
    dia, vad, bs = _pipelines(name, torch.device("cpu"))
    seg, emb = torch.from_numpy(z[f"{name}_seg"]), torch.from_numpy(z[f"{name}_emb"])
    outs, vouts = [], []
    for i in range(0, len(chunks), bs):
        outs += dia.finalise(chunks[i:i + bs], seg[i:i + bs], emb[i:i + bs])
        vouts += vad.finalise(chunks[i:i + bs], seg[i:i + bs])
    assert np.array_equal(_table(outs), z[f"{name}_turns"])
    assert np.array_equal(_digest(outs), z[f"{name}_audio"])
    assert np.array_equal(_table(vouts), z[f"{name}_vad_turns"])
    # reset() starts a new stream: the same input gives the same output again
    dia.reset()
    dia.set_timestamp_shift(scenarios.PIPE_CASES[name][2])
    again = []
    for i in range(0, len(chunks), bs):
        again += dia.finalise(chunks[i:i + bs], seg[i:i + bs], emb[i:i + bs])
    assert np.array_equal(_table(again), z[f"{name}_turns"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(scenarios.PIPE_CASES))
def test_whole_pipeline_on_the_gpu_reproduces_the_reference_pipelines_outputs(name):
    z = np.load(GOLD / "pipeline_toy.npz")
    chunks = _chunks()
    dia, vad, bs = _pipelines(name, torch.device("cuda", 0))
    outs, vouts = [], []
    for i in range(0, len(chunks), bs):
        outs += dia(chunks[i:i + bs])
        vouts += vad(chunks[i:i + bs])
    got, want = _table(outs), z[f"{name}_turns"]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, [0, 3]], want[:, [0, 3]])            # same chunks, same speakers
    assert np.allclose(got[:, 1:3], want[:, 1:3], rtol=0, atol=1e-9)
    assert np.array_equal(_digest(outs), z[f"{name}_audio"])
    gv, wv = _table(vouts), z[f"{name}_vad_turns"]
    assert gv.shape == wv.shape and np.allclose(gv, wv, rtol=0, atol=1e-9)
