"""WeSpeaker ResNet34 (pyannote/wespeaker-voxceleb-resnet34-LM) on the GPU against the float64 restatement
(tests/wespeaker_ref.py), in both arithmetic modes: stage by stage through dz_wsp_peek (fbank, conv1, layers 1 - 4,
pooled statistics, embedding), NaN rows, batch invariance, forward_multi vs the reference-shaped call, no host
synchronisation, and the whole pipeline against the all-CPU chain.

Gates (those of tests/test_gpu_ecapa.py): relative L2 <= 2e-4 on every stage, cosine >= 0.99999 on embeddings."""
import numpy as np
import pytest
import torch

import wespeaker_ref as R
from diart_amd import models as M
from diart_amd.synth import synth_streams, synth_wespeaker_state

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")
# (samples, weight frames): 5 s without weights; 2 s with pyannote/segmentation's 293 frames; 79760 samples
# (497 -> 497 -> 249 -> 125 -> 63 frames: odd at every stride) with segmentation-3.0's 589 frames
CASES = [(80000, None), (32000, 293), (79760, 589)]


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def cos_min(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1).min().item()


def case_inputs(S, Fw, n=3, seed=0):
    x = torch.from_numpy(synth_streams(n, S / 16000 + 0.01, seed0=60 + seed))[:, :S].contiguous()
    w = None
    if Fw is not None:
        g = torch.Generator().manual_seed(S + Fw)
        w = torch.rand(n, Fw, generator=g)
        w[:, : Fw // 5] = 0.0                        # a silent stretch: weights exactly zero there
    return x, w


@pytest.fixture(scope="module")
def state():
    return synth_wespeaker_state()


@pytest.fixture(scope="module")
def oracle(state):
    return R.WeSpeakerRef(state)


@pytest.fixture(scope="module")
def oracle_stages(oracle):
    cache = {}

    def get(S, Fw):
        if (S, Fw) not in cache:
            x, w = case_inputs(S, Fw)
            cache[(S, Fw)] = oracle.stages(x, w)
        return cache[(S, Fw)]
    return get


@pytest.fixture(scope="module")
def hips(gpu, state):
    return {p: M.HipWeSpeakerEmbedding(state, max_batch=8, precision=p).to(gpu) for p in PRECISIONS}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("S,Fw", CASES)
def test_stages_against_float64(gpu, hips, oracle_stages, precision, S, Fw):
    hip = hips[precision]
    x, w = case_inputs(S, Fw)
    got = hip(x[:, None].to(gpu), None if w is None else w.to(gpu)).cpu()
    want = oracle_stages(S, Fw)
    T = R.frames(S)
    N = x.shape[0]
    names = ["fbank", "conv1", "layer1", "layer2", "layer3", "layer4", "pooled"]
    errs = {}
    for i, name in enumerate(names):
        g, frames = hip.peek(S, i)
        ref = want[name]
        assert g.numel() == ref.numel(), name
        if i <= 1:
            assert frames == T[0]
        elif i <= 5:
            assert frames == T[i - 1]
        errs[name] = rel(g.cpu().view(ref.shape), ref)
    errs["emb"] = rel(got, want["emb"])
    print(precision, S, Fw, {k: f"{v:.2e}" for k, v in errs.items()}, "cos", cos_min(got, want["emb"]))
    assert all(v <= 2e-4 for v in errs.values()), errs
    assert cos_min(got, want["emb"]) >= 0.99999


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_weights_and_nan_rows(gpu, hips, oracle, precision):
    hip = hips[precision]
    S = 32000
    x, w = case_inputs(S, 293, n=4, seed=5)
    w[1] = 0.0                                        # all-zero weights: mean 0, std 0 by the 3.1 formula: finite
    base = hip(x[:, None].to(gpu), w.to(gpu)).cpu()
    assert torch.isfinite(base).all()
    want1 = oracle(x[1:2], w[1:2])
    assert torch.isfinite(want1).all() and rel(base[1:2], want1) <= 2e-4
    xb = x.clone()
    xb[2, 12345] = float("nan")
    xb[3, 20000] = float("inf")
    got = hip(xb[:, None].to(gpu), w.to(gpu)).cpu()
    assert torch.isnan(got[2]).all() and torch.isnan(got[3]).all()
    assert torch.equal(got[:2], base[:2]), "a NaN row changed its neighbours"
    # a NaN past the last frame (S - 400 not a multiple of 160: samples no frame reads) is not seen, like kaldi
    S2 = 32100
    x2 = torch.from_numpy(synth_streams(2, 2.1, seed0=9))[:, :S2].contiguous()
    ok = hip(x2[:, None].to(gpu)).cpu()
    x2[0, S2 - 1] = float("nan")
    assert torch.equal(hip(x2[:, None].to(gpu)).cpu(), ok)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_invariance(gpu, state, precision):
    """Every row of a batch of 1, 3, 64 or 192 (output tiles that straddle rows, ragged last tiles) is bit-identical
    to that row alone: every output element is its own dot product in a fixed order, and the fbank, pooling and
    seg_1 reductions are per row."""
    hip = M.HipWeSpeakerEmbedding(state, max_batch=192, precision=precision).to(gpu)
    S = 32000
    x = torch.from_numpy(synth_streams(192, 2.01, seed0=300))[:, :S].contiguous().to(gpu)
    g = torch.Generator().manual_seed(11)
    w = torch.rand(192, 293, generator=g).to(gpu)
    alone = torch.stack([hip(x[i:i + 1, None], w[i:i + 1])[0] for i in range(192)]).cpu()
    for B in (1, 3, 64, 192):
        for start in sorted({0, 192 - B}):
            got = hip(x[start:start + B, None], w[start:start + B]).cpu()
            assert torch.equal(got, alone[start:start + B]), (B, start)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_multi_equals_repeated_rows(gpu, hips, precision):
    hip = hips[precision]
    S, K = 80000, 3
    x = torch.from_numpy(synth_streams(2, 5.01, seed0=70))[:, :S].contiguous().to(gpu)
    g = torch.Generator().manual_seed(4)
    w = torch.rand(2, K, 589, generator=g).to(gpu)
    multi = hip.forward_multi(x[:, None], w).cpu()
    rows = x[:, None].repeat(1, K, 1).reshape(2 * K, 1, S)
    want = hip(rows, w.reshape(2 * K, -1)).cpu().view(2, K, -1)
    assert torch.equal(multi, want)
    normed = hip.forward_multi(x[:, None], w, normalize=True).cpu()
    assert torch.allclose(normed, torch.nn.functional.normalize(want, dim=-1), rtol=0, atol=1e-6)


def sleep_cycles_for(seconds, device):
    cyc = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cyc)
    b.record()
    b.synchronize()
    return int(cyc * seconds * 1e3 / max(a.elapsed_time(b), 1e-3))


def test_forward_multi_does_not_wait_for_the_gpu(gpu, hips):
    hip = hips["f16x3"]
    S = 32000
    x = torch.from_numpy(synth_streams(4, 2.01, seed0=80))[:, :S].contiguous().to(gpu)
    w = torch.rand(4, 3, 293, generator=torch.Generator().manual_seed(2)).to(gpu)
    want = hip.forward_multi(x[:, None], w).cpu()            # (warm: the handle exists)
    cycles = sleep_cycles_for(0.3, gpu)
    torch.cuda.synchronize(gpu)
    torch.cuda._sleep(cycles)
    ev = torch.cuda.Event()
    ev.record()
    out = hip.forward_multi(x[:, None], w)
    pending = not ev.query()
    torch.cuda.synchronize(gpu)
    assert pending, "dz_wsp_forward_multi waited for work queued before it"
    assert torch.equal(out.cpu(), want)


# --------------------------------------------------------------------------- #
# the whole pipeline: blocks API vs the all-CPU chain (tests/test_gpu_der.py's gates and near-tie accounting)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("powerset", [True, False], ids=["segmentation-3.0", "segmentation"])
def test_pipeline_matches_cpu_chain(gpu, state, oracle, powerset):
    from oracle.clustering_ref import OnlineSpeakerClusteringRef
    from oracle.functional_ref import normalize_embeddings_ref, overlapped_speech_penalty_ref
    from oracle.models_ref import PyanNetRef, powerset_to_multilabel
    from oracle.pyannote_stub import SlidingWindow as SW, SlidingWindowFeature as SWF
    from oracle.tail_ref import TailRef
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    from diart_amd.features import Annotation, Segment
    from diart_amd.metrics import DiarizationErrorRate
    from diart_amd.synth import synth_segmentation_state, synth_stream
    from test_gpu_der import accumulate, rolling_chunks
    stream = synth_stream(31, 12.0)
    seg_sd = synth_segmentation_state(seed=77, powerset=True) if powerset else synth_segmentation_state()
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=16, powerset=powerset),
        embedding=M.EmbeddingModel.from_state(state, max_batch=16), latency=0.5, tau_active=0.5,
        normalize_embedding_weights=powerset, device=gpu)
    pipe = SpeakerDiarization(cfg)
    chunks = rolling_chunks(stream)
    outs = []
    for i in range(0, len(chunks), 8):
        outs += pipe(chunks[i:i + 8])
    hyp = accumulate(outs)
    # ---- all-CPU chain -------------------------------------------------------------------
    seg_m = PyanNetRef(powerset=powerset).eval()
    seg_m.load_state_dict(seg_sd)
    clu, tail, ref = OnlineSpeakerClusteringRef(0.5, 0.3, 1.0, "cosine", 20), TailRef(0.5, 0.5, 0.5), Annotation("stream")
    clu_i, tail_i, ref_i = OnlineSpeakerClusteringRef(0.5, 0.3, 1.0, "cosine", 20), TailRef(0.5, 0.5, 0.5), Annotation("stream")
    flips = near_ties = 0

    def embed(x, seg):
        w = overlapped_speech_penalty_ref(seg)
        if powerset:
            mn, mx = w.min(dim=1, keepdim=True).values, w.max(dim=1, keepdim=True).values
            w = ((w - mn) / (mx - mn)).nan_to_num(1e-8)
        B = x.shape[0]
        rows = x.repeat(1, 3, 1).reshape(B * 3, 1, -1)
        return normalize_embeddings_ref(oracle(rows, w.permute(0, 2, 1).reshape(B * 3, -1)).float().view(B, 3, -1))

    for i0 in range(0, len(chunks), 8):
        batch = chunks[i0:i0 + 8]
        x = torch.from_numpy(np.stack([c.data[:, 0] for c in batch]))[:, None, :]
        with torch.no_grad():
            out = seg_m(x)
        seg = cfg.segmentation(x.to(gpu)).cpu()
        if powerset:
            # hard powerset decisions may flip only where the two best classes are within fp32 noise (test_gpu_der.py)
            cpu_seg = powerset_to_multilabel(out)
            top2 = out.topk(2, dim=-1).values
            margin = top2[..., 0] - top2[..., 1]
            differ = (seg != cpu_seg).any(dim=-1)
            assert (margin[differ] < 1e-3).all(), "a hard decision flipped away from a near-tie"
            flips += int(differ.sum())
            near_ties += int((margin < 1e-3).sum())
        else:
            cpu_seg = out
            assert (seg - cpu_seg).abs().max() < 1e-4
        emb_g = embed(x, seg)
        same = torch.equal(seg, cpu_seg)
        emb_c = emb_g if same else embed(x, cpu_seg)
        for which_seg, emb, c_, t_, r_ in ((seg, emb_g, clu, tail, ref), (cpu_seg, emb_c, clu_i, tail_i, ref_i)):
            for j in range(len(batch)):
                i = i0 + j
                scores, _ = c_(which_seg[j].numpy(), emb[j].numpy())
                _, turns = t_(SWF(scores, SW(start=i * 0.5, duration=5 / 293, step=5 / 293)))
                for n, (a, b, spk) in enumerate(turns):
                    r_[Segment(a, b), (i, n)] = f"speaker{spk}"
    ref, ref_i = ref.support(0.05), ref_i.support(0.05)
    d = DiarizationErrorRate()(ref, hyp, detailed=True)
    di = DiarizationErrorRate()(ref_i, hyp, detailed=True)
    budget = 0.005 + 3 * flips * (5 / 293) / max(di["total"], 1e-9)
    print(f"wespeaker ({'powerset' if powerset else 'multilabel'}): DER(GPU vs CPU chain on the GPU's segmentation) = "
          f"{100 * d['diarization error rate']:.3f} % of {d['total']:.1f} s; DER(vs independent CPU chain) = "
          f"{100 * di['diarization error rate']:.3f} % (budget {100 * budget:.3f} %); {flips} flips at {near_ties} near ties")
    assert d["total"] > 1.0 and d["diarization error rate"] <= 0.005
    assert di["total"] > 1.0 and di["diarization error rate"] <= budget
