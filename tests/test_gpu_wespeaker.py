"""WeSpeaker ResNet34 (pyannote/wespeaker-voxceleb-resnet34-LM) on the GPU against the float64 restatement
(tests/wespeaker_ref.py), in both arithmetic modes: stage by stage through dz_wsp_peek (fbank, conv1, layers 1 - 4,
pooled statistics, embedding), NaN rows, batch invariance, forward_multi vs the reference-shaped call, no host
synchronisation, and the whole pipeline against the all-CPU chain.

Gates: those of tests/test_gpu_ecapa.py (relative L2 <= 2e-4 on every stage, cosine >= 0.99999 on embeddings) and,
stricter, per row and stage at about 3x the worst row measured (ROW_GATES); the pooling kernel alone on the model's
own layer-4 output; pyannote's float32 pooling arithmetic on single-non-zero-frame weights."""
import numpy as np
import pytest
import torch

import wespeaker_ref as R
from diart_amd import _lib, models as M
from diart_amd.synth import synth_streams, synth_wespeaker_state

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")
# (samples, weight frames): 5 s without weights; 2 s with pyannote/segmentation's 293 frames; 79760 samples
# (497 -> 497 -> 249 -> 125 -> 63 frames: odd at every stride) with segmentation-3.0's 589 frames; 1680 samples, the
# shortest the API accepts (9 -> 9 -> 5 -> 3 -> 2 frames); 10 s
CASES = [(80000, None), (32000, 293), (79760, 589), (1680, None), (160000, 293)]
STAGES = ["fbank", "conv1", "layer1", "layer2", "layer3", "layer4", "pooled"]
# per row and stage, about 3x the worst row measured on an MI355X over every case of this file and both precisions
# (relative L2 per row; fbank: the power-domain measure of fbank_error).  Worst rows measured (f16x3 / f32): fbank
# 1.07e-6 / 1.07e-6, conv1 1.72e-5 / 1.72e-5, layer1 1.52e-5 / 1.52e-5, layer2 1.07e-5 / 1.07e-5, layer3 5.72e-6 /
# 5.73e-6, layer4 5.03e-6 / 5.01e-6, pooled 6.80e-6 / 6.76e-6, emb 7.23e-6 / 7.22e-6, all on the quiet 1680-sample
# rows of the batch sweep (their log-mel features carry the f32 fbank's absolute error; the power-domain fbank
# measure does not grow there); the 2 s - 10 s rows stay at or below 2.2e-6.
_ROW_GATE = {"fbank": 3.2e-6, "conv1": 5.2e-5, "layer1": 4.6e-5, "layer2": 3.2e-5, "layer3": 1.8e-5, "layer4": 1.5e-5,
             "pooled": 2.1e-5, "emb": 2.2e-5}
ROW_GATES = {"f16x3": _ROW_GATE, "f32": _ROW_GATE}
POOL_GATE = 1e-6                # the pooling kernel alone, on the model's own layer-4 output (relative L2 per row;
                                # worst row measured 3.2e-7, Fw = 1, both precisions)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rel_rows(a, b):
    """relative L2 of every row (leading axis)"""
    a, b = a.double().reshape(a.shape[0], -1), b.double().reshape(b.shape[0], -1)
    return (a - b).norm(dim=1) / (b.norm(dim=1) + 1e-30)


def fbank_error(raw_gpu, wave):
    """Worst fbank error of every row in the power domain: |e - e64| over the frame's power scale (its spectral
    energy after the DC removal, or that of a one-ulp DC residue when larger: wespeaker_ref.fbank_raw), where
    e = exp(log-mel) of each (bin, frame).  A flat log-domain gate would fail near-silent frames whose f32 DC removal
    leaves a residue the float64 one does not; this measure stays fp32-grade for every frame."""
    want, scale = R.fbank_raw(wave)                                   # (N, T, 80), (N, T)
    got = raw_gpu.double().view(want.shape[0], 80, -1).permute(0, 2, 1)
    err = (got.exp() - want.exp()).abs() / scale[..., None]
    return err.reshape(err.shape[0], -1).amax(dim=1)


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
    errs, rows = {}, {}
    for i, name in enumerate(STAGES):
        g, frames = hip.peek(S, i)
        ref = want[name]
        assert g.numel() == ref.numel(), name
        if i <= 1:
            assert frames == T[0]
        elif i <= 5:
            assert frames == T[i - 1]
        errs[name] = rel(g.cpu().view(ref.shape), ref)
        rows[name] = rel_rows(g.cpu().view(ref.shape), ref)
    raw, frames = hip.peek(S, 7)
    assert frames == T[0]
    rows["fbank"] = fbank_error(raw.cpu(), x)
    errs["emb"] = rel(got, want["emb"])
    rows["emb"] = rel_rows(got, want["emb"])
    print(precision, S, Fw, {k: f"{v:.2e}" for k, v in errs.items()}, "cos", cos_min(got, want["emb"]))
    print("WSP-ROWS", precision, S, Fw, {k: f"{v.max().item():.3e}" for k, v in rows.items()})
    assert all(v <= 2e-4 for v in errs.values()), errs
    assert cos_min(got, want["emb"]) >= 0.99999
    bad = {k: v.max().item() for k, v in rows.items() if v.max().item() > ROW_GATES[precision][k]}
    assert not bad, bad


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


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", [1, 5, 8, 24, 32])
def test_batch_geometries_against_float64(gpu, state, oracle, precision, N):
    """1680-sample rows (9 -> 9 -> 5 -> 3 -> 2 frames) in batches whose GEMM heights N 80 9 (layer 1) and N 10 2 (layer
    4) end tiles at every residue the 80-multiple heights reach (N 8: 5760 = 15 x 384; N 24 / 32: layer 4 at 480 / 640
    rows, 0 mod 96 / 128), ragged elsewhere: every row of a batch against float64 with the per-row gates, so the bits
    test_batch_invariance shows equal are right too."""
    S = 1680
    hip = M.HipWeSpeakerEmbedding(state, max_batch=N, precision=precision).to(gpu)
    x = torch.from_numpy(synth_streams(N, 0.2, seed0=400 + N))[:, :S].contiguous()
    w = torch.rand(N, 7, generator=torch.Generator().manual_seed(N))
    got = hip(x[:, None].to(gpu), w.to(gpu)).cpu()
    want = oracle.stages(x, w)
    worst = {}
    for i, name in enumerate(STAGES):
        g, _ = hip.peek(S, i)
        worst[name] = rel_rows(g.cpu().view(want[name].shape), want[name]).max().item()
    worst["fbank"] = fbank_error(hip.peek(S, 7)[0].cpu(), x).max().item()
    worst["emb"] = rel_rows(got, want["emb"]).max().item()
    print("WSP-ROWS", precision, S, N, {k: f"{v:.3e}" for k, v in worst.items()})
    assert cos_min(got, want["emb"]) >= 0.99999
    bad = {k: v for k, v in worst.items() if v > ROW_GATES[precision][k]}
    assert not bad, bad


def pool64(x_cl, w):
    """float64 StatsPool (pyannote.audio 3.1) of channels-last layer-4 output (N, 10, T4, 256)."""
    return R.WeSpeakerRef.pool(x_cl.double().permute(0, 3, 1, 2), w)


def pool32(x_cl, w):
    """pyannote.audio 3.1's StatsPool._pool in torch float32, operation for operation (w: (N, T4), no resampling)."""
    N, Fq, T, C = x_cl.shape
    seq = x_cl.permute(0, 3, 1, 2).reshape(N, C * Fq, T)
    w = w.float().unsqueeze(1)
    v1 = w.sum(dim=2) + 1e-8
    mean = (seq * w).sum(dim=2) / v1
    dx2 = (seq - mean.unsqueeze(2)) ** 2
    v2 = (w ** 2).sum(dim=2)
    var = (dx2 * w).sum(dim=2) / (v1 - v2 / v1 + 1e-8)
    return torch.cat([mean, torch.sqrt(var)], dim=1)


def pool_weights(B, K, Fw, seed):
    """(B, K, Fw): random weights with an exact-zero stretch; the last speaker of each window is a 0/1 row (what
    min-max normalisation makes of a powerset decision), the first of window 0 is all zero."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(B, K, Fw, generator=g)
    w[:, :, : max(Fw // 4, 0)] = 0.0
    w[:, -1] = (torch.rand(B, Fw, generator=g) < 0.5).float()
    w[0, 0] = 0.0
    return w


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Fw,K", [("T4", 1), (21, 5), (1, 8), (293, 3), (589, 5)])
def test_pooling_on_the_models_own_layer4(gpu, hips, precision, Fw, K):
    """The pooling kernel alone: dz_wsp_forward_multi's pooled statistics (peek 6) against a float64 StatsPool of the
    GPU's own layer-4 output (peek 5), so trunk error does not hide pooling error.  Fw = T4 (no resampling), 21 < T4
    (upsampled), 1, 293, 589; K = 1, 5, 8; zero stretches, 0/1 rows and an all-zero row."""
    hip = hips[precision]
    S, B = 32000, 3
    T4 = hip.num_frames(S, 4)
    fw = T4 if Fw == "T4" else Fw
    x = torch.from_numpy(synth_streams(B, 2.01, seed0=500))[:, :S].contiguous().to(gpu)
    w = pool_weights(B, K, fw, seed=fw * 10 + K)
    out = hip.forward_multi(x[:, None], w.to(gpu)).cpu()
    l4, frames = hip.peek(S, 5)
    assert frames == T4
    l4 = l4.cpu().view(B, 10, T4, 256)
    pooled, _ = hip.peek(S, 6)
    pooled = pooled.cpu().view(B * K, 5120)
    want = pool64(l4.repeat_interleave(K, dim=0), w.reshape(B * K, fw))
    err = rel_rows(pooled, want)
    print("WSP-POOL", precision, Fw, K, f"{err.max().item():.3e}")
    assert torch.isfinite(out).all()
    assert err.max().item() <= POOL_GATE, err


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_nonzero_frame_matches_pyannote_float32(gpu, hips, precision):
    """A weight row with one non-zero frame of value w: the 3.1 denominator v1 - w^2 / v1 + 1e-8 is negative in float32
    for some w (tests/test_wespeaker_host.py shows which), so pyannote's own float32 arithmetic gives a NaN std there
    where float64 is finite.  The kernel follows pyannote's float32 operation for operation: NaN where it is NaN, the
    same bits where it is finite.  w = 1.0 (what min-max normalisation gives a lone frame) has std exactly 0."""
    hip = hips[precision]
    S, B, K = 32000, 2, 8
    T4 = hip.num_frames(S, 4)
    x = torch.from_numpy(synth_streams(B, 2.01, seed0=510))[:, :S].contiguous().to(gpu)
    # w = 1.0, then float32 values whose denominator is negative (NaN std) or positive, picked by the formula itself
    w32 = torch.linspace(0.2, 1.0, 4001)
    v1 = w32 + 1e-8
    neg = (v1 - w32 * w32 / v1 + 1e-8) < 0
    vals = torch.cat([torch.tensor([1.0]), w32[neg][:4], w32[~neg][1::997][:3]])
    w = torch.zeros(B, K, T4)
    for b in range(B):
        for k in range(K):
            w[b, k, (7 * k + 3 * b) % T4] = vals[k]
    hip.forward_multi(x[:, None], w.to(gpu))
    l4 = hip.peek(S, 5)[0].cpu().view(B, 10, T4, 256)
    got = hip.peek(S, 6)[0].cpu().view(B * K, 5120)
    want = pool32(l4.repeat_interleave(K, dim=0), w.reshape(B * K, T4))
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    print("WSP-SINGLE", precision, "NaN stds:", int(nan_w.sum()), "of", want.numel() // 2)
    assert nan_w.any(), "no float32 NaN among the single-frame rows: the case does not test the edge"
    assert torch.equal(nan_g, nan_w)
    assert torch.equal(got[~nan_g], want[~nan_w])
    one = torch.arange(B) * K                                            # the rows with w = 1.0
    assert torch.isfinite(got[one]).all() and (got[one][:, 2560:] == 0).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_degenerate_windows(gpu, state, oracle, precision):
    """Silence, DC, a zero-padded tail, near-silence, clipping, a click, a short burst (test_gpu_models.py's windows):
    finite embeddings, no range flag, the ordinary embedding gates, with and without weights."""
    from test_gpu_models import _degenerate_windows
    names, x = _degenerate_windows()
    n = len(names)
    hip = M.HipWeSpeakerEmbedding(state, max_batch=n, precision=precision).to(gpu)
    w = torch.rand(n, 3, 293, generator=torch.Generator().manual_seed(5)) ** 2 + 1e-8
    g0 = hip(x.to(gpu)).cpu()
    gm = hip.forward_multi(x.to(gpu), w.to(gpu)).cpu()
    _lib.range_check(gpu.index)
    assert torch.isfinite(g0).all() and torch.isfinite(gm).all()
    r0, rm = oracle.multi(x[:, 0]), oracle.multi(x[:, 0], w)
    for i, nm in enumerate(names):
        e0, em = rel(g0[i:i + 1], r0[i:i + 1]), rel(gm[i], rm[i])
        print("WSP-DEGENERATE", precision, nm, f"{e0:.2e} {em:.2e}")
        assert e0 <= 2e-4 and em <= 2e-4, (nm, e0, em)
        assert cos_min(g0[i:i + 1], r0[i:i + 1]) >= 0.99999 and cos_min(gm[i], rm[i]) >= 0.99999, nm


@pytest.mark.parametrize("precision", PRECISIONS)
def test_strided_views_and_handle_reuse(gpu, state, precision):
    """Rolling windows given as an unfold of one buffer (rows 8000 samples apart, addressed in place) give the bits of
    contiguous copies; after a call at max_batch, or at another length, a call with fewer rows gives the bits of a
    fresh model."""
    S, n = 32000, 5
    buf = torch.from_numpy(synth_streams(1, 4.6, seed0=520))[0].to(gpu)
    view = buf.unfold(0, S, 8000)[:n]
    assert view.stride() == (8000, 1) and view.data_ptr() == buf.data_ptr()
    copy = view.contiguous()
    w = torch.rand(n, 3, 293, generator=torch.Generator().manual_seed(6)).to(gpu)
    hip = M.HipWeSpeakerEmbedding(state, max_batch=n, precision=precision).to(gpu)
    assert torch.equal(hip(view[:, None]).cpu(), hip(copy[:, None]).cpu())
    assert torch.equal(hip.forward_multi(view[:, None], w).cpu(), hip.forward_multi(copy[:, None], w).cpu())
    fresh = M.HipWeSpeakerEmbedding(state, max_batch=n, precision=precision).to(gpu)
    want = fresh.forward_multi(copy[1:3, None], w[1:3]).cpu()
    want1 = fresh(copy[3:4, None], w[3:4, 0]).cpu()
    hip(copy[:, None], w[:, 0])                                      # max_batch rows
    assert torch.equal(hip.forward_multi(copy[1:3, None], w[1:3]).cpu(), want)
    hip(torch.from_numpy(synth_streams(n, 3.01, seed0=530))[:, :48000].contiguous().to(gpu)[:, None])  # another length
    assert torch.equal(hip(copy[3:4, None], w[3:4, 0]).cpu(), want1)
    assert torch.equal(hip.forward_multi(copy[1:3, None], w[1:3]).cpu(), want)


def test_range_flag_through_the_blocks_api(gpu, state):
    """A state whose first block's BatchNorm scale is 2e4: its activations pass 65504 (up to ~4e5).  The f16x3 blocks-API
    call raises through the range check; f32 stays within the float64 gates."""
    from diart_amd.blocks import SpeakerEmbedding
    sd = dict(state)
    sd["resnet.layer1.0.bn1.weight"] = state["resnet.layer1.0.bn1.weight"] * 2e4
    S = 32000
    x = torch.from_numpy(synth_streams(2, 2.01, seed0=540))[:, :S].contiguous()
    w = torch.rand(2, 293, 3, generator=torch.Generator().manual_seed(7))
    _lib.range_check(gpu.index)
    split = SpeakerEmbedding(M.EmbeddingModel.from_state(sd, max_batch=2, precision="f16x3"), device=gpu)
    with pytest.raises(_lib.DiartAmdError, match="65504"):
        split(x[:, :, None], w)
    exact = SpeakerEmbedding(M.EmbeddingModel.from_state(sd, max_batch=2, precision="f32"), device=gpu)
    got = exact(x[:, :, None], w)
    _lib.range_check(gpu.index)
    want = R.WeSpeakerRef(sd).multi(x, w.permute(0, 2, 1))
    assert got.shape == want.shape
    e = rel(got, want)
    print("WSP-RANGE f32", f"{e:.2e}", "cos", cos_min(got.reshape(6, -1), want.reshape(6, -1)))
    assert e <= 2e-4 and cos_min(got.reshape(6, -1), want.reshape(6, -1)) >= 0.99999


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
