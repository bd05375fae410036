"""speechbrain ResNet (speechbrain/spkrec-resnet-voxceleb) on the GPU against the float64 restatement
(tests/sb_resnet_ref.py), in both arithmetic modes: stage by stage through dz_sbr_peek (fbank, stem, layers 1 - 4,
pooled statistics, embedding) over the batch geometries the wrapper produces, forward_groups against single calls and
across pass boundaries, and the whole pipeline (blocks API, N-stream engine, StreamServer).

The stage tests run a narrow synthetic state (widths 32 / 32 / 64 / 64, blocks 2 / 1 / 1 / 1: an identity-shortcut
block, strided blocks with and without a width change, every kernel instance class) on rows of 0.3 - 1.3 s, whose
frame counts are odd and even at each stride (131 -> 66 -> 33 -> 17 and 122 -> 61 -> 31 -> 16); the full width
(128 / 128 / 256 / 256) runs once, on 2 rows of at most 1 s.

Gates: relative L2 per stage against the float64 restatement over each row's own frames, about 3x the worst measured
on an MI355X (DESIGN.md 4.14 holds the table): GATES below."""
import numpy as np
import pytest
import torch

import sb_resnet_ref as R
from diart_amd import models as M
from diart_amd.pipeline import GroupsBatch
from diart_amd.synth import synth_sb_resnet_state, synth_segmentation_state, synth_streams

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")
NARROW = dict(channels=(32, 32, 64, 64), block_sizes=(2, 1, 1, 1))
STAGES = ["feats", "stem", "layer1", "layer2", "layer3", "layer4", "pooled", "emb"]
# worst measured over the cases below, f16x3 / f32: feats 1.29e-6 / 1.29e-6, stem 1.42e-6 / 1.42e-6,
# layer1 1.32e-6 / 1.32e-6, layer2 1.41e-6 / 1.42e-6, layer3 1.28e-6 / 1.30e-6, layer4 1.27e-6 / 1.26e-6, pooled
# 6.2e-7 / 6.7e-7, emb 7.1e-7 / 7.6e-7.  The trunk's figures are the features' (the STFT's float32 against float64, which
# the sentence mean then makes relative to a smaller norm): no layer adds to them.
GATES = {"feats": 4e-6, "stem": 4.5e-6, "layer1": 4e-6, "layer2": 4.5e-6, "layer3": 4e-6, "layer4": 4e-6, "pooled": 2e-6,
         "emb": 2.3e-6}
GATE = GATES["emb"]
S13 = 20800          # 1.3 s: Tc = 131
S5 = 80000


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def same_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def sample_masks(S, spans):
    """Per-sample masks (mask_frames = S: nearest resampling is the identity): row i keeps [a, b)."""
    m = torch.zeros(len(spans), S)
    for i, (a, b) in enumerate(spans):
        m[i, a:b] = 1.0
    return m


def osp_masks(n, Fw, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(n, Fw, generator=g)
    w[0, : Fw // 3] = 0.0
    w[-1, Fw // 2:] = 0.1
    return w


def edge_spans(lmax=19360, lo=4800):
    """Kept lengths at the relative-length rounding edges (oracle.ecapa_ref.rounding_edges) of a batch whose longest row
    keeps 19360 samples (T_g = 122, even, below the handle's 131), plus that row, 0.3 s, and 2 samples (too short)."""
    from oracle.ecapa_ref import rounding_edges
    e = rounding_edges(lmax, lo=lo)
    lens = [lmax] + e["half"][:2] + e["int"][:1] + e["near"][:2] + e["differs"][:2] + [lo, 2]
    return [(0, L) for L in lens]


def waves(n, S, seed):
    return torch.from_numpy(synth_streams(n, S / 16000.0 + 0.01, seed0=seed))[:, :S].contiguous()


CASES = {
    "no_masks": lambda: (waves(3, S13, 40), None),
    "osp": lambda: (waves(3, S13, 41), osp_masks(3, 77, 1)),
    "edges": lambda: (waves(len(edge_spans()), S13, 42), sample_masks(S13, edge_spans())),
}


@pytest.fixture(scope="module")
def state():
    return synth_sb_resnet_state(**NARROW)


@pytest.fixture(scope="module")
def oracle(state):
    return R.SbResNetRef(state)


@pytest.fixture(scope="module")
def hips(gpu, state):
    return {p: M.HipSbResNetEmbedding(state, max_batch=12, precision=p).to(gpu) for p in PRECISIONS}


def run_hip(hip, x, masks):
    """One forward and every stage peek offers, trimmed to nothing: the buffers' own layouts."""
    S, N = x.shape[-1], x.shape[0]
    out = hip(x[:, None].to(hip.device), None if masks is None else masks.to(hip.device)).cpu()
    shape = hip._packed.shape
    res = {"emb": out}
    t, Tc = hip.peek(S, 0)
    res["feats"] = t.cpu().view(N, Tc, 80)
    widths = (shape["stem"],) + shape["channels"]
    F = 80
    for l, k in enumerate(["stem", "layer1", "layer2", "layer3", "layer4"]):
        if l:
            F = (F - 1) // shape["strides"][l - 1] + 1
        t, Tl = hip.peek(S, 1 + l)
        res[k] = t.cpu().view(N, Tl, F, widths[l])
    res["pooled"] = hip.peek(S, 6)[0].cpu().view(N, -1)
    res["lens"] = hip.peek(S, 7)[0].cpu().long()
    res["T"] = hip.peek(S, 8)[0].cpu().long()
    res["ext"] = hip.peek(S, 9)[0].cpu().long().view(5, N)
    return res


def stage_errors(got, want, geom, oracle_, shape):
    """Relative L2 per stage over the rows' own frames; the frames behind them must hold +0.0."""
    T = R.frames(geom["T"], shape["strides"])
    assert (got["T"] == geom["T"]).all() and torch.equal(got["lens"], geom["lens"].long())
    assert all((got["ext"][l] == T[l]).all() for l in range(5))
    errs = {"feats": rel(got["feats"][:, :T[0]], want["feats"])}
    for l, k in enumerate(["stem", "layer1", "layer2", "layer3", "layer4"]):
        errs[k] = rel(got[k][:, :T[l]], want[k])
        assert (got[k][:, T[l]:].view(torch.int32) == 0).all(), f"{k}: a frame at or past {T[l]} is not +0.0"
    errs["pooled"] = rel(got["pooled"], oracle_.device_order(want["pooled"], shape["channels"][3], shape["freq"]))
    ok = ~geom["too_short"]
    errs["emb"] = rel(got["emb"][ok], want["emb"][ok])
    assert torch.isnan(got["emb"][~ok]).all() and torch.isfinite(got["emb"][ok]).all()
    return errs


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_stages_against_float64(gpu, hips, oracle, precision, case):
    x, masks = CASES[case]()
    hip = hips[precision]
    got = run_hip(hip, x, masks)
    geom = oracle.geometry(x[:, None].double(), masks)
    errs = stage_errors(got, oracle.stages(geom), geom, oracle, hip._packed.shape)
    print("SBR-STAGES", precision, case, "T", geom["T"], {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(errs[k] <= GATES[k] for k in STAGES), errs


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stages_at_full_width(gpu, precision):
    """128 / 128 / 256 / 256 channels (the 128 x 128 split tile, BN = 128 in exact f32, 2560 pooled channels), one block
    per layer, 2 rows of 1 s and 0.6 s."""
    sd = synth_sb_resnet_state(block_sizes=(1, 1, 1, 1), seed=77)
    hip = M.HipSbResNetEmbedding(sd, max_batch=2, precision=precision).to(gpu)
    ref = R.SbResNetRef(sd)
    x, masks = waves(2, 16000, 44), sample_masks(16000, [(0, 16000), (3000, 12600)])
    got = run_hip(hip, x, masks)
    geom = ref.geometry(x[:, None].double(), masks)
    errs = stage_errors(got, ref.stages(geom), geom, ref, hip._packed.shape)
    print("SBR-STAGES-FULL", precision, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(errs[k] <= GATES[k] for k in STAGES), errs


@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_short_and_nan_samples(gpu, state, oracle, precision):
    hip = M.HipSbResNetEmbedding(state, max_batch=4, precision=precision, min_num_samples=480).to(gpu)
    ref = R.SbResNetRef(state, min_samples=480)
    x = waves(4, S13, 43)
    # every row keeps fewer than min_num_samples samples: all NaN, and the geometry reports 0 frames
    out = hip(x[:, None].to(gpu), sample_masks(S13, [(0, 479), (100, 400), (0, 0), (5, 200)]).to(gpu)).cpu()
    assert torch.isnan(out).all()
    assert (hip.peek(S13, 8)[0].cpu() == 0).all()
    # a NaN / Inf where the mask drops the sample is never seen; where it keeps it, only that row is NaN
    masks = sample_masks(S13, [(0, S13), (0, 10000), (0, 10000), (5000, 15000)])
    base = hip(x[:, None].to(gpu), masks.to(gpu)).cpu()
    xb = x.clone()
    xb[1, 12000] = float("nan")        # dropped by row 1's mask
    xb[2, 7000] = float("inf")         # kept by row 2's mask
    got = hip(xb[:, None].to(gpu), masks.to(gpu)).cpu()
    assert torch.equal(got[[0, 1, 3]], base[[0, 1, 3]])
    assert torch.isnan(got[2]).all()
    want = ref(xb[:, None].double(), masks)
    assert torch.isnan(want[2]).all() and rel(got[[0, 1, 3]], want[[0, 1, 3]]) <= GATE
    # one too-short row beside kept ones
    masks = sample_masks(S13, [(0, S13), (0, 479), (0, 480), (0, 10000)])
    got, want = hip(x[:, None].to(gpu), masks.to(gpu)).cpu(), ref(x[:, None].double(), masks)
    assert torch.isnan(got[1]).all() and torch.isnan(want[1]).all() and rel(got[[0, 2, 3]], want[[0, 2, 3]]) <= GATE


# --------------------------------------------------------------------------- #
# forward_groups: each group is its own call
# --------------------------------------------------------------------------- #
def groups_inputs(G, K=3, Fw=77, seed=0, S=S13):
    x = waves(G, S, 500 + seed)
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(G, K, Fw, generator=g) > 0.4).float()
    m[0, 1] = 0.0                                    # a silent speaker: too short -> NaN
    m[1, :, 30:] = 0.0                               # a group whose longest row is short
    m[1, 2, :] = 0.0
    m[1, 2, :5] = 1.0
    if G > 2:
        m[2] = 0.0                                   # every row too short: an all-NaN group
    return x, m


@pytest.mark.parametrize("precision", PRECISIONS)
def test_groups_equal_single_calls(gpu, hips, oracle, precision):
    hip = hips[precision]
    G, K = 4, 3
    x, m = groups_inputs(G, K)
    out = hip.forward_groups(x[:, None].to(gpu), m.to(gpu)).cpu()
    Tg = hip.peek(S13, 8)[0].cpu().view(G, K)
    for g in range(G):
        single = hip(x[g:g + 1, None].repeat(K, 1, 1).to(gpu), m[g].to(gpu)).cpu()
        assert same_nan(out[g], single), (precision, g)
        assert (hip.peek(S13, 8)[0].cpu() == Tg[g]).all()
        want = oracle(x[g:g + 1, None].repeat(K, 1, 1).double(), m[g])
        ok = ~torch.isnan(want).any(dim=1)
        assert torch.equal(ok, ~torch.isnan(out[g]).any(dim=1))
        if ok.any():
            assert rel(out[g][ok], want[ok]) <= GATE
    assert torch.isnan(out[2]).all() and torch.isnan(out[0, 1]).all()
    assert len(set(Tg[:, 0].tolist())) >= 3            # the groups have frame counts of their own
    # neighbours replaced: the other groups do not change
    x2, m2 = groups_inputs(G, K, seed=9)
    x3, m3 = x.clone(), m.clone()
    x3[0], m3[0], x3[3], m3[3] = x2[0], m2[0], x2[3], m2[3]
    out3 = hip.forward_groups(x3[:, None].to(gpu), m3.to(gpu)).cpu()
    assert same_nan(out3[1:3], out[1:3])
    normed = hip.forward_groups(x[:, None].to(gpu), m.to(gpu), normalize=True).cpu()
    ok = ~torch.isnan(out).any(dim=-1)
    assert torch.allclose(normed[ok], torch.nn.functional.normalize(out[ok], dim=-1), rtol=0, atol=1e-6)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_result_does_not_depend_on_rows_per_pass(gpu, state, hips, precision):
    """7 rows of one call, and 3 groups of 3 rows, in passes of 2 rows (a pass boundary falls inside a group) against the
    default's single pass: the same bits."""
    x = waves(7, S13, 600)
    masks = sample_masks(S13, [(0, S13), (0, 4800), (100, 9000), (0, 19360), (7, 12345), (0, 2), (3000, 20000)])
    small = M.HipSbResNetEmbedding(state, max_batch=12, precision=precision, rows_per_pass=2).to(gpu)
    a = small(x[:, None].to(gpu), masks.to(gpu)).cpu()
    b = hips[precision](x[:, None].to(gpu), masks.to(gpu)).cpu()
    assert same_nan(a, b) and torch.isnan(a[5]).all() and torch.isfinite(a[[0, 1, 2, 3, 4, 6]]).all()
    xg, mg = groups_inputs(3, 3, seed=4)                # 9 rows: pass boundaries inside every group
    a = small.forward_groups(xg[:, None].to(gpu), mg.to(gpu)).cpu()
    b = hips[precision].forward_groups(xg[:, None].to(gpu), mg.to(gpu)).cpu()
    assert same_nan(a, b)


def test_forward_groups_does_not_wait_for_the_gpu(gpu, hips):
    hip = hips["f16x3"]
    x, m = groups_inputs(2)
    want = hip.forward_groups(x[:, None].to(gpu), m.to(gpu)).cpu()
    cyc = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cyc)
    b.record()
    b.synchronize()
    cycles = int(cyc * 300.0 / max(a.elapsed_time(b), 1e-3))
    xd, md = x[:, None].to(gpu), m.to(gpu)
    torch.cuda.synchronize(gpu)
    torch.cuda._sleep(cycles)
    ev = torch.cuda.Event()
    ev.record()
    out = hip.forward_groups(xd, md)
    pending = not ev.query()
    torch.cuda.synchronize(gpu)
    assert pending, "dz_sbr_forward_groups waited for work queued before it"
    assert same_nan(out.cpu(), want)


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
    from diart_amd.synth import synth_stream
    from test_gpu_der import accumulate, rolling_chunks
    stream = synth_stream(31, 12.0)
    seg_sd = synth_segmentation_state(seed=77, powerset=True) if powerset else synth_segmentation_state()
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=16, powerset=powerset),
        embedding=M.EmbeddingModel.from_state(state, max_batch=48), latency=0.5, tau_active=0.5,
        normalize_embedding_weights=powerset, device=gpu)
    assert type(M.EmbeddingLoader(state)()) is M.HipSbResNetEmbedding
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
        rows = x.repeat(1, 3, 1).reshape(B * 3, 1, -1).double()
        return normalize_embeddings_ref(oracle(rows, w.permute(0, 2, 1).reshape(B * 3, -1)).float().view(B, 3, -1))

    for i0 in range(0, len(chunks), 8):
        batch = chunks[i0:i0 + 8]
        x = torch.from_numpy(np.stack([c.data[:, 0] for c in batch]))[:, None, :]
        with torch.no_grad():
            out = seg_m(x)
        seg = cfg.segmentation(x.to(gpu)).cpu()
        if powerset:
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
    print(f"sb-resnet ({'powerset' if powerset else 'multilabel'}): DER(GPU vs CPU chain on the GPU's segmentation) = "
          f"{100 * d['diarization error rate']:.3f} % of {d['total']:.1f} s; DER(vs independent CPU chain) = "
          f"{100 * di['diarization error rate']:.3f} % (budget {100 * budget:.3f} %); {flips} flips at {near_ties} near ties")
    assert d["total"] > 1.0 and d["diarization error rate"] <= 0.005
    assert di["total"] > 1.0 and di["diarization error rate"] <= budget


# --------------------------------------------------------------------------- #
# the N-stream engine: StreamBatch and StreamServer against each stream's own pipeline at batch 1
# --------------------------------------------------------------------------- #
W, HOP = 80000, 8000


def engine(states, n, precision, gpu, **kw):
    from diart_amd.pipeline import StreamBatch
    seg_sd, emb_sd = states
    return StreamBatch(M.HipSegmentation(seg_sd, max_batch=n, powerset=True, precision=precision),
                       M.HipSbResNetEmbedding(emb_sd, precision=precision), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu, **kw)


def blocks_pipeline(states, precision, gpu):
    from diart_amd.blocks import SpeakerDiarization, SpeakerDiarizationConfig
    seg_sd, emb_sd = states
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=1, powerset=True, precision=precision),
        embedding=M.EmbeddingModel.from_state(emb_sd, max_batch=3, precision=precision),
        latency=0.5, tau_active=0.5, normalize_embedding_weights=True, device=gpu)
    return SpeakerDiarization(cfg)


@pytest.fixture(scope="module")
def states(state):
    return synth_segmentation_state(seed=77, powerset=True), state


def tracks(ann):
    return sorted((s.start, s.end, str(lab)) for s, _, lab in ann.itertracks(yield_label=True))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_engine_equals_per_stream_pipelines(gpu, states, precision):
    from diart_amd.blocks.aggregation import BatchedOutputTail
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    n, steps = 4, 6
    audio = synth_streams(n, (W + HOP * steps) / 16000.0, seed0=960)
    d_audio = torch.from_numpy(audio).to(gpu)
    pipe = engine(states, n, precision, gpu, tail=True)
    assert pipe.depth == 2 and isinstance(pipe, GroupsBatch)
    refs = [blocks_pipeline(states, precision, gpu) for _ in range(n)]
    worst = 0.0
    for t in range(steps):
        ticket = pipe.launch(d_audio[:, t * HOP:t * HOP + W])
        seg, emb, _, _ = pipe.finish(ticket, want_scores=False)
        emb = emb.copy()
        _, _, _, _, turns, nturns = ticket["tail"]
        for i in range(n):
            c = SlidingWindowFeature(audio[i][t * HOP:t * HOP + W, None],
                                     SlidingWindow(start=t * 0.5, duration=1 / 16000, step=1 / 16000))
            batch = torch.from_numpy(c.data)[None]
            rseg = refs[i].segmentation(batch)
            remb = refs[i].embedding(batch, rseg)
            want = refs[i].finalise([c], rseg, remb)[0][0]
            r = remb.reshape(-1, 256).numpy()
            assert np.array_equal(np.isnan(emb[i]), np.isnan(r)), (precision, t, i)
            ok = ~np.isnan(r).any(axis=1)
            d = np.abs(emb[i][ok] - r[ok]).max(initial=0.0)
            worst = max(worst, d)
            assert d <= 1e-6, (precision, t, i)
            got = BatchedOutputTail.annotation(turns[i], int(nturns[i]))
            assert tracks(got) == tracks(want), (precision, t, i)
    print(f"{precision}: engine vs per-stream embeddings, max |diff| {worst:.2e}")
    with pytest.raises(ValueError):
        engine(states, n, precision, gpu, emb_split=2)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_engine_adds_nothing_to_the_model_s_own_forward(gpu, states, precision):
    """The groups-form counterpart of WeSpeaker's halves-equal-the-whole test: a ``GroupsBatch`` of 3 streams, two full
    steps (one on each lane) and one ``slots=[2, 0]`` step (fewer rows than streams, on the first lane again).  After
    ``finish`` the step's device embeddings equal the model's own ``forward_groups`` on the same windows and the step's
    own OSP weights bit for bit, NaN rows included: the engine's schedule adds nothing to the forward."""
    n = 3
    seg_sd, emb_sd = states
    audio = torch.from_numpy(synth_streams(n, (W + 3 * HOP) / 16000.0, seed0=965)).to(gpu)
    pipe = GroupsBatch(M.HipSegmentation(seg_sd, max_batch=n, powerset=True, precision=precision),
                       M.HipSbResNetEmbedding(emb_sd, precision=precision), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu)
    assert pipe.depth == 2
    for t, slots in enumerate((None, None, [2, 0])):
        windows = audio[:, t * HOP:t * HOP + W] if slots is None else audio[slots, t * HOP:t * HOP + W]
        ticket = pipe.launch(windows, slots=slots)
        pipe.finish(ticket)
        rows = len(windows)
        want = pipe.emb.forward_groups(windows[:, None], ticket["w"][:rows], normalize=True)
        assert want.shape == (rows, 3, 256)
        assert same_nan(ticket["emb"][:rows], want), (precision, t, slots)


def test_stream_server_equals_dedicated_pipelines(gpu, states):
    from diart_amd.inference import StreamingInference
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = states
    lengths = {"ana": 8.0, "ben": 7.0}
    audio = {k: synth_streams(1, v, seed0=980 + i)[0] for i, (k, v) in enumerate(lengths.items())}
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=2, powerset=True),
                       M.HipSbResNetEmbedding(emb_sd), max_streams=2, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu)
    assert isinstance(srv.batch, GroupsBatch)
    rng = np.random.default_rng(6)
    pos = {k: 0 for k in audio}
    join_at = {"ana": 0, "ben": 2}
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
    assert max(widths) >= 2
    for k in audio:
        got = srv.close(k)
        usable = len(audio[k]) // HOP * HOP
        want = StreamingInference(blocks_pipeline(states, M.default_precision(), gpu), audio[k][:usable], 16000, k,
                                  (0, 0), 1)()
        assert want is not None and got.to_rttm() == want.to_rttm(), k
