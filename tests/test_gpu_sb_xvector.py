"""speechbrain x-vector (speechbrain/spkrec-xvect-voxceleb) on the GPU against the float64 restatement
(tests/sb_xvector_ref.py), in both arithmetic modes: stage by stage through dz_sbx_peek (fbank, TDNN 1 - 5, pooled
statistics, embedding) over the batch geometries the wrapper produces, the deviation the deterministic pooling noise
costs, forward_groups against single calls, and the whole pipeline (blocks API and N-stream engine).

Gates: relative L2 <= 2e-4 per stage (ECAPA's embedding gate), over the frames of each row's own geometry."""
import numpy as np
import pytest
import torch

import sb_xvector_ref as R
from diart_amd import models as M
from diart_amd.pipeline import GroupsBatch
from diart_amd.synth import synth_sb_xvector_state, synth_segmentation_state, synth_streams

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")
GATE = 2e-4
STAGES = ["feats", "tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5"]
WIDTH = {"feats": 24, "tdnn1": 512, "tdnn2": 512, "tdnn3": 512, "tdnn4": 512, "tdnn5": 1500}
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


def edge_spans():
    """Kept lengths at the relative-length rounding edges of a 5 s longest row (oracle.ecapa_ref.rounding_edges),
    plus the longest row itself, 480 (the shortest kept row) and 479 (too short)."""
    from oracle.ecapa_ref import rounding_edges
    e = rounding_edges(S5, lo=R.MIN_NUM_SAMPLES)
    lens = [S5] + e["half"][:2] + e["int"][:1] + e["near"][:2] + e["differs"][:2] + [480, 479]
    return [(0, L) for L in lens]


CASES = {
    "no_masks": lambda: (torch.from_numpy(synth_streams(3, 5.01, seed0=40))[:, :S5].contiguous(), None),
    "osp": lambda: (torch.from_numpy(synth_streams(3, 5.01, seed0=41))[:, :S5].contiguous(), osp_masks(3, 293, 1)),
    "edges": lambda: (torch.from_numpy(synth_streams(len(edge_spans()), 5.01, seed0=42))[:, :S5].contiguous(),
                      sample_masks(S5, edge_spans())),
}


@pytest.fixture(scope="module")
def state():
    return synth_sb_xvector_state()


@pytest.fixture(scope="module")
def oracle(state):
    return R.SbXvectorRef(state)


@pytest.fixture(scope="module")
def hips(gpu, state):
    return {p: M.HipSbXvectorEmbedding(state, max_batch=12, precision=p).to(gpu) for p in PRECISIONS}


def run_hip(hip, x, masks):
    S, N = x.shape[-1], x.shape[0]
    out = hip(x[:, None].to(hip.device), None if masks is None else masks.to(hip.device)).cpu()
    res = {"emb": out}
    for i, k in enumerate(STAGES):
        t, Tc = hip.peek(S, i)
        res[k] = t.cpu().view(N, Tc, WIDTH[k])
    res["pooled"] = hip.peek(S, 6)[0].cpu().view(N, 3000)
    for k, idx in (("lens", 7), ("nvalid", 8), ("T", 9)):
        res[k] = hip.peek(S, idx)[0].cpu().long()
    return res


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", list(CASES))
def test_stages_against_float64(gpu, hips, oracle, precision, case):
    x, masks = CASES[case]()
    got = run_hip(hips[precision], x, masks)
    geom = oracle.geometry(x[:, None].double(), masks)
    want = oracle.stages(geom)
    T = geom["T"]
    assert (got["T"] == T).all() and torch.equal(got["nvalid"], geom["nvalid"].long())
    assert torch.equal(got["lens"], geom["lens"].long())
    errs = {k: rel(got[k][:, :T], want[k]) for k in STAGES}
    errs["pooled"] = rel(got["pooled"], want["pooled"])
    ok = ~geom["too_short"]
    errs["emb"] = rel(got["emb"][ok], want["emb"][ok])
    print(precision, case, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= GATE for v in errs.values()), errs
    assert torch.isnan(got["emb"][~ok]).all() and torch.isfinite(got["emb"][ok]).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_short_and_nan_samples(gpu, hips, oracle, precision):
    hip = hips[precision]
    x = torch.from_numpy(synth_streams(4, 5.01, seed0=43))[:, :S5].contiguous()
    # every row keeps fewer than 480 samples: all NaN, and the geometry reports 0 frames
    out = hip(x[:, None].to(gpu), sample_masks(S5, [(0, 479), (100, 400), (0, 0), (5, 200)]).to(gpu)).cpu()
    assert torch.isnan(out).all()
    assert (hip.peek(S5, 9)[0].cpu() == 0).all()
    # a NaN / Inf where the mask drops the sample is never seen; where it keeps it, only that row is NaN
    masks = sample_masks(S5, [(0, S5), (0, 40000), (0, 40000), (20000, 60000)])
    base = hip(x[:, None].to(gpu), masks.to(gpu)).cpu()
    xb = x.clone()
    xb[1, 50000] = float("nan")        # dropped by row 1's mask
    xb[2, 30000] = float("inf")        # kept by row 2's mask
    got = hip(xb[:, None].to(gpu), masks.to(gpu)).cpu()
    assert torch.equal(got[[0, 1, 3]], base[[0, 1, 3]])
    assert torch.isnan(got[2]).all()
    want = oracle(xb[:, None].double(), masks)
    assert torch.isnan(want[2]).all() and rel(got[[0, 1, 3]], want[[0, 1, 3]]) <= GATE


def test_noise_deviation(gpu, hips, oracle):
    """speechbrain draws the mean's noise in [1e-5, 9e-5] on every call; this path adds the midpoint.  The reference's
    own run-to-run spread and the deviation of the midpoint from its random draws are measured and bounded."""
    x, masks = CASES["osp"]()
    geom = oracle.geometry(x[:, None].double(), masks)
    mid = oracle.stages(geom)["emb"]
    draws = [oracle.stages(geom, noise=torch.Generator().manual_seed(s))["emb"] for s in range(4)]
    dev_mid = max(rel(d, mid) for d in draws)
    dev_runs = max(rel(draws[i], draws[j]) for i in range(4) for j in range(i + 1, 4))
    got = hips["f32"](x[:, None].to(gpu), masks.to(gpu)).cpu()
    dev_hip = max(rel(got, d) for d in draws)
    print(f"noise: midpoint vs random band {dev_mid:.2e}, reference run to run {dev_runs:.2e}, "
          f"HIP (f32) vs random band {dev_hip:.2e}, HIP vs midpoint {rel(got, mid):.2e}")
    assert dev_mid <= 1e-4 and dev_runs <= 2e-4 and dev_hip <= GATE + dev_mid


# --------------------------------------------------------------------------- #
# forward_groups: each group is its own call
# --------------------------------------------------------------------------- #
def groups_inputs(G, K=3, Fw=589, seed=0):
    x = torch.from_numpy(synth_streams(G, 5.01, seed0=500 + seed))[:, :S5].contiguous()
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(G, K, Fw, generator=g) > 0.4).float()
    m[0, 1] = 0.0                                    # a silent speaker: too short -> NaN
    m[1, :, 100:] = 0.0                               # a group whose longest row is short
    m[1, 2, :] = 0.0
    m[1, 2, :5] = 1.0                                # ~680 samples: kept
    if G > 2:
        m[2, :, 3:] = 0.0                            # every row too short: an all-NaN group
    return x, m


@pytest.mark.parametrize("precision", PRECISIONS)
def test_groups_equal_single_calls(gpu, hips, oracle, precision):
    hip = hips[precision]
    G, K = 4, 3
    x, m = groups_inputs(G, K)
    out = hip.forward_groups(x[:, None].to(gpu), m.to(gpu)).cpu()
    Tg = hip.peek(S5, 9)[0].cpu().view(G, K)
    for g in range(G):
        single = hip(x[g:g + 1, None].repeat(K, 1, 1).to(gpu), m[g].to(gpu)).cpu()
        assert same_nan(out[g], single), (precision, g)
        assert (hip.peek(S5, 9)[0].cpu() == Tg[g]).all()
        want = oracle(x[g:g + 1, None].repeat(K, 1, 1).double(), m[g])
        ok = ~torch.isnan(want).any(dim=1)
        assert torch.equal(ok, ~torch.isnan(out[g]).any(dim=1))
        if ok.any():
            assert rel(out[g][ok], want[ok]) <= GATE
    assert torch.isnan(out[2]).all() and torch.isnan(out[0, 1]).all()
    # neighbours replaced: the other groups do not change
    x2, m2 = groups_inputs(G, K, seed=9)
    x3, m3 = x.clone(), m.clone()
    x3[0], m3[0], x3[3], m3[3] = x2[0], m2[0], x2[3], m2[3]
    out3 = hip.forward_groups(x3[:, None].to(gpu), m3.to(gpu)).cpu()
    assert same_nan(out3[1:3], out[1:3])
    normed = hip.forward_groups(x[:, None].to(gpu), m.to(gpu), normalize=True).cpu()
    ok = ~torch.isnan(out).any(dim=-1)
    assert torch.allclose(normed[ok], torch.nn.functional.normalize(out[ok], dim=-1), rtol=0, atol=1e-6)


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
    assert pending, "dz_sbx_forward_groups waited for work queued before it"
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
    assert type(M.EmbeddingLoader(state)()) is M.HipSbXvectorEmbedding
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
    print(f"sb-xvector ({'powerset' if powerset else 'multilabel'}): DER(GPU vs CPU chain on the GPU's segmentation) = "
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
                       M.HipSbXvectorEmbedding(emb_sd, precision=precision), n, tau_active=0.5,
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
    n, steps = 3, 8
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
            r = remb.reshape(-1, 512).numpy()
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
                       M.HipSbXvectorEmbedding(emb_sd, precision=precision), n, tau_active=0.5,
                       normalize_embedding_weights=True, device=gpu)
    assert pipe.depth == 2
    for t, slots in enumerate((None, None, [2, 0])):
        windows = audio[:, t * HOP:t * HOP + W] if slots is None else audio[slots, t * HOP:t * HOP + W]
        ticket = pipe.launch(windows, slots=slots)
        pipe.finish(ticket)
        rows = len(windows)
        want = pipe.emb.forward_groups(windows[:, None], ticket["w"][:rows], normalize=True)
        assert want.shape == (rows, 3, 512)
        assert same_nan(ticket["emb"][:rows], want), (precision, t, slots)


def test_stream_server_equals_dedicated_pipelines(gpu, states):
    from diart_amd.inference import StreamingInference
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = states
    lengths = {"ana": 8.0, "ben": 7.0}
    audio = {k: synth_streams(1, v, seed0=980 + i)[0] for i, (k, v) in enumerate(lengths.items())}
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=2, powerset=True),
                       M.HipSbXvectorEmbedding(emb_sd), max_streams=2, tau_active=0.5,
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
