"""Config 3 embedding (ECAPA-TDNN) across the batch geometries the pipeline produces: the HIP path stage by stage
against the float64 restatement (oracle/ecapa_ref.py with ``dtype=torch.float64``, which keeps the reference's
float32 length arithmetic), gated per row in both precisions.

The geometry of a call is data-dependent: T = 1 + lmax // 160 for the longest kept row, and N T decides where the
128-row tiles of the split-f16 GEMMs end.  The frame counts each row's relative length selects (peek 6 nvalid:
sentence mean; peek 7 nmask: squeeze-excitation mean and attentive pooling) are asserted exactly.  Frame-wise stages
are compared on all T frames (the reference runs the network over the padding too), the attention logits on the
frames the softmax sees.

Gates: relative L2 per row against float64, set at about twice the worst row measured on an MI355X over every case
and both precisions (features 1.0e-5, block 0 8.2e-6, MFA 9.6e-6, logits 2.0e-6, pooled 3.4e-6, embeddings
1.5e-6 with 1 - cosine 1.0e-12).  None is looser than the whole-tensor gates of test_gpu_ecapa.py (2e-5 features
and block 0, 1e-4 MFA and pooled, 2e-4 and cosine >= 0.99999 embeddings)."""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.synth import synth_ecapa_state, synth_streams

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16x3", "f32")
MAX_ROWS = 96                   # bench.py --config 3: 32 chunks x 3 speakers
GATES = {"feats": 2e-5, "block0": 2e-5, "mfa": 2e-5, "logits": 1e-5, "pooled": 1e-5, "emb": 1e-5}
COS_GATE = 1e-10                # 1 - cosine of the embeddings
PEEK = {"feats": (0, 80), "block0": (1, 1024), "logits": (2, 3072), "mfa": (3, 3072)}
CHUNK = 8                       # rows of float64 network per step


@pytest.fixture(scope="module")
def state():
    return synth_ecapa_state()


@pytest.fixture(scope="module")
def o64(state):
    from oracle.ecapa_ref import PretrainedSpeakerEmbeddingRef
    return PretrainedSpeakerEmbeddingRef(state, dtype=torch.float64)


@pytest.fixture(scope="module")
def hips(gpu, state):
    return {p: M.HipEcapaEmbedding(state, max_batch=MAX_ROWS, precision=p).to(gpu) for p in PRECISIONS}


def sample_masks(S, spans):
    """Per-sample masks (mask_frames = S: the nearest resampling is the identity): row i keeps [a, b)."""
    m = torch.zeros(len(spans), S)
    for i, (a, b) in enumerate(spans):
        m[i, a:b] = 1.0
    return m


def run_hip(hip, x, masks):
    """Forward + every intermediate of it (CPU copies)."""
    S = x.shape[-1]
    out = hip(x.to(hip.device), None if masks is None else masks.to(hip.device)).cpu()
    N = x.shape[0]
    res = {"emb": out}
    _, T = hip.peek(S, 5)
    for k, (idx, c) in PEEK.items():
        res[k] = hip.peek(S, idx)[0].cpu().view(N, T, c)
    res["pooled"] = hip.peek(S, 4)[0].cpu().view(N, 6144)
    for k, idx in (("lens", 5), ("nvalid", 6), ("nmask", 7)):
        res[k] = hip.peek(S, idx)[0].cpu().long()
    res["T"] = T
    return res


def row_errors(got, ref, stage, nmask, ok):
    """Relative L2 per row (rows with ok False -> 0).  Features are in dB and computed from values down to the
    -100 dB of the 1e-10 clamp, where one float32 ulp is 7.6e-6 dB: a row's feature error is taken relative to
    its RMS but to no less than 1 dB RMS (a quiet row sits on the clamp almost everywhere, so the sentence mean
    leaves it close to zero: 0.05 dB RMS at 1e-6 full scale, exactly zero for an all-zero kept region)."""
    a, b = got.double(), ref.double()
    if stage == "logits":
        keep = (torch.arange(b.shape[1])[None, :, None] < nmask[:, None, None]).double()
        a, b = a * keep, b * keep
    a, b = a.flatten(1), b.flatten(1)
    num = (a - b).norm(dim=1)
    den = b.norm(dim=1)
    if stage == "feats":
        den = den.clamp_min(b.shape[1] ** 0.5)
    e = num / den.clamp_min(1e-30)
    return torch.where(ok, e, torch.zeros_like(e))


def check_case(name, x, masks, o64, hips, bad_rows=()):
    """Run both precisions, compare every stage per row with the float64 oracle, assert the gates; returns
    {precision: {stage: worst row}} (printed for the record)."""
    x = x.contiguous()
    geom = o64.geometry(x, masks)
    N, T = x.shape[0], geom["T"]
    bad = torch.zeros(N, dtype=torch.bool)
    bad[list(bad_rows)] = True
    runs = {p: run_hip(hips[p], x, masks) for p in PRECISIONS}
    want_lens = torch.where(bad, -(geom["lens"] + 1), geom["lens"])
    for p, r in runs.items():
        assert r["T"] == T, (p, r["T"], T)
        assert torch.equal(r["lens"], want_lens), p
        assert torch.equal(r["nvalid"], geom["nvalid"]), (p, (r["nvalid"] - geom["nvalid"]).nonzero().flatten())
        assert torch.equal(r["nmask"], geom["nmask"]), (p, (r["nmask"] - geom["nmask"]).nonzero().flatten())
    errs = {p: {k: torch.zeros(N, dtype=torch.float64) for k in GATES} for p in PRECISIONS}
    cos = {p: torch.ones(N, dtype=torch.float64) for p in PRECISIONS}
    nan_rows = geom["too_short"] | bad
    for r0 in range(0, N, CHUNK):
        rows = slice(r0, min(N, r0 + CHUNK))
        ref = o64.stages(geom, rows)
        ok = ~bad[rows]                                  # a kept NaN sample: the reference's stages are NaN
        emb_ok = ~nan_rows[rows]
        for p, r in runs.items():
            for k in GATES:
                e = row_errors(r[k][rows], ref[k], k, geom["nmask"][rows], emb_ok if k == "emb" else ok)
                errs[p][k][rows] = e
            c = torch.nn.functional.cosine_similarity(r["emb"][rows].double(), ref["emb"], dim=-1)
            cos[p][rows] = torch.where(emb_ok, c, torch.ones_like(c))
    worst = {}
    for p, r in runs.items():
        assert torch.equal(torch.isnan(r["emb"]).all(dim=1), nan_rows), p
        assert not torch.isnan(r["emb"][~nan_rows]).any(), p
        worst[p] = {k: errs[p][k].max().item() for k in GATES}
        worst[p]["1-cos"] = 1.0 - cos[p].min().item()
        print(f"{name} N={N} T={T} NT%128={N * T % 128} {p}: " + " ".join(f"{k} {v:.2e}" for k, v in worst[p].items()))
    for p in PRECISIONS:
        for k, tol in GATES.items():
            assert worst[p][k] < tol, (name, p, k, worst[p][k], int(errs[p][k].argmax()))
        assert worst[p]["1-cos"] < COS_GATE, (name, p, worst[p]["1-cos"])
    return worst


# --------------------------------------------------------------------------- #
# a. rounding edges of the relative lengths
# --------------------------------------------------------------------------- #
def test_length_rounding_edges(o64, hips):
    """Kept lengths where float32(len / lmax) * T lands on an integer, on k + 0.5, within an ulp of either, and where
    float32 rounding differs from exact rational rounding, in one batch whose longest row is lmax = 62340."""
    from oracle.ecapa_ref import rounding_edges
    S, lmax = 80000, 62340
    e = rounding_edges(lmax)
    lens = [lmax]
    for k, n in (("differs", 5), ("int", 4), ("half", 4), ("near", 4)):
        lens += [v for v in e[k] if v not in lens][:n]
    assert set(e["differs"][:5]) <= set(lens) and len(lens) == 18
    x = torch.from_numpy(synth_streams(len(lens), S / 16000, seed0=300))[:, None, :S]
    spans = [((i * 997) % (S - n + 1), (i * 997) % (S - n + 1) + n) for i, n in enumerate(lens)]
    check_case("edges", x, sample_masks(S, spans), o64, hips)


# --------------------------------------------------------------------------- #
# b. geometry sweep: T at its minimum, N T mod 128 in {0, 1, 127, ...}, N from 1 to 96
# --------------------------------------------------------------------------- #
SWEEP = [  # (N, lmax): T = 1 + lmax // 160
    (1, 640),        # T 5, NT 5: the smallest legal geometry
    (7, 799),        # T 5, NT 35
    (96, 640),       # T 5, NT 480 = 96 mod 128
    (33, 800),       # T 6, NT 198 = 70
    (64, 959),       # T 6, NT 384 = 0
    (7, 8640),       # T 55, NT 385 = 1
    (33, 4800),      # T 31, NT 1023 = 127 (+ a kept NaN sample)
    (65, 10240),     # T 65, NT 4225 = 1
    (96, 1120),      # T 8, NT 768 = 0
    (96, 20320),     # T 128, NT 12288 = 0
]


@pytest.mark.parametrize("N,lmax", SWEEP, ids=[f"N{n}-T{1 + l // 160}" for n, l in SWEEP])
def test_geometry_sweep(o64, hips, N, lmax):
    S = lmax + 37
    g = torch.Generator().manual_seed(N * 100003 + lmax)
    x = torch.from_numpy(synth_streams(N, S / 16000 + 0.01, seed0=400 + N))[:, None, :S].clone()
    lens = torch.randint(640, lmax + 1, (N,), generator=g)
    lens[0] = lmax
    if N >= 7:
        lens[1:3] = torch.randint(1, 640, (2,), generator=g)      # too short: NaN rows with rel = 1
        lens[3] = 640
    spans = []
    for n in lens.tolist():
        a = int(torch.randint(0, S - n + 1, (1,), generator=g))
        spans.append((a, a + n))
    bad = ()
    if N == 33:
        a, b = spans[5]
        x[5, 0, (a + b) // 2] = float("nan")                      # kept: the row's embedding is NaN
        bad = (5,)
    check_case(f"sweep N={N} lmax={lmax}", x, sample_masks(S, spans), o64, hips, bad_rows=bad)


# --------------------------------------------------------------------------- #
# c. the product's own shape: 32 chunks x 3 speakers of 5 s, masks from OSP weights
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("chunks,Fw", [(32, 293), (16, 589)])
def test_product_shape_osp_masks(o64, hips, chunks, Fw):
    """The SpeakerEmbedding path: the chunk's waveform once per speaker, masks = min-max normalised OSP weights
    (as test_gpu_ecapa.py::test_operator_api_with_ecapa), nearest-resampled from Fw frames to 80000 samples."""
    from oracle.functional_ref import overlapped_speech_penalty_ref
    S = 80000
    wav = torch.from_numpy(synth_streams(chunks, 5.0, seed0=500))[:, :S]
    g = torch.Generator().manual_seed(Fw)
    seg = torch.rand(chunks, Fw, 3, generator=g)
    seg[:, :, 2] *= 0.05                                          # a mostly silent third speaker
    w = overlapped_speech_penalty_ref(seg)
    mn, mx = w.min(dim=1, keepdim=True).values, w.max(dim=1, keepdim=True).values
    w = ((w - mn) / (mx - mn)).nan_to_num(1e-8)
    x = wav[:, None, :].repeat(1, 3, 1).reshape(3 * chunks, 1, S)
    masks = w.permute(0, 2, 1).reshape(3 * chunks, Fw)
    check_case(f"osp Fw={Fw}", x, masks, o64, hips)


# --------------------------------------------------------------------------- #
# d. a handle's result does not depend on what it computed before
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("precision", PRECISIONS)
def test_result_independent_of_call_history(gpu, state, precision):
    S = 80000
    x = torch.from_numpy(synth_streams(MAX_ROWS, 5.0, seed0=600))[:, None, :S].contiguous()
    short, medium = torch.zeros(7, S), torch.zeros(33, S)
    for i in range(7):
        short[i, 1000 * i: 1000 * i + 700 + 211 * i] = 1.0          # lmax = 1966: T = 13
    for i in range(33):
        medium[i, 300 * i: 300 * i + 20000 + 397 * i] = 1.0         # lmax = 32704: T = 205
    calls = [(x, None), (x[:7], short), (x[40:73], medium), (x[:5], None)]
    reused = M.HipEcapaEmbedding(state, max_batch=MAX_ROWS, precision=precision).to(gpu)
    got = []
    for xi, mi in calls:
        got.append(run_hip(reused, xi, mi))
    for (xi, mi), r in zip(calls, got):
        fresh = run_hip(M.HipEcapaEmbedding(state, max_batch=MAX_ROWS, precision=precision).to(gpu), xi, mi)
        assert r["T"] == fresh["T"]
        for k in ("emb", "feats", "block0", "mfa", "logits", "pooled", "lens", "nvalid", "nmask"):
            assert torch.equal(r[k], fresh[k]), (xi.shape[0], k)


# --------------------------------------------------------------------------- #
# e. signal level: the DFT is the one split-f16 GEMM fed raw audio
# --------------------------------------------------------------------------- #
def test_signal_levels(o64, hips):
    """Full scale, 1e-2, 16-bit LSB noise, 1e-5 and 1e-6, an all-zero kept region and a DC offset, in one batch:
    the 1e-10 clamp and the top-db floor are reached from both sides."""
    S = 24000
    base = torch.from_numpy(synth_streams(8, 1.5, seed0=700))[:, :S].double()
    base = base / base.abs().amax(dim=1, keepdim=True)             # full scale: peak 1
    g = torch.Generator().manual_seed(7)
    lsb = torch.round(torch.randn(S, generator=g, dtype=torch.float64) * 3.0) * 2.0 ** -15
    rows = [base[0], 1e-2 * base[1], lsb, 1e-5 * base[3], 1e-6 * base[4], torch.zeros(S, dtype=torch.float64),
            0.05 + 0.1 * base[6], 1e-6 * base[7]]
    x = torch.stack(rows).float()[:, None, :]
    x[5, 0, :4000] = 0.3 * x[0, 0, :4000]                          # the zero row has signal outside its kept region
    spans = [(0, S), (0, S), (0, S), (500, S - 300), (0, S - 2000), (6000, 21000), (0, S), (1234, 1234 + 9000)]
    check_case("levels", x, sample_masks(S, spans), o64, hips)
