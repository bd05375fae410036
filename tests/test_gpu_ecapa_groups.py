"""Config 3 embedding over groups: ``HipEcapaEmbedding.forward_groups`` (dz_ecapa_forward_groups) runs G groups of
K rows in one launch sequence, each group with the batch geometry of its own K rows, derived on the device.

The yardstick is ``dz_ecapa_forward`` on one group alone (the live reference embeds a chunk's K speaker rows in a
call of their own): a group's rows must come out bit-identical to it, whatever the other groups hold, and within
the float64 gates of test_gpu_ecapa_geometry.py (restated here) against oracle/ecapa_ref.py run on that group.
The call must not wait for the GPU."""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.synth import synth_ecapa_state, synth_streams

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16x3", "f32")
EMB_GATE, COS_GATE = 1e-5, 1e-10      # relative L2 per row / 1 - cosine against float64 (test_gpu_ecapa_geometry.py)
MAX_ROWS = 192                        # 64 streams x 3 speakers


@pytest.fixture(scope="module")
def state():
    return synth_ecapa_state()


@pytest.fixture(scope="module")
def o64(state):
    from oracle.ecapa_ref import PretrainedSpeakerEmbeddingRef
    return PretrainedSpeakerEmbeddingRef(state, dtype=torch.float64)


@pytest.fixture(scope="module")
def hips(gpu, state):
    """Per precision: one model for the groups calls, one for the single-group calls of the existing entry."""
    return {p: (M.HipEcapaEmbedding(state, max_batch=MAX_ROWS, precision=p).to(gpu),
                M.HipEcapaEmbedding(state, max_batch=MAX_ROWS, precision=p).to(gpu)) for p in PRECISIONS}


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_bit_equal(a, b, what):
    assert a.shape == b.shape, what
    diff = (bits(a) != bits(b)).reshape(a.shape[0], -1).any(dim=1)
    assert not diff.any(), (what, diff.nonzero().flatten().tolist())


def solo(hip, wave, masks):
    """dz_ecapa_forward on one group: the group's waveform once per row, its K mask rows -> (K, 192) + peek 5/6/7."""
    K, S = masks.shape[0], wave.shape[-1]
    x = wave.reshape(1, 1, S).expand(K, 1, S).contiguous()
    out = hip(x, masks).cpu()
    geo = [hip.peek(S, i)[0].cpu() for i in (5, 6, 7)]
    return out, geo, hip.peek(S, 5)[1]


def groups(hip, waves, masks, normalize=False):
    G, K = masks.shape[:2]
    S = waves.shape[-1]
    out = hip.forward_groups(waves, masks, normalize=normalize)
    geo = [hip.peek(S, i)[0].cpu().view(G, K) for i in (5, 6, 7, 8)]
    return out.cpu(), geo, hip.peek(S, 5)[1]


def sample_masks(S, spans):
    m = torch.zeros(len(spans), S)
    for i, (a, b) in enumerate(spans):
        m[i, a:b] = 1.0
    return m


# --------------------------------------------------------------------------- #
# 1. one group = the existing entry on the same rows
# --------------------------------------------------------------------------- #
def _one_group_cases():
    from oracle.ecapa_ref import rounding_edges
    cases = []
    S, lmax = 80000, 62340                                   # rounding edges of float32(len / lmax) * T
    e = rounding_edges(lmax)
    lens = [lmax]
    for k, n in (("differs", 5), ("int", 4), ("half", 4), ("near", 4)):
        lens += [v for v in e[k] if v not in lens][:n]
    lens += [639, 17]                                        # too short: NaN rows with rel = 1
    spans = [((i * 997) % (S - n + 1), (i * 997) % (S - n + 1) + n) for i, n in enumerate(lens)]
    cases.append(("edges", S, spans, None))
    for N, lmax in ((7, 799), (96, 640), (64, 959), (33, 4800), (65, 10240)):   # N T mod 128 = 35, 96, 0, 127, 1
        S = lmax + 37
        g = torch.Generator().manual_seed(N * 100003 + lmax)
        ln = torch.randint(640, lmax + 1, (N,), generator=g)
        ln[0] = lmax
        ln[1:3] = torch.randint(1, 640, (2,), generator=g)
        ln[3] = 640
        sp = []
        for n in ln.tolist():
            a = int(torch.randint(0, S - n + 1, (1,), generator=g))
            sp.append((a, a + n))
        cases.append((f"N{N}-T{1 + lmax // 160}", S, sp, 5 if N == 33 else None))
    cases.append(("all-short", 4000, [(0, 600), (100, 300), (3000, 3639)], None))
    return cases


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_group_equals_the_existing_entry(hips, precision):
    """G = 1, K = N: every row bit-identical to dz_ecapa_forward on the same rows (rounding-edge lengths, the N T mod
    128 sweep, too-short rows, a kept NaN sample, an all-too-short call); peek 5 / 6 / 7 identical."""
    hg, hs = hips[precision]
    for name, S, spans, nan_row in _one_group_cases():
        N = len(spans)
        wave = torch.from_numpy(synth_streams(1, S / 16000 + 0.01, seed0=40 + N))[:, :S].clone()
        if nan_row is not None:
            a, b = spans[nan_row]
            wave[0, (a + b) // 2] = float("nan")             # kept by this row (and any row that keeps that sample)
        masks = sample_masks(S, spans).to(hg.device)
        d_wave = wave.to(hg.device)
        want, wgeo, wT = solo(hs, d_wave, masks)
        got, ggeo, gT = groups(hg, d_wave.view(1, 1, S), masks.view(1, N, S))
        assert gT == 1 + S // 160
        assert_bit_equal(got.view(N, 192), want, (name, precision))
        for i, (a, b) in enumerate(zip(ggeo[:3], wgeo)):
            assert torch.equal(a.flatten(), b), (name, precision, 5 + i)
        assert (ggeo[3] == wT).all(), (name, precision)
        if nan_row is not None:
            assert torch.isnan(got.view(N, 192)[nan_row]).all()
        assert torch.isnan(got.view(N, 192)[1]).all() or name == "edges"


# --------------------------------------------------------------------------- #
# 2. groups with different geometries = their own calls, and the float64 oracle per group
# --------------------------------------------------------------------------- #
def osp_groups(G, Fw=293, S=80000, seed=0):
    """G chunks of K = 3 speakers: waveforms (G, 1, S), min-max normalised OSP weights (G, 3, Fw) as masks, each
    group's speech cut at a different frame (so lmax_g differs), group 1 all too short, group 2 a NaN sample."""
    from oracle.functional_ref import overlapped_speech_penalty_ref
    wav = torch.from_numpy(synth_streams(G, S / 16000, seed0=800 + seed))[:, None, :S].clone()
    g = torch.Generator().manual_seed(Fw + seed)
    seg = torch.rand(G, Fw, 3, generator=g)
    seg[:, :, 2] *= 0.05
    w = overlapped_speech_penalty_ref(seg)
    mn, mx = w.min(dim=1, keepdim=True).values, w.max(dim=1, keepdim=True).values
    w = ((w - mn) / (mx - mn)).nan_to_num(1e-8).permute(0, 2, 1).contiguous()     # (G, 3, Fw)
    for i in range(G):
        cut = Fw - (i * 37) % (Fw - 8)
        w[i, :, cut:] = 0.0
    if G > 1:
        w[1] = 0.0
        w[1, 0, :2] = 1.0                                    # 2 frames ~ 546 samples: every row too short
    if G > 2:
        w[2, 0, 10] = 1.0
        f = int(10.5 * S / Fw)
        wav[2, 0, f] = float("nan")                          # kept by row 0 of group 2
    return wav, w


@pytest.mark.parametrize("G", [1, 7, 64])
def test_groups_equal_their_own_calls(hips, o64, G):
    """K = 3, OSP-style masks at Fw = 293: each group bit-identical to dz_ecapa_forward on that group alone; T_g
    (peek 8), nvalid and nmask equal the oracle's frame counts; (G = 7) each group within the float64 gates."""
    wav, w = osp_groups(G, seed=G)
    S = wav.shape[-1]
    geoms = [o64.geometry(wav[i:i + 1].expand(3, 1, S), w[i]) for i in range(G)]
    refs = {}
    for p in PRECISIONS:
        hg, hs = hips[p]
        got, ggeo, _ = groups(hg, wav.to(hg.device), w.to(hg.device))
        got = got.view(G, 3, 192)
        for i in range(G):
            want, wgeo, _ = solo(hs, wav[i].to(hs.device), w[i].to(hs.device))
            assert_bit_equal(got[i], want, (p, G, i))
            gm = geoms[i]
            T = gm["T"]
            assert (ggeo[3][i] == T).all(), (p, i, ggeo[3][i], T)
            if T == 0:
                assert (ggeo[1][i] == 0).all() and (ggeo[2][i] == 0).all()
                assert torch.isnan(got[i]).all()
            else:
                assert torch.equal(ggeo[1][i].long(), gm["nvalid"].long()), (p, i)
                assert torch.equal(ggeo[2][i].long(), gm["nmask"].long()), (p, i)
        if G > 2:                                            # the NaN sample poisons its own row only
            assert torch.isnan(got[2, 0]).all()
            for k in (1, 2):
                assert bool(torch.isnan(got[2, k]).all()) == bool(geoms[2]["too_short"][k]), (p, k)
                assert bool(torch.isnan(got[2, k]).any()) == bool(geoms[2]["too_short"][k]), (p, k)
        if G == 7:
            for i in range(G):
                if geoms[i]["T"] == 0:
                    continue
                if i not in refs:
                    refs[i] = o64.stages(geoms[i])["emb"]
                ref = refs[i]
                ok = ~torch.isnan(ref).any(dim=1)
                if i == 2:
                    ok[0] = False                            # the reference's row is NaN through its stages
                assert torch.isnan(got[i][~ok]).all()
                a, b = got[i][ok].double(), ref[ok]
                err = ((a - b).norm(dim=1) / b.norm(dim=1)).max().item()
                cos = torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()
                assert err < EMB_GATE and 1.0 - cos < COS_GATE, (p, i, err, 1.0 - cos)
    lmaxes = {g["T"] for g in geoms}
    assert G == 1 or len(lmaxes) >= min(G, 4), lmaxes


def test_normalize_flag_is_the_embedding_normalisation(hips):
    """normalize = 1 is EmbeddingNormalization(1) of the block (dz_l2_normalize) on the same rows, NaN rows kept."""
    from diart_amd import functional as F
    wav, w = osp_groups(5, seed=11)
    hg, _ = hips["f16x3"]
    raw = hg.forward_groups(wav.to(hg.device), w.to(hg.device))
    want = F.normalize_embeddings(raw.view(15, 192)).view(5, 3, 192).cpu()
    got = hg.forward_groups(wav.to(hg.device), w.to(hg.device), normalize=True).cpu()
    assert_bit_equal(got.view(15, 192), want.view(15, 192), "normalize")
    assert torch.isnan(got[1]).all()


# --------------------------------------------------------------------------- #
# 3. a group does not see its neighbours
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("precision", PRECISIONS)
def test_neighbour_independence(hips, precision):
    """Replacing the other groups (other audio, other masks, other lengths) or permuting the groups leaves every
    group's rows bitwise unchanged."""
    hg, _ = hips[precision]
    wav, w = osp_groups(7, seed=21)
    wav2, w2 = osp_groups(7, seed=22)
    d = lambda t: t.to(hg.device)                            # noqa: E731
    base = hg.forward_groups(d(wav), d(w)).cpu()
    for j in (0, 3, 6):
        wx, mx = wav2.clone(), w2.clone()
        wx[j], mx[j] = wav[j], w[j]
        got = hg.forward_groups(d(wx), d(mx)).cpu()
        assert_bit_equal(got[j], base[j], (precision, "replaced", j))
    perm = torch.tensor([4, 0, 6, 2, 5, 1, 3])
    got = hg.forward_groups(d(wav[perm].contiguous()), d(w[perm].contiguous())).cpu()
    assert_bit_equal(got, base[perm], (precision, "permuted"))
    one = hg.forward_groups(d(wav[3:4].contiguous()), d(w[3:4].contiguous())).cpu()
    assert_bit_equal(one[0], base[3], (precision, "alone"))


# --------------------------------------------------------------------------- #
# 4. no host synchronisation
# --------------------------------------------------------------------------- #
def sleep_cycles_for(seconds, device):
    """torch.cuda._sleep cycles that last about `seconds` on this device (calibrated here)."""
    cyc = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cyc)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    return int(cyc * seconds * 1e3 / max(ms, 1e-3))


def test_groups_forward_does_not_wait_for_the_gpu(hips, gpu):
    hg, _ = hips["f16x3"]
    wav, w = osp_groups(64, seed=31)
    d_wav, d_w = wav.to(gpu), w.to(gpu)
    want = hg.forward_groups(d_wav, d_w).cpu()               # (warm: the handle exists)
    cycles = sleep_cycles_for(0.3, gpu)
    torch.cuda.synchronize(gpu)
    torch.cuda._sleep(cycles)
    ev = torch.cuda.Event()
    ev.record()
    out = hg.forward_groups(d_wav, d_w)
    pending = not ev.query()
    torch.cuda.synchronize(gpu)
    assert pending, "dz_ecapa_forward_groups waited for work queued before it"
    assert_bit_equal(out.cpu(), want, "after the sleep")
