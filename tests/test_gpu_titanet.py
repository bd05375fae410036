"""NeMo TitaNet-L on the HIP kernels (``dz_ttn_*``, csrc/k_titanet.hip) against the float64 restatement
(tests/titanet_ref.py), synthetic weights, both precisions.

Gate: relative L2 <= 2e-4 per stage and for the embedding, over each row's own valid frames — the gate ECAPA and
the speechbrain x-vector are held to (tests/test_gpu_sb_xvector.py).  Measured on an MI355X: every stage and the
embedding within 1.1e-6 ("f16x3") and 1.5e-6 ("f32"); the depthwise kernel within 8.4e-8.  The depthwise kernel alone is held to 2e-6:
at most 15 fused multiply-adds in float32 (15 x 2^-24 = 9e-7 in the worst case) plus, for the plane output, the
22-bit split (2^-22 = 2.4e-7)."""
import pytest
import torch

from diart_amd import _lib
from diart_amd.models import EmbeddingLoader, HipTitaNetEmbedding
from diart_amd.synth import synth_titanet_state
from diart_amd.weights import from_kb
from titanet_ref import TitaNetRef

pytestmark = pytest.mark.gpu

GATE = 2e-4
S, FW = 32000, 200                  # 2 s windows (201 frames), 200 mask frames of 160 samples
STAGES = ("feats", "block0", "block1", "block2", "block3", "block4")
WIDTH = (80, 1024, 1024, 1024, 1024, 3072)


@pytest.fixture(scope="module")
def sd():
    return synth_titanet_state()


@pytest.fixture(scope="module")
def ref(sd):
    return TitaNetRef(sd)


@pytest.fixture(scope="module", params=["f16x3", "f32"])
def model(request, sd):
    return HipTitaNetEmbedding(sd, max_batch=8, precision=request.param).to(torch.device("cuda"))


def _inputs(seed=0):
    """Six rows: full mask | half the samples | fewer than min_num_samples | digital silence | a silent stretch | a
    mask with holes."""
    g = torch.Generator().manual_seed(seed)
    wav = 0.1 * torch.randn(6, 1, S, generator=g)
    wav[:, 0] += 0.05 * torch.sin(torch.arange(S) * 0.05)[None]
    masks = torch.ones(6, FW)
    masks[1, 100:] = 0.0
    masks[2] = 0.0
    masks[2, 7] = 1.0                       # 160 kept samples < 257
    wav[3] = 0.0
    wav[4, 0, 9000:20000] = 0.0
    masks[5] = (torch.rand(FW, generator=g) > 0.4).float()
    return wav, masks


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm().clamp(min=1e-300))


SILENT = 3          # the digitally silent row of _inputs(): its normalised features are exactly zero on the device


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_stages_and_embedding_against_float64(model, ref):
    wav, masks = _inputs()
    out = model(wav.cuda(), masks.cuda()).cpu()
    geom = ref.geometry(wav, masks)
    want = ref.stages(geom)
    frames = geom["frames"].tolist()
    lens, _ = model.peek(S, 7)
    assert lens.cpu().tolist() == ref.select(wav, masks)[1].tolist()
    assert model.peek(S, 9)[0].cpu().tolist() == frames
    worst = {}
    for which, (name, width) in enumerate(zip(STAGES, WIDTH)):
        got, T = model.peek(S, which)
        got = got.cpu().view(6, T, width)
        if name == "feats":
            # every bin of a silent row is log(2^-24) at every frame: the float64 sums of the normalisation are exact,
            # the row is exactly zero (the reference: zero up to its own rounding), and a relative error is undefined
            assert bool((got[SILENT] == 0).all()) and float(want[name][SILENT].abs().max()) < 1e-6
        worst[name] = max(_rel(got[r, :n], want[name][r, :n]) for r, n in enumerate(frames)
                          if not (name == "feats" and r == SILENT))
    pooled = model.peek(S, 6)[0].cpu().view(6, 6144)
    worst["pooled"] = max(_rel(pooled[r], want["pooled"][r]) for r in range(6))
    ok = ~geom["too_short"]
    assert torch.isnan(out[~ok]).all() and torch.isfinite(out[ok]).all()
    worst["emb"] = max(_rel(out[r], want["emb"][r]) for r in range(6) if ok[r])
    print(model.precision, {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= GATE for v in worst.values()), worst


def test_all_short_call_and_no_masks(model, ref):
    wav, _ = _inputs(1)
    masks = torch.zeros(6, FW)
    masks[:, 3] = 1.0
    out = model(wav.cuda(), masks.cuda()).cpu()
    assert torch.isnan(out).all() and torch.isnan(ref(wav, masks)).all()
    out = model(wav[:3].cuda(), None).cpu()
    want = ref(wav[:3], None)
    worst = max(_rel(out[r], want[r]) for r in range(3))
    print(model.precision, f"masks=None {worst:.2e}")
    assert worst <= GATE


def test_groups_match_forward_bit_for_bit_and_launches_repeat(model):
    wav, masks = _inputs(2)
    G, K = 3, 2
    gm = masks.view(G, K, FW).cuda()
    a = model.forward_groups(wav[:G].cuda(), gm)
    b = model.forward_groups(wav[:G].cuda(), gm)
    assert torch.equal(_bits(a), _bits(b))
    for g in range(G):
        alone = model(wav[g:g + 1].expand(K, 1, S).contiguous().cuda(), gm[g])
        assert torch.equal(_bits(a[g]), _bits(alone)), g
    # a group whose rows are ALL below min_num_samples is NaN as a whole and leaves its neighbours' bits alone
    short = gm.clone()
    short[1] = 0.0
    short[1, :, 5] = 1.0
    c = model.forward_groups(wav[:G].cuda(), short)
    assert torch.isnan(c[1]).all()
    assert torch.equal(_bits(c[0]), _bits(a[0])) and torch.equal(_bits(c[2]), _bits(a[2]))
    alone = model(wav[1:2].expand(K, 1, S).contiguous().cuda(), short[1])
    assert torch.isnan(alone).all()
    n = model.forward_groups(wav[:G].cuda(), gm, normalize=True).cpu()
    fin = torch.isfinite(n).all(dim=2)
    assert torch.allclose(n[fin].norm(dim=1), torch.ones(int(fin.sum())), atol=1e-5)


@pytest.mark.parametrize("taps", [3, 7, 11, 15])
@pytest.mark.parametrize("planes", [False, True])
def test_depthwise_alone(taps, planes):
    g = torch.Generator().manual_seed(taps)
    rows, T, Cc = 3, 70, 256
    x = torch.randn(rows, T, Cc, generator=g)
    w = torch.randn(taps, Cc, generator=g)
    frames = torch.tensor([1, T, 33], dtype=torch.int32)
    dev = torch.device("cuda")
    xd, wd, fd = x.to(dev), w.to(dev), frames.to(dev)
    y = torch.zeros(rows, T, Cc, device=dev)
    pl = torch.zeros(2 * rows * T * Cc, dtype=torch.int16, device=dev)
    lib = _lib.load()
    for relu in (0, 1):
        _lib.check(lib.dz_k_ttn_depthwise(_lib.context(0), xd.data_ptr(), Cc, wd.data_ptr(), taps, fd.data_ptr(), rows, T,
                                          Cc, relu, None if planes else y.data_ptr(), pl.data_ptr() if planes else None,
                                          None), "dz_k_ttn_depthwise")
        torch.cuda.synchronize()
        if planes:
            p = from_kb(pl.cpu().view(torch.float16), rows * T, Cc).double()
            got = (p[0] + p[1] / 2048.0).view(rows, T, Cc)
        else:
            got = y.cpu().double()
        u = (x.relu() if relu else x).double()
        mask = (torch.arange(T)[None, :] < frames[:, None])[:, :, None]
        want = torch.nn.functional.conv1d((u * mask).transpose(1, 2), w.double().t()[:, None, :], padding=taps // 2,
                                          groups=Cc).transpose(1, 2)
        err = max(_rel(got[r], want[r]) for r in range(rows))
        print(f"depthwise k={taps} planes={planes} relu={relu}: {err:.2e}")
        assert err <= 2e-6


def test_loader_builds_the_titanet_handle(sd):
    m = EmbeddingLoader(sd, max_batch=4)()
    assert isinstance(m, HipTitaNetEmbedding) and m.dimension == 192
