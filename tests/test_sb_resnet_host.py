"""speechbrain ResNet (speechbrain/spkrec-resnet-voxceleb): what needs no GPU — checkpoint detection by EmbeddingLoader /
EmbeddingModel.from_pretrained, the C ABI additions, the packer's shape checks and folding, and the float64
restatement's (R) points (tests/sb_resnet_ref.py)."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import sb_resnet_ref as R
from diart_amd import _lib, models, weights
from diart_amd.synth import (synth_ecapa_state, synth_embedding_state, synth_sb_resnet_state, synth_sb_xvector_state,
                             synth_titanet_state, synth_wespeaker_state)

NARROW = dict(channels=(32, 32, 64, 64), block_sizes=(2, 1, 1, 1))


@pytest.fixture(scope="module")
def state():
    return synth_sb_resnet_state(**NARROW)


def test_state_keys_are_the_tables(state):
    k = weights.sb_resnet_key
    bn = lambda p: {f"{p}.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    wb = lambda p: {p + ".weight", p + ".bias"}
    want = wb(k("stem")) | bn(k("stem_bn")) | wb(k("att1")) | bn(k("att_bn")) | wb(k("att2")) | bn(k("norm_stats")) \
        | wb(k("fc")) | bn(k("norm_embed"))
    for L, nb in enumerate(NARROW["block_sizes"], start=1):
        for i in range(nb):
            want |= {k("conv1", L, i) + ".weight", k("conv2", L, i) + ".weight"} | bn(k("bn1", L, i)) | bn(k("bn2", L, i))
            want |= wb(k("se1", L, i)) | wb(k("se2", L, i))
            if i == 0 and L > 1:
                want |= {k("down", L, i) + ".weight"} | bn(k("down_bn", L, i))
    assert set(state) == want
    assert k("conv1", 2, 0) == "layer2.0.conv1" and k("se2", 1, 1) == "layer1.1.se.fc.2"
    assert k("down_bn", 3, 0) == "layer3.0.downsample.1" and k("att2") == "attention.3"
    assert state["conv1.weight"].shape == (32, 1, 3, 3) and state["attention.0.weight"].shape == (128, 640, 1)
    assert state["fc_embed.weight"].shape == (256, 1280)
    # the identity-shortcut block, strided blocks with and without a width change
    assert "layer1.0.downsample.0.weight" not in state and "layer1.1.downsample.0.weight" not in state
    assert state["layer2.0.downsample.0.weight"].shape == (32, 32, 1, 1)
    assert state["layer3.0.downsample.0.weight"].shape == (64, 32, 1, 1)
    full = weights.sb_resnet_shape(synth_sb_resnet_state(block_sizes=(1, 1, 1, 1)))
    assert full["channels"] == (128, 128, 256, 256) and full["pooled"] == 2560 and full["freq"] == 10


def test_loader_detects_the_checkpoint(state, tmp_path):
    """Without the architecture a state with these keys fell through to the pyannote x-vector (HipEmbedding), whose
    packer then failed on a missing SincNet key."""
    assert type(models.EmbeddingLoader(state)()) is models.HipSbResNetEmbedding
    assert type(models.EmbeddingLoader(state, arch="sb-resnet")()) is models.HipSbResNetEmbedding
    ckpt = tmp_path / "embedding_model.ckpt"
    torch.save(state, ckpt)
    m = models.EmbeddingModel.from_pretrained(str(ckpt))
    m.load()
    assert type(m.model) is models.HipSbResNetEmbedding
    assert m.model.dimension == 256 and m.model.precision in ("f16x3", "f32")
    assert models.HipSbResNetEmbedding(state, precision="f32").precision == "f32"
    with pytest.raises(ValueError, match="share"):
        models.HipSbResNetEmbedding(state, repeated_rows="share")
    m = models.EmbeddingLoader(state, strides=(1, 2, 2, 2), min_num_samples=400, rows_per_pass=2)()
    assert (m.strides, m.min_num_samples, m.rows_per_pass) == ((1, 2, 2, 2), 400, 2)
    with pytest.raises(TypeError, match="titanet"):
        models.EmbeddingLoader(state, pad_mode="reflect")()
    with pytest.raises(TypeError):
        models.EmbeddingLoader(synth_ecapa_state(channels=64), rows_per_pass=2)()


def test_other_detection_unchanged():
    assert type(models.EmbeddingLoader(synth_ecapa_state(channels=64))()) is models.HipEcapaEmbedding
    assert type(models.EmbeddingLoader(synth_wespeaker_state())()) is models.HipWeSpeakerEmbedding
    assert type(models.EmbeddingLoader(synth_embedding_state())()) is models.HipEmbedding
    assert type(models.EmbeddingLoader(synth_sb_xvector_state())()) is models.HipSbXvectorEmbedding
    assert type(models.EmbeddingLoader(synth_titanet_state())()) is models.HipTitaNetEmbedding


def test_abi_symbols_and_struct_size():
    lib = C.CDLL(str(_lib.lib_path()))
    for n in ("dz_sbr_abi_size", "dz_sbr_create", "dz_sbr_forward", "dz_sbr_forward_groups", "dz_sbr_peek",
              "dz_sbr_destroy", "dz_k_conv2d_masked", "dz_k_sbr_se_gate", "dz_k_sbr_se_apply", "dz_k_sbr_att_pool"):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    # a block: 3 convolutions of 3 pointers, 4 squeeze-excitation pointers, 4 ints
    assert C.sizeof(_lib.SbrBlock) == 8 * (9 + 4) + 16
    # 5 pointers, 32 blocks, 3 dz_layer of 5 pointers, zeros, 4 ints
    assert _lib.load().dz_sbr_abi_size() == C.sizeof(_lib.SbrWeights) == 8 * 5 + 32 * 120 + 8 * 15 + 8 + 16
    sizes = (C.c_int * 5)()
    assert _lib.load().dz_abi_struct_sizes(C.byref(sizes)) == 0 and _lib.load().dz_version() == 230


def test_frame_sequence_and_shapes(state):
    assert R.frames(501) == [501, 501, 251, 126, 63]
    assert R.frames(1) == [1, 1, 1, 1, 1]
    assert R.frames(2) == [2, 2, 1, 1, 1] and R.frames(6, (2, 2, 2, 2)) == [6, 3, 2, 1, 1]
    ref = R.SbResNetRef(state)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 4000, generator=g, dtype=torch.float64) * 0.1
    st = ref.stages(ref.geometry(x))
    T = R.frames(26)
    assert st["feats"].shape == (2, 26, 80) and st["stem"].shape == (2, 26, 80, 32)
    for l, (f, c) in enumerate(((80, 32), (40, 32), (20, 64), (10, 64)), start=1):
        assert st[f"layer{l}"].shape == (2, T[l], f, c)
    assert st["pooled"].shape == (2, 1280) and st["emb"].shape == (2, 256)
    # a single frame runs (T = 1 -> 1): the variance is 0 and the clamp gives sqrt(1e-5)
    one = ref.stages(ref.geometry(x[:, :, :100]))
    assert one["layer4"].shape == (2, 1, 10, 64) and torch.isfinite(one["emb"]).all()
    assert torch.allclose(one["pooled"][:, 640:], torch.full((2, 640), 1e-5, dtype=torch.float64).sqrt())


def test_too_short_and_nan_rows(state):
    ref = R.SbResNetRef(state, min_samples=480)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 1, 4000, generator=g, dtype=torch.float64) * 0.1
    masks = torch.zeros(3, 50)
    masks[0] = 1.0
    masks[1, :10] = 1.0            # 800 samples: kept
    masks[2, :5] = 1.0             # 400 samples: too short -> NaN
    out = ref(x, masks)
    assert out.shape == (3, 256)
    assert torch.isfinite(out[:2]).all() and torch.isnan(out[2]).all()
    assert torch.isnan(ref(x, masks * 0 + (torch.arange(50) < 5).float())).all()        # every row too short
    # a NaN sample makes its own row NaN and no other
    x[1, 0, 100] = float("nan")
    out = R.SbResNetRef(state)(x)
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all()


def test_min_num_samples_is_derived(state):
    """pyannote's bisection on the restated graph: zero-padded convolutions and a constant-padded STFT accept every
    length, so it ends at its lower end, 3."""
    ref = R.SbResNetRef(state)
    call = lambda w: ref(w.unsqueeze(1))
    assert R.min_num_samples(call) == 3
    assert weights.SB_RESNET_MIN_NUM_SAMPLES == 3 and models.HipSbResNetEmbedding(state).min_num_samples == 3

    def needs_four_frames(w):           # the bisection finds a bound where the graph has one
        if 1 + w.shape[1] // 160 < 4:
            raise RuntimeError("too short")
    assert R.min_num_samples(needs_four_frames) == 480


def test_packer_reads_the_shapes_and_refuses_by_name(state):
    shape = weights.sb_resnet_shape(state)
    assert shape["channels"] == (32, 32, 64, 64) and shape["block_sizes"] == (2, 1, 1, 1) and shape["stem"] == 32
    assert shape["se"] == [[32, 32], [32], [64], [64]] and shape["pooled"] == 640
    assert weights.sb_resnet_shape(synth_sb_resnet_state(se_reduction=4, **NARROW))["se"] == [[8, 8], [8], [16], [16]]
    for key, bad in (("layer2.0.conv2.weight", torch.zeros(32, 64, 3, 3)), ("layer1.1.bn1.running_var", torch.zeros(64)),
                     ("attention.0.weight", torch.zeros(128, 2560, 1)), ("fc_embed.weight", torch.zeros(192, 1280)),
                     ("layer3.0.se.fc.2.weight", torch.zeros(64, 32))):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            weights.sb_resnet_shape({**state, key: bad})
    missing = {k: v for k, v in state.items() if not k.startswith("layer3.0.downsample")}
    with pytest.raises(ValueError, match=r"layer3\.0\.downsample\.0\.weight"):
        weights.sb_resnet_shape(missing)
    with pytest.raises(ValueError, match="strides"):
        weights.sb_resnet_shape(state, strides=(1, 2, 3, 2))
    with pytest.raises(ValueError, match="48 channels"):
        weights.sb_resnet_shape(synth_sb_resnet_state(channels=(48, 48, 64, 64), block_sizes=(1, 1, 1, 1)))


def test_folded_matrices_restate_the_graph(state):
    """``sb_resnet_fold`` (what the kernels multiply with) against the unfolded restatement, in float64: the stem, one
    strided block's convolutions, and the head with its channel re-ordering."""
    ref = R.SbResNetRef(state)
    f = weights.sb_resnet_fold(state)
    g = torch.Generator().manual_seed(5)
    st = ref.stages(ref.geometry(torch.randn(2, 1, 3000, generator=g, dtype=torch.float64) * 0.1))
    conv = lambda x, m, b, k, s: torch.nn.functional.conv2d(
        x.permute(0, 3, 1, 2), m.reshape(m.shape[0], k, k, -1).permute(0, 3, 1, 2), b, s, k // 2).permute(0, 2, 3, 1)
    stem = torch.relu(conv(st["feats"].unsqueeze(-1), f["stem.w"], f["stem.b"], 3, 1))
    assert torch.allclose(stem, st["stem"], rtol=0, atol=1e-10)
    # block 2 = layer2.0 (stride 2, same width): conv1 and the shortcut as the kernels see them
    x = st["layer1"]
    mid = torch.relu(conv(x, f["b2.conv1.w"], f["b2.conv1.b"], 3, 2))
    y = conv(mid, f["b2.conv2.w"], f["b2.conv2.b"], 3, 1)
    gate = torch.sigmoid(torch.relu(y.mean(dim=(1, 2)) @ f["b2.se.w1t"] + f["b2.se.b1"]) @ f["b2.se.w2t"] + f["b2.se.b2"])
    out = torch.relu(y * gate[:, None, None, :] + conv(x, f["b2.down.w"], f["b2.down.b"], 1, 2))
    assert torch.allclose(out, st["layer2"], rtol=0, atol=1e-10)
    # the head over channels f C4 + c
    x4 = st["layer4"].flatten(2)                                           # (N, T4, F4 C4)
    a = torch.relu(x4 @ f["att1.w"].t() + f["att1.b"]) * f["att1.s"] + f["att1.h"]
    w = torch.softmax(a @ f["att2.w"].t() + f["att2.b"], dim=1)
    mu = (x4 * w).sum(dim=1)
    sg = ((x4 ** 2 * w).sum(dim=1) - mu ** 2).clamp(min=1e-5).sqrt()
    pooled = torch.cat([mu, sg], dim=1)
    assert torch.allclose(pooled, ref.device_order(st["pooled"], 64, 10), rtol=0, atol=1e-10)
    assert torch.allclose(pooled @ f["fc.w"].t() + f["fc.b"], st["emb"], rtol=0, atol=1e-9)


# ---- an independent float32 build of the same graph from torch.nn modules ------------------------------------------
class _SE(nn.Module):
    def __init__(self, c, cr):
        super().__init__()
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(c, cr), nn.ReLU(), nn.Linear(cr, c), nn.Sigmoid())

    def forward(self, x):
        return x * self.fc(self.pool(x).flatten(1))[:, :, None, None]


class _Block(nn.Module):
    def __init__(self, cin, c, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, c, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(c)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(c)
        self.se = _SE(c, c)
        self.downsample = None
        if stride != 1 or cin != c:
            self.downsample = nn.Sequential(nn.Conv2d(cin, c, 1, stride, bias=False), nn.BatchNorm2d(c))

    def forward(self, x):
        y = self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x)))))
        return torch.relu(self.se(y) + (x if self.downsample is None else self.downsample(x)))


class _Net(nn.Module):
    def __init__(self, channels, block_sizes, strides=(1, 2, 2, 2)):
        super().__init__()
        self.conv1 = nn.Conv2d(1, channels[0], 3, 1, 1)
        self.bn1 = nn.BatchNorm2d(channels[0])
        cin, f = channels[0], 80
        for L, (c, nb, s) in enumerate(zip(channels, block_sizes, strides), start=1):
            setattr(self, f"layer{L}", nn.Sequential(*[_Block(cin if i == 0 else c, c, s if i == 0 else 1) for i in range(nb)]))
            cin, f = c, (f - 1) // s + 1
        self.attention = nn.Sequential(nn.Conv1d(cin * f, 128, 1), nn.ReLU(), nn.BatchNorm1d(128), nn.Conv1d(128, cin * f, 1),
                                       nn.Softmax(dim=2))
        self.norm_stats = nn.BatchNorm1d(2 * cin * f)
        self.fc_embed = nn.Linear(2 * cin * f, 256)
        self.norm_embed = nn.BatchNorm1d(256)

    def forward(self, feats):
        x = torch.relu(self.bn1(self.conv1(feats.unsqueeze(1))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = x.transpose(2, 3).flatten(1, 2)
        w = self.attention(x)
        mu = (x * w).sum(dim=2)
        sg = torch.sqrt(((x ** 2 * w).sum(dim=2) - mu ** 2).clamp(min=1e-5))
        return self.norm_embed(self.fc_embed(self.norm_stats(torch.cat([mu, sg], dim=1))))


# float32-vs-float64 forward difference of this graph on these inputs, relative L2 per row: measured 3.3e-7 at worst
# over the rows below (3.3e-7 / 3.0e-7 / 2.2e-7 per length), given 3x
F32_GATE = 1.0e-6


def test_restatement_against_an_independent_float32_build(state):
    net = _Net(**NARROW).eval()
    net.load_state_dict(state, strict=True)
    ref = R.SbResNetRef(state)
    g = torch.Generator().manual_seed(6)
    worst = 0.0
    for n in (4000, 9000, 100):
        geom = ref.geometry(torch.randn(3, 1, n, generator=g, dtype=torch.float64) * 0.1)
        st = ref.stages(geom)
        with torch.no_grad():
            got = net(st["feats"].float()).double()
        rel = ((got - st["emb"]).norm(dim=1) / st["emb"].norm(dim=1)).max().item()
        print(f"n={n}: float32 nn build vs float64 restatement, worst relative L2 {rel:.3g}")
        worst = max(worst, rel)
    assert worst < F32_GATE, worst
