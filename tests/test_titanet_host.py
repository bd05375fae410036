"""NeMo TitaNet-L without a GPU: the float64 restatement (tests/titanet_ref.py), the ``.nemo`` reader, the loader's
recognition and every folded / packed weight against float64 unfolding."""
import io
import tarfile

import pytest
import torch
import torch.nn.functional as F

import titanet_ref as R
from diart_amd import checkpoint, models, weights
from diart_amd.synth import synth_titanet_state

# trainable parameters of the restatement without the 7205-way classifier; with it (192 x 7205 = 1 383 360 weights)
# 23 505 648 — the model card's "~25.3 M" is not reached by this reading of the architecture
PARAMETERS = 22_122_288


@pytest.fixture(scope="module")
def sd():
    return synth_titanet_state()


@pytest.fixture(scope="module")
def ref(sd):
    return R.TitaNetRef(sd)


def _wave(n, S=8000, seed=0):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn(n, 1, S, generator=g)


def test_shapes_and_parameter_count(sd, ref):
    assert R.parameter_count(sd) == PARAMETERS
    geom = ref.geometry(_wave(2), None)
    st = ref.stages(geom)
    assert geom["frames"].tolist() == [51, 51]
    assert st["feats"].shape == (2, 64, 80)                   # 51 frames padded to a multiple of 16
    assert [st[f"block{i}"].shape[2] for i in range(5)] == [1024, 1024, 1024, 1024, 3072]
    assert st["pooled"].shape == (2, 6144) and st["emb"].shape == (2, 192)
    assert bool((st["feats"][:, 51:] == 0).all())
    assert R.valid_frames(torch.tensor([8000]), "padded").tolist() == [51]
    assert R.MIN_NUM_SAMPLES == weights.TITANET_MIN_NUM_SAMPLES == 257


def _nemo(tmp_path, sd, gz, yaml):
    path = tmp_path / ("model.nemo")
    buf = io.BytesIO()
    torch.save(sd, buf)
    with tarfile.open(path, "w:gz" if gz else "w") as tar:
        for name, data in (("./model_config.yaml", yaml.encode()), ("./model_weights.ckpt", buf.getvalue())):
            info = tarfile.TarInfo(name)
            info.size = len(data)
            tar.addfile(info, io.BytesIO(data))
    return path


@pytest.mark.parametrize("gz", [False, True])
def test_nemo_archive_round_trip(tmp_path, gz):
    tiny = {"encoder.encoder.0.mconv.0.conv.weight": torch.randn(4, 1, 3), "decoder.emb_layers.0.1.weight": torch.randn(2, 4, 1),
            "counter": torch.tensor(7)}
    path = _nemo(tmp_path, tiny, gz, "preprocessor:\n  n_fft: 512\n  stft_pad_mode: constant  # newer NeMo\n")
    got = checkpoint.read_state(path)
    assert set(got) == set(tiny) and all(torch.equal(got[k], v) for k, v in tiny.items())
    assert checkpoint.nemo_frontend(path) == {"pad_mode": "constant"}
    assert checkpoint.nemo_frontend(_nemo(tmp_path, tiny, gz, "preprocessor:\n  n_fft: 512\n")) == {}
    # an entry of the same name in another section does not switch the front end
    other = "augmentor:\n  pad_mode: constant\npreprocessor:\n  n_fft: 512\n  frame_count: padded\ndecoder:\n  pad_mode: constant\n"
    assert checkpoint.nemo_frontend(_nemo(tmp_path, tiny, gz, other)) == {"frame_count": "padded"}


def test_nemo_archive_without_weights_is_refused(tmp_path):
    path = tmp_path / "empty.nemo"
    with tarfile.open(path, "w") as tar:
        info = tarfile.TarInfo("model_config.yaml")
        info.size = 0
        tar.addfile(info, io.BytesIO(b""))
    with pytest.raises(ValueError, match="model_weights.ckpt"):
        checkpoint.read_state(path)


def test_loader_recognises_titanet(sd, tmp_path):
    m = models.EmbeddingLoader(sd, max_batch=4)()
    assert isinstance(m, models.HipTitaNetEmbedding) and m.dimension == 192 and m.min_num_samples == 257
    m = models.EmbeddingLoader(_nemo(tmp_path, sd, True, "preprocessor:\n  stft_pad_mode: constant\n"), max_batch=4)
    assert m().pad_mode == "constant"
    # the loader passes every (R) switch through, over what the archive records
    m = models.EmbeddingModel.from_pretrained(m.state, pad_mode="reflect", frame_count="padded", min_num_samples=400,
                                              attention_order="bn_relu_tanh").get_model()
    assert (m.pad_mode, m.frame_count, m.min_num_samples, m.attention_order) == ("reflect", "padded", 400, "bn_relu_tanh")
    with pytest.raises(TypeError):
        models.EmbeddingLoader(sd, pad="reflect")
    from diart_amd.synth import synth_sb_xvector_state
    with pytest.raises(TypeError, match="titanet"):
        models.EmbeddingLoader(synth_sb_xvector_state(), pad_mode="reflect")()
    assert isinstance(models.EmbeddingModel.from_pretrained(sd).get_model(), models.HipTitaNetEmbedding)
    assert isinstance(models.EmbeddingLoader(sd, arch="titanet")(), models.HipTitaNetEmbedding)
    with pytest.raises(ValueError, match="share"):
        models.HipTitaNetEmbedding(sd, repeated_rows="share")


def test_folded_weights_against_float64(sd):
    """The fold the packer uploads (computed in float64, rounded once to float32) vs conv + BatchNorm unfolded in
    float64, and the f16 planes of a pointwise layer vs the folded matrix (22 bits: 2^-22 relative)."""
    pk = weights.PackedTitaNet(sd, torch.device("cpu"), precision="f16x3")
    f64 = pk.folded
    assert len(f64) == 11 * 3 + 5 * 2 + 3 * 2 + 9 and all(v.dtype == torch.float64 for v in f64.values())
    assert pk.struct.min_num_samples == 257 and pk.struct.pad_reflect == 1 and pk.struct.frame_nfft == 0
    m = f64["pw2.1.w"]
    planes = weights.from_kb(weights.kb_major(weights.split_f16(m.float())).view(torch.float16), 1024, 1024).double()
    assert float((planes[0] + planes[1] / 2048.0 - m).norm() / m.norm()) < 2.0 ** -22
    d = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = torch.randn(2, 1024, 9, dtype=torch.float64)
    for i, (reps, k, cin, cout, residual) in enumerate(weights.TITANET_BLOCKS):
        for j in range(reps):
            xi = x[:, :cin]
            bn = weights.titanet_key("bn", i, j)
            want = F.batch_norm(F.conv1d(xi, d[weights.titanet_key("pw", i, j)]), d[bn + ".running_mean"], d[bn + ".running_var"],
                                d[bn + ".weight"], d[bn + ".bias"], training=False, eps=1e-3)
            got = torch.einsum("oc,nct->not", f64[f"pw{i}.{j}.w"], xi) + f64[f"pw{i}.{j}.b"][None, :, None]
            assert torch.allclose(got, want, rtol=1e-11, atol=1e-11), (i, j)
            dw = F.conv1d(xi, d[weights.titanet_key("dw", i, j)], padding=k // 2, groups=cin)
            taps = f64[f"dw{i}.{j}"]
            mine = sum(taps[t][None, :, None] * F.pad(xi, (k // 2, k // 2))[:, :, t:t + 9] for t in range(k))
            assert torch.allclose(mine, dw, rtol=1e-11, atol=1e-11), (i, j)
        assert torch.equal(f64[f"se{i}.2t"].t(), d[weights.titanet_key("se", i, l=2)])
    p = torch.randn(3, 6144, dtype=torch.float64)
    e = weights.TITANET_KEYS["emb_bn"]
    want = F.batch_norm(p, d[e + ".running_mean"], d[e + ".running_var"], d[e + ".weight"], d[e + ".bias"], training=False,
                        eps=1e-5) @ d[weights.TITANET_KEYS["emb_fc"] + ".weight"][:, :, 0].t() + d[weights.TITANET_KEYS["emb_fc"] + ".bias"]
    assert torch.allclose(p @ f64["fc.w"].t() + f64["fc.b"], want, rtol=1e-10, atol=1e-10)
    # the attention layer, both orders: tanh(relu(W x + b) s + h)
    z = torch.randn(4, 9216, dtype=torch.float64)
    a, b = weights.TITANET_KEYS["att_conv"], weights.TITANET_KEYS["att_bn"]
    lin = z @ d[a + ".weight"][:, :, 0].t() + d[a + ".bias"]
    bnf = lambda v: F.batch_norm(v, d[b + ".running_mean"], d[b + ".running_var"], d[b + ".weight"], d[b + ".bias"],
                                 training=False, eps=1e-5)
    for order, want in (("relu_bn_tanh", bnf(lin.relu())), ("bn_relu_tanh", bnf(lin).relu())):
        f = weights.titanet_fold(sd, order, dtype=torch.float64)
        got = (z[:, :3072] @ f["att.w"].t() + z[:, 3072:] @ f["att.wms"].t() + f["att.b"]).relu() * f["att.s"] + f["att.h"]
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-10), order


def test_dft_and_mel_operands_against_torch_stft():
    x = torch.randn(3, 4000, dtype=torch.float64)
    spec = torch.stft(x, 512, 160, 400, torch.hann_window(400, periodic=False, dtype=torch.float64), center=True,
                      pad_mode="constant", return_complex=True)
    want = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)
    frames = F.pad(x, (200, 200)).unfold(1, 400, 160)                      # the 400 samples under each window
    ri = frames @ weights.titanet_dft_matrices().t()
    got = ri[..., :257] ** 2 + ri[..., 257:] ** 2
    assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-9, atol=1e-9)
    assert torch.allclose(weights.titanet_mel_filterbank().t(), R.mel_filterbank(), rtol=0, atol=1e-15)
    m = weights.titanet_mel_filterbank()
    # anchors of the slaney scale worked out by hand (200 / 3 Hz per mel below 1 kHz = mel 15, 27 log steps per factor
    # 6.4 above; 82 points from 0 to mel(8000) = 15 + 27 ln 8 / ln 6.4 = 45.24564, 0.5585882 apart): the centres of
    # triangles 0, 1, 79 and the two around the 1 kHz break (points 26, 27), as the bins (31.25 Hz apart) where a
    # triangle peaks and ends; slaney normalisation: height 2 / (right - left), so a triangle has unit area in Hz
    centre = {0: 37.23921, 1: 74.47842, 25: 968.21947, 26: 1005.64528, 78: 7408.54219, 79: 7698.59322}
    for i, c in centre.items():
        left, right = (0.0 if i == 0 else centre.get(i - 1)), (8000.0 if i == 79 else centre.get(i + 1))
        row = m[i]
        assert abs(int(row.argmax()) * 31.25 - c) <= 31.25 / 2 + 1e-9, i
        if left is not None and right is not None:
            nz = torch.nonzero(row)[:, 0]
            assert int(nz[0]) == int(left // 31.25) + 1 and int(nz[-1]) == -int(-right // 31.25) - 1, i
            k = int(row.argmax())            # a point on the rising or falling edge has the triangle's exact height
            f = k * 31.25
            h = 2.0 / (right - left) * ((f - left) / (c - left) if f <= c else (right - f) / (right - c))
            assert abs(float(row[k]) - h) < 1e-7 * h, i
    assert abs(float(m[79].sum()) * 31.25 - 1.0) < 0.01       # 19 bins wide: the bin sum is the area to 1 %
    assert m.shape == (80, 257) and float(m[:, -1].abs().max()) == 0.0 and bool((m.sum(dim=1) > 0).all())


@pytest.mark.parametrize("pad_mode", R.PAD_MODES)
def test_masked_path_equals_the_compacted_signal(sd, pad_mode):
    ref = R.TitaNetRef(sd, pad_mode=pad_mode)
    wav = _wave(3, seed=3)
    g = torch.Generator().manual_seed(4)
    masks = (torch.rand(3, 50, generator=g) > 0.3).float()
    masks[0] = 1.0                                        # (the longest row: the batch pads every row to its length)
    out = ref(wav, masks)
    signals, lens = ref.select(wav, masks)
    for r in range(3):
        # the row alone, already compacted and padded like the batch: no mask needed
        alone = ref.stages({"signals": signals[r:r + 1], "lens": lens[r:r + 1], "too_short": torch.tensor([False]),
                            "frames": R.valid_frames(lens[r:r + 1])})["emb"]
        assert torch.allclose(out[r], alone[0], rtol=1e-9, atol=1e-11), r
    if pad_mode == "constant":                            # zeros past the row: the batch's length does not show at all
        n = int(lens[1])
        alone = ref(signals[1:2, None, :n], None)
        assert torch.allclose(out[1], alone[0], rtol=1e-9, atol=1e-11)


def test_wrapper_nan_rules(ref):
    wav = _wave(3, seed=5)
    short = torch.zeros(3, 50)
    short[:, 0] = 1.0                                     # 160 kept samples each
    assert torch.isnan(ref(wav, short)).all()
    some = torch.ones(3, 50)
    some[1] = short[1]
    out = ref(wav, some)
    assert torch.isnan(out[1]).all() and torch.isfinite(out[[0, 2]]).all()
    assert torch.isfinite(ref(wav, None)).all() and ref(wav, None).shape == (3, 192)
    assert torch.allclose(ref(wav, None), ref(wav, torch.ones(3, 50)))


def test_stream_seed_keeps_the_f64_and_f32_reference_pipelines_together(ref):
    """The seed check of tests/test_gpu_titanet_blocks.py, on the oracle's own segmentation: over the synthetic
    stream the reference-shaped pipeline assigns the same speakers at every step whether its float64 embeddings are
    rounded to float32 or not, and the stream exercises the clustering (turns at every step, three speakers)."""
    import numpy as np
    import titanet_chain as chain
    from diart_amd.synth import synth_segmentation_state, synth_stream
    from oracle.models_ref import PyanNetRef, powerset_to_multilabel
    from test_gpu_der import rolling_chunks
    seg_m = PyanNetRef(powerset=True).eval()
    seg_m.load_state_dict(synth_segmentation_state(seed=77, powerset=True))
    chunks = rolling_chunks(synth_stream(chain.STREAM_SEED, chain.STREAM_SECONDS))
    x = torch.from_numpy(np.stack([c.data[:, 0] for c in chunks]))[:, None, :]
    with torch.no_grad():
        seg = powerset_to_multilabel(seg_m(x))
    emb = chain.embed(ref, chunks, seg)
    a, b = chain.tracks(seg, emb, rounded=False), chain.tracks(seg, emb, rounded=True)
    assert a == b and len(a) == 15
    assert sum(map(len, a)) >= 15 and len({s for st in a for *_, s in st}) >= 2
