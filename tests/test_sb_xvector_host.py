"""speechbrain x-vector (speechbrain/spkrec-xvect-voxceleb): what needs no GPU — checkpoint detection by
EmbeddingLoader / EmbeddingModel.from_pretrained, the C ABI additions, the weight packing and the float64
restatement's (R) points (tests/sb_xvector_ref.py, DESIGN.md "speechbrain x-vector")."""
import ctypes as C

import pytest
import torch

import sb_xvector_ref as R
from diart_amd import _lib, models
from diart_amd.synth import (synth_ecapa_state, synth_embedding_state, synth_sb_xvector_state,
                             synth_segmentation_state, synth_wespeaker_state)


@pytest.fixture(scope="module")
def state():
    return synth_sb_xvector_state()


def test_state_keys_are_speechbrains(state):
    convs = {f"blocks.{i}.conv.{p}" for i in (0, 3, 6, 9, 12) for p in ("weight", "bias")}
    norms = {f"blocks.{i}.norm.{p}" for i in (2, 5, 8, 11, 14)
             for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(state) == convs | norms | {"blocks.16.w.weight", "blocks.16.w.bias"}
    assert state["blocks.0.conv.weight"].shape == (512, 24, 5)
    assert state["blocks.12.conv.weight"].shape == (1500, 512, 1)
    assert state["blocks.16.w.weight"].shape == (512, 3000)
    # BatchNorm statistics are not the identity: the folding is exercised
    for i in (2, 5, 8, 11, 14):
        assert (state[f"blocks.{i}.norm.running_mean"].abs() > 0.05).all()
        assert (state[f"blocks.{i}.norm.running_var"] - 1).abs().max() > 0.2


def test_loader_detects_the_checkpoint(state, tmp_path):
    assert type(models.EmbeddingLoader(state)()) is models.HipSbXvectorEmbedding
    assert type(models.EmbeddingLoader(state, arch="sb-xvector")()) is models.HipSbXvectorEmbedding
    # speechbrain's embedding_model.ckpt is a plain torch.save of the state dict
    ckpt = tmp_path / "embedding_model.ckpt"
    torch.save(state, ckpt)
    m = models.EmbeddingModel.from_pretrained(str(ckpt))
    m.load()
    assert type(m.model) is models.HipSbXvectorEmbedding
    assert m.model.dimension == 512 and m.model.precision in ("f16x3", "f32")
    assert models.HipSbXvectorEmbedding(state, precision="f32").precision == "f32"


def test_other_detection_unchanged():
    assert type(models.EmbeddingLoader(synth_ecapa_state())()) is models.HipEcapaEmbedding
    assert type(models.EmbeddingLoader(synth_wespeaker_state())()) is models.HipWeSpeakerEmbedding
    assert type(models.EmbeddingLoader(synth_embedding_state())()) is models.HipEmbedding


def test_abi_symbols_and_struct_size():
    lib = C.CDLL(str(_lib.lib_path()))
    for n in ("dz_sbx_abi_size", "dz_sbx_create", "dz_sbx_forward", "dz_sbx_forward_groups", "dz_sbx_peek",
              "dz_sbx_destroy"):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    # dft, dft_split, mel, 5 dz_layer of 5 pointers, lin_w, lin_b, zeros
    assert _lib.load().dz_sbx_abi_size() == C.sizeof(_lib.SbxWeights) == 8 * (3 + 5 * 5 + 3)


def test_min_num_samples_is_derived():
    assert R.min_num_samples() == R.MIN_NUM_SAMPLES == 480
    assert models.HipSbXvectorEmbedding.min_num_samples == R.MIN_NUM_SAMPLES


def test_restatement_shapes_and_too_short_rows(state):
    ref = R.SbXvectorRef(state)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 1, 4000, generator=g, dtype=torch.float64) * 0.1
    masks = torch.zeros(3, 50)
    masks[0] = 1.0
    masks[1, :10] = 1.0            # 800 samples: kept
    masks[2, :5] = 1.0             # 400 samples: too short -> NaN
    out = ref(x, masks)
    assert out.shape == (3, 512)
    assert torch.isfinite(out[:2]).all() and torch.isnan(out[2]).all()
    # every row too short: all NaN, nothing computed
    assert torch.isnan(ref(x, masks * 0 + (torch.arange(50) < 5).float())).all()


def test_reflect_padding_bounds_the_length(state):
    """At 479 samples (T = 3) the reference's reflect pad of 3 frames fails; at 480 (T = 4) it runs."""
    ref = R.SbXvectorRef(state)
    with pytest.raises(RuntimeError):
        ref.tdnn(R.fbank(torch.zeros(1, 479, dtype=torch.float64) + 0.01))
    assert torch.isfinite(ref.tdnn(R.fbank(torch.randn(1, 480, dtype=torch.float64)))[-1]).all()


def test_stats_pool_single_frame_and_noise_band():
    x = torch.randn(2, 10, 1500, dtype=torch.float64)
    rel = torch.tensor([1.0, 0.1], dtype=torch.float32)       # round(0.1 * 10) = 1 frame: std NaN, as torch.std
    p = R.stats_pool(x, rel, R.NOISE_MID)
    assert torch.allclose(p[0, :1500], x[0].mean(0) + 5e-5) and torch.isfinite(p[0]).all()
    assert torch.isnan(p[1, 1500:]).all() and torch.allclose(p[1, :1500], x[1, 0] + 5e-5)
    band = R.noise_band((64, 1500), torch.Generator().manual_seed(0))
    assert abs(band.min().item() - 1e-5) < 1e-15 and abs(band.max().item() - 9e-5) < 1e-15
