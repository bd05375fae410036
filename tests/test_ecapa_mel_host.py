"""The mel-spectrogram ECAPA-TDNN's host side (no GPU): the restated front end against torch.stft, the packer's DFT
operand and mel bank against it and against the closed forms, the loader's recognition of the model, and the batch
geometry's arithmetic at hop 256."""
import math

import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd import weights as W
from diart_amd.synth import synth_ecapa_state

import ecapa_mel_ref as R


@pytest.fixture(scope="module")
def state():
    return synth_ecapa_state()


# --------------------------------------------------------------------------- #
# front end
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("L", [1024, 1279, 4000, 16000])
def test_restated_stft_is_torch_stft(L):
    x = torch.randn(3, L, dtype=torch.float64, generator=torch.Generator().manual_seed(L))
    want = torch.stft(x, n_fft=1024, hop_length=256, win_length=1024, window=torch.hann_window(1024, dtype=torch.float64),
                      center=True, pad_mode="reflect", return_complex=True).transpose(1, 2)
    got = R.stft(x)
    assert got.shape == want.shape == (3, 1 + L // 256, 513)
    assert (got - want).abs().max().item() < 1e-11 * math.sqrt(L)


def test_reflection_reads_the_rows_own_samples_near_the_end():
    """Index i >= L reads 2 (L - 1) - i: the last frame's right half is the mirror of the samples before L - 1."""
    L = 2048
    x = torch.arange(L, dtype=torch.float64)[None]
    fr = R.frames(x)[0]
    assert fr.shape == (9, 1024)
    assert fr[0, :513].tolist() == list(range(512, -1, -1))                 # i < 0 reads -i
    assert fr[8, 511:].tolist() == list(range(2047, 2047 - 513, -1))       # t = 8 starts at 1536: ... 2047, 2046, ...


def test_packed_dft_operand_reproduces_the_stft():
    x = torch.randn(2, 5000, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    d = W.ecapa_mel_spec_dft()
    assert d.shape == (1026, 1024) and d.dtype == torch.float64
    y = R.frames(x) @ d.t()
    want = R.stft(x)
    assert (y[..., :513] - want.real).abs().max().item() < 1e-10
    assert (y[..., 513:] + want.imag).abs().max().item() < 1e-10        # (the sine rows give -Im)
    # the imaginary rows of bins 0 and 512 are exact zeros, the window's first tap too
    assert not d[513].any() and not d[1025].any() and not d[:, 0].any()


def test_split_planes_hold_the_dft_operand():
    """The Hann window brings the operand's entries down to 1e-5: the (hi, lo) planes still represent the matrix to
    f32 grade (split_f16 measures it and refuses a layer beyond 2^-20)."""
    W.SPLIT_REPORT.clear()
    W.split_f16(W.ecapa_mel_spec_dft().float(), "dft")
    assert W.SPLIT_REPORT[-1][2] < 2.0 ** -21


# --------------------------------------------------------------------------- #
# slaney bank
# --------------------------------------------------------------------------- #
def test_slaney_bank_pins():
    fb = W.ecapa_mel_spec_filterbank()
    assert fb.shape == (80, 513) and fb.dtype == torch.float64
    assert torch.allclose(fb, R.mel_filterbank().t(), rtol=0, atol=1e-15)
    assert torch.equal(W.titanet_mel_filterbank(), W.slaney_mel_filterbank(80, 512, 16000, 0.0, 8000.0))
    # centre frequencies: linear below 1 kHz, log-spaced above it (closed form)
    top = 15.0 + 27.0 * math.log(8.0) / math.log(6.4)
    m = np.arange(82) * top / 81.0
    edges = np.where(m < 15.0, m * 200.0 / 3.0, 1000.0 * 6.4 ** ((m - 15.0) / 27.0))
    assert np.allclose(R.mel_points().numpy(), edges, rtol=1e-13)
    below = edges[edges < 1000.0]
    assert np.allclose(np.diff(below), below[1] - below[0], rtol=1e-12)
    above = edges[edges >= 1000.0]
    assert np.allclose(above[1:] / above[:-1], 6.4 ** (top / 81.0 / 27.0), rtol=1e-12)
    # a triangle of the continuous bank has unit area: its peak is 2 / width, where the sampled row has its maximum
    freqs = np.linspace(0.0, 8000.0, 513)
    for i in range(80):
        lo, c, hi = edges[i], edges[i + 1], edges[i + 2]
        tri = np.maximum(0.0, np.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c))) * 2.0 / (hi - lo)
        assert np.allclose(fb[i].numpy(), tri, rtol=1e-10, atol=1e-15)
        # (sampled every 15.625 Hz, a triangle at least two bins wide integrates to its area within the sampling error)
        assert abs(fb[i].sum().item() * 15.625 - 1.0) < 0.2
    # zero rows: none; zero columns: exactly the two band edges f_min = 0 (bin 0) and f_max = Nyquist (bin 512)
    assert (fb.sum(1) > 0).all()
    assert (fb.sum(0) == 0).nonzero().flatten().tolist() == [0, 512]


# --------------------------------------------------------------------------- #
# loader
# --------------------------------------------------------------------------- #
YAML = """# Feature parameters
sample_rate: 16000
n_fft: 1024
win_length: 1024
hop_length: {hop}
n_mel_channels: 80
mel_fmin: 0.0
mel_fmax: 8000.0
power: 1
mel_normalized: False
norm: "slaney"
mel_scale: "slaney"

compute_features: !name:speechbrain.lobes.models.HifiGAN.mel_spectogram
    sample_rate: !ref <sample_rate>
    hop_length: !ref <hop_length>
    n_mels: !ref <n_mel_channels>
mean_var_norm: !new:speechbrain.processing.features.InputNormalization
    norm_type: sentence
    std_norm: False
embedding_model: !new:speechbrain.lobes.models.ECAPA_TDNN.ECAPA_TDNN
    input_size: !ref <n_mel_channels>
"""


def _checkpoint(tmp_path, state, yaml=None):
    path = tmp_path / "embedding_model.ckpt"
    torch.save(state, path)
    if yaml is not None:
        (tmp_path / "hyperparams.yaml").write_text(yaml)
    return path


def test_loader_recognises_the_model_by_its_yaml(tmp_path, state):
    model = M.EmbeddingLoader(_checkpoint(tmp_path, state, YAML.format(hop=256)))()
    assert type(model) is M.HipEcapaMelEmbedding and model.dimension == 192
    assert model.min_num_samples == 1024 and model.features == W.ECAPA_MEL_FEATURES
    assert model.features["n_mels"] == 80 and model.features["f_max"] == 8000.0 and model.features["normalized"] is False


def test_loader_without_the_yaml_is_the_fbank_ecapa(tmp_path, state):
    assert type(M.EmbeddingLoader(_checkpoint(tmp_path, state))()) is M.HipEcapaEmbedding
    (tmp_path / "hyperparams.yaml").write_text("compute_features: !new:speechbrain.lobes.features.Fbank\n    n_mels: 80\n")
    assert type(M.EmbeddingLoader(tmp_path / "embedding_model.ckpt")()) is M.HipEcapaEmbedding


def test_loader_refuses_a_hop_the_kernels_are_not_built_for(tmp_path, state):
    with pytest.raises(ValueError, match="hop_length"):
        M.EmbeddingLoader(_checkpoint(tmp_path, state, YAML.format(hop=160)))()
    with pytest.raises(ValueError, match="n_fft"):
        M.EmbeddingLoader(state, arch="ecapa-mel", n_fft=512)()
    with pytest.raises(ValueError, match="min_num_samples"):
        M.EmbeddingLoader(state, arch="ecapa-mel", min_num_samples=512)()


def test_loader_options_override_the_yaml(tmp_path, state):
    model = M.EmbeddingLoader(_checkpoint(tmp_path, state, YAML.format(hop=160)), hop_length=256, min_num_samples=2048,
                              f_max=7600.0)()
    assert type(model) is M.HipEcapaMelEmbedding
    assert model.min_num_samples == 2048 and model.features["f_max"] == 7600.0


def test_plain_dict(state):
    assert type(M.EmbeddingLoader(state)()) is M.HipEcapaEmbedding           # arch=None: "ecapa" exactly as before
    model = M.EmbeddingLoader(state, arch="ecapa-mel")()
    assert type(model) is M.HipEcapaMelEmbedding
    assert type(M.EmbeddingModel.from_state(state, arch="ecapa-mel").get_model()) is M.HipEcapaMelEmbedding
    with pytest.raises(ValueError, match="share"):
        M.EmbeddingLoader(state, arch="ecapa-mel", repeated_rows="share")()
    with pytest.raises(TypeError, match="hop_length"):
        M.EmbeddingLoader(state, arch="ecapa", hop_length=256)()


def test_model_pickles_with_its_options(state):
    import pickle
    model = M.HipEcapaMelEmbedding(state, precision="f32", min_num_samples=1280, f_min=20.0)
    again = pickle.loads(pickle.dumps(model))
    assert again.min_num_samples == 1280 and again.features == model.features and again.precision == "f32"


# --------------------------------------------------------------------------- #
# batch geometry at hop 256
# --------------------------------------------------------------------------- #
def _kernel_arithmetic(lens, min_num_samples=1024):
    """ecapa_geometry_kernel's float32 arithmetic (k_ecapa.hip) at hop 256, in numpy."""
    lens = np.asarray(lens)
    lmax = int(lens.max())
    if lmax < min_num_samples:
        z = np.zeros(len(lens), dtype=np.int64)
        return 0, z, z
    T = 1 + lmax // 256
    rel = np.where(lens < min_num_samples, np.float32(1), lens.astype(np.float32) / np.float32(lmax)).astype(np.float32)
    v = rel * np.float32(T)
    assert v.dtype == np.float32
    return T, np.clip(np.rint(v), 1, T).astype(np.int64), np.clip(np.ceil(v), 1, T).astype(np.int64)


@pytest.mark.parametrize("lmax", [1024, 1025, 1279, 1280, 15360, 16000])
def test_geometry_arithmetic(lmax):
    lens = [l for l in (1023, 1024, 1025, 1279, 1280) if l <= lmax] + [lmax]
    g = R.geometry_of_lengths(lens)
    T, nvalid, nmask = _kernel_arithmetic(lens)
    assert g["T"] == T == 1 + lmax // 256 >= 5
    assert g["too_short"].tolist() == [l < 1024 for l in lens]
    assert g["nvalid"].tolist() == nvalid.tolist() and g["nmask"].tolist() == nmask.tolist()
    assert g["nvalid"][-1] == g["nmask"][-1] == T                             # the longest row has every frame
    if 1023 in lens:
        assert g["nvalid"][0] == T                                            # a too-short row counts as full
    assert R.geometry_of_lengths([1023, 600])["T"] == 0                       # every row too short: no frames


def test_frames_for_the_minimum():
    """1024 is the shortest signal with the 5 frames the dilation-4 reflect padding needs, and longer than the STFT's 512."""
    assert 1 + 1023 // 256 == 4 and 1 + 1024 // 256 == 5 and R.MIN_NUM_SAMPLES == W.ECAPA_MEL_MIN_NUM_SAMPLES == 1024


@pytest.mark.parametrize("lmax", [15360, 16000])
def test_rounding_edges_at_hop_256(lmax):
    e = R.rounding_edges(lmax)
    assert e["T"] == 1 + lmax // 256
    edges = sorted(set(e["half"] + e["differs"] + e["near"] + e["int"][:4]))
    assert e["half"], "no half-integer edge to test torch.round's half-to-even at"
    g = R.geometry_of_lengths(edges + [lmax])
    _, nvalid, nmask = _kernel_arithmetic(edges + [lmax])
    assert g["nvalid"].tolist() == nvalid.tolist() and g["nmask"].tolist() == nmask.tolist()
    for l in e["half"]:            # on k + 0.5 the count is the EVEN neighbour
        v = np.float32(l) / np.float32(lmax) * np.float32(e["T"])
        i = (edges + [lmax]).index(l)
        assert int(g["nvalid"][i]) % 2 == 0 and abs(int(g["nvalid"][i]) - float(v)) == 0.5
        assert int(g["nmask"][i]) == math.ceil(float(v))
