"""WeSpeaker ResNet34 (pyannote/wespeaker-voxceleb-resnet34-LM) without a GPU: checkpoint detection and loading, the
folded-BatchNorm packing, the kaldi mel bank, the frame arithmetic of every stage and the C ABI of dz_wsp_*."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import wespeaker_ref as R
from diart_amd import _lib, checkpoint, models
from diart_amd.synth import synth_ecapa_state, synth_embedding_state, synth_segmentation_state, synth_wespeaker_state
from diart_amd.weights import fold_conv_bn, kaldi_mel_banks, wsp_conv_matrix


def test_loader_detects_wespeaker_and_keeps_the_other_archs():
    assert isinstance(models.EmbeddingLoader(synth_wespeaker_state())(), models.HipWeSpeakerEmbedding)
    m = models.EmbeddingLoader(synth_wespeaker_state(), arch="wespeaker", precision="f32")()
    assert isinstance(m, models.HipWeSpeakerEmbedding) and m.dimension == 256 and m.precision == "f32"
    assert isinstance(models.EmbeddingLoader(synth_ecapa_state())(), models.HipEcapaEmbedding)
    xv = models.EmbeddingLoader(synth_embedding_state())()
    assert type(xv) is models.HipEmbedding and xv.weight_interp == "linear"
    # an explicit arch still wins over the keys
    assert type(models.EmbeddingLoader(synth_embedding_state(), arch="xvector")()) is models.HipEmbedding


def test_lightning_checkpoint_loads_through_read_state(tmp_path):
    sd = synth_wespeaker_state(seed=3)
    ckpt = {"epoch": 7, "pytorch-lightning_version": "2.1.0", "state_dict": dict(sd),
            "pyannote.audio": {"versions": {"pyannote.audio": "3.1.0", "torch": "2.1.1"},
                               "architecture": {"module": "pyannote.audio.models.embedding.wespeaker.resnet",
                                                "class": "WeSpeakerResNet34"}},
            "hyper_parameters": {"sample_rate": 16000, "num_channels": 1}}
    f = tmp_path / "wespeaker.ckpt"
    torch.save(ckpt, f)
    got = checkpoint.read_state(f)
    assert set(got) == set(sd)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    m = models.EmbeddingLoader(str(f))()
    assert isinstance(m, models.HipWeSpeakerEmbedding)


@pytest.mark.parametrize("key", ["resnet.conv1", "resnet.layer1.2.conv2", "resnet.layer3.0.conv1",
                                 "resnet.layer3.0.shortcut"])
def test_folded_bn_equals_conv_then_bn_in_float64(key):
    sd = {k: v.double() for k, v in synth_wespeaker_state().items()}
    if key.endswith("shortcut"):
        w, bn, stride, pad = sd[key + ".0.weight"], key + ".1", 2, 0
    else:
        w, stride, pad = sd[key + ".weight"], 1, 1
        bn = key.rsplit(".", 1)[0] + "." + key.rsplit(".", 1)[1].replace("conv", "bn")
    p = {n: sd[f"{bn}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")}
    x = torch.randn(2, w.shape[1], 12, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = F.batch_norm(F.conv2d(x, w, stride=stride, padding=pad), p["running_mean"], p["running_var"], p["weight"],
                        p["bias"], training=False, eps=1e-5)
    fw, fb = fold_conv_bn(w, p)
    got = F.conv2d(x, fw, fb, stride=stride, padding=pad)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # the packed matrix: k = (kh 3 + kw) Cin + c over channels-last im2col rows
    m = wsp_conv_matrix(fw)
    kh = w.shape[2]
    xl = F.pad(x, (pad, pad, pad, pad)).permute(0, 2, 3, 1)             # (N, F, T, C)
    Fo, To = got.shape[2], got.shape[3]
    cols = []
    for a in range(kh):
        for b in range(kh):
            cols.append(xl[:, a: a + stride * (Fo - 1) + 1: stride, b: b + stride * (To - 1) + 1: stride, :])
    im2col = torch.cat(cols, dim=-1)                                     # (N, Fo, To, taps Cin)
    assert torch.allclose(im2col @ m.t() + fb, got.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_kaldi_mel_bank():
    mb = kaldi_mel_banks()
    assert mb.shape == (80, 257) and mb.dtype == torch.float64
    assert torch.all(mb[:, 256] == 0)                                    # the Nyquist column
    assert torch.all(mb >= 0) and torch.all(mb <= 1)
    assert torch.allclose(mb, R.mel_banks(), rtol=0, atol=1e-12)        # the restatement's own construction
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo, hi = mel(20.0), mel(8000.0)
    d = (hi - lo) / 81
    bin_mel = torch.tensor([mel(31.25 * k) for k in range(256)], dtype=torch.float64)
    for b in range(80):
        row = mb[b, :256]
        nz = torch.nonzero(row).flatten()
        assert len(nz) >= 1
        peak = int(torch.argmax(row))
        # rises to its peak, then falls (a triangle sampled on the FFT bins)
        assert torch.all(row[nz[0]: peak + 1].diff() >= 0) and torch.all(row[peak: nz[-1] + 1].diff() <= 0)
        l, c, r = lo + b * d, lo + (b + 1) * d, lo + (b + 2) * d
        assert torch.all((bin_mel[nz] > l) & (bin_mel[nz] < r))          # support strictly inside (left, right)
        tri = lambda m: max(0.0, min((m - l) / (c - l), (r - m) / (r - c)))
        assert tri(c) == 1.0                                             # the triangle peaks at 1 on its centre
        assert abs(float(row[peak]) - tri(float(bin_mel[peak]))) < 1e-12


@pytest.mark.parametrize("S", [80000, 32000, 79760, 400 + 160 * 124, 401, 16000 * 3 + 37])
def test_frames_per_stage(S):
    lib = _lib.load()
    got = [lib.dz_wsp_frames_for(S, s) for s in range(5)]
    assert got == R.frames(S)
    T = 1 + (S - 400) // 160
    x = torch.zeros(1, 1, 80, T)
    shapes = [T, T]
    for _ in range(3):
        x = F.conv2d(x[:, :1], torch.zeros(1, 1, 3, 3), stride=2, padding=1)
        shapes.append(x.shape[-1])
        assert F.conv2d(torch.zeros(1, 1, 80, shapes[-2]), torch.zeros(1, 1, 1, 1), stride=2).shape[-1] == shapes[-1]
    assert got == shapes
    assert lib.dz_wsp_frames_for(399, 0) == 0 and lib.dz_wsp_frames_for(S, 5) == -1


def test_odd_frames_at_every_stage_exist():
    """79760 samples: 497 -> 497 -> 249 -> 125 -> 63 frames, odd at every stride (the GPU tests use it)."""
    got = [_lib.load().dz_wsp_frames_for(79760, s) for s in range(5)]
    assert got == [497, 497, 249, 125, 63] and all(t % 2 == 1 for t in got)


def test_abi_symbols_and_struct_size():
    lib = C.CDLL(str(_lib.lib_path()))
    for n in ("dz_wsp_abi_size", "dz_wsp_frames_for", "dz_wsp_create", "dz_wsp_forward", "dz_wsp_forward_multi",
              "dz_wsp_peek", "dz_wsp_destroy", "dz_k_conv2d"):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert _lib.load().dz_wsp_abi_size() == C.sizeof(_lib.WspWeights) == 8 + 24 + 16 * 3 * 24 + 16
    # the existing five-struct check is untouched
    assert len(_lib.SIGNATURES["dz_abi_struct_sizes"][1]) == 1


def test_stream_batch_refuses_wespeaker():
    from diart_amd.pipeline import StreamBatch
    seg = models.HipSegmentation(synth_segmentation_state())
    emb = models.HipWeSpeakerEmbedding(synth_wespeaker_state())
    with pytest.raises(ValueError, match="HipEmbedding.*HipEcapaEmbedding"):
        StreamBatch(seg, emb, 2)


# --------------------------------------------------------------------------- #
# the GPU tests' own references, checked on the CPU
# --------------------------------------------------------------------------- #
def test_conv_restatement_equals_conv2d_in_float64():
    """tests/test_gpu_conv2d.py's implicit GEMM (im2col rows in the kernels' k order times the test's own matrix, then
    bias, residual, ReLU) is F.conv2d in float64 on every geometry the GPU test runs."""
    from test_gpu_conv2d import CASES, EPI, _operands
    for case in CASES:
        B, Fi, Ti, cin, cout, taps, stride, epi = case
        x, w4, m, b, r = _operands(case)
        want, scale = R.conv_ref(x, w4, b, r, EPI[epi][1], stride)
        y = R.im2col(x.double(), taps, stride) @ m.double().t() + b.double()
        if r is not None:
            y = y + r.double()
        if EPI[epi][1]:
            y = F.relu(y)
        assert y.shape == want.shape, case
        assert ((y - want).abs() / scale).max().item() < 1e-13, case


def test_single_frame_pooling_denominator_is_negative_in_float32():
    """pyannote.audio 3.1's StatsPool with one non-zero weight w: v1 = w + 1e-8, var = 0 / (v1 - w^2 / v1 + 1e-8).  In
    float64 the denominator is 1e-8 + O(1e-16) > 0; in float32 w + 1e-8 rounds to w (for w > ~0.17) and w^2 / w may
    round to w plus one ulp: the denominator is then 1e-8 - ulp(w) < 0 and sqrt gives NaN.  This happens for a few
    percent of w; w = 1.0 (min-max normalised) is exact and gives std 0."""
    w = torch.linspace(0.01, 1.0, 100000, dtype=torch.float32)
    v1 = w + 1e-8
    den = v1 - w * w / v1 + 1e-8
    neg = den < 0
    frac = neg.float().mean().item()
    assert 0.005 < frac < 0.1, frac
    w64 = w[neg].double()
    v64 = w64 + 1e-8
    assert (v64 - w64 * w64 / v64 + 1e-8 > 0).all()                    # float64: positive wherever float32 is negative
    one = torch.tensor([1.0])
    v1 = one + 1e-8
    assert v1.item() == 1.0 and (v1 - one * one / v1 + 1e-8).item() > 0


def test_gates_see_planted_mistakes():
    """Each of three mistakes moves the float64 reference past the new gates: a periodic Hamming window (/ 400 instead of
    / 399), the split-f16 cross products without their 2^-11, and the time padding shifted by one column."""
    from test_gpu_conv2d import CASES, EPI, GATE, _operands
    from test_gpu_wespeaker import ROW_GATES, case_inputs, rel
    fb_gate = max(g["fbank"] for g in ROW_GATES.values())
    # 1. window: the power-domain fbank measure, per row, on the stage test's 2 s rows
    x, _ = case_inputs(32000, 293)
    want, scale = R.fbank_raw(x)
    bad, _ = R.fbank_raw(x, window_div=400)
    err = ((bad.exp() - want.exp()).abs() / scale[..., None]).reshape(x.shape[0], -1).amax(dim=1)
    old = rel(R.fbank(x, window_div=400), R.fbank(x))
    print(f"periodic window: fbank {err.min().item():.2e} (gate {fb_gate:.1e}); old whole-tensor rel L2 {old:.2e}")
    assert err.min().item() > fb_gate
    c_gate = max(GATE.values())
    for case in CASES[:4] + CASES[-4:]:
        B, Fi, Ti, cin, cout, taps, stride, epi = case
        xs, w4, m, b, r = _operands(case)
        relu = EPI[epi][1]
        want, scale = R.conv_ref(xs, w4, b, r, relu, stride)

        def finish(y):
            y = y + b.double() + (r.double() if r is not None else 0.0)
            return F.relu(y) if relu else y
        cols = R.im2col(xs.double(), taps, stride)
        # 2. the (lo hi + hi lo) products added without their 2^-11
        xh = cols.float().half().double()
        xl = ((cols.float() - xh.float()) * 2048).half().double()
        wp = R.split_planes(m).view(torch.float16).double()
        y = finish(xh @ wp[0].t() + (xl @ wp[0].t() + xh @ wp[1].t()))
        e2 = ((y - want).abs() / scale).max().item()
        o2 = rel(y, want)
        # 3. the time padding one column to the right (3x3 only)
        e3 = o3 = float("inf")
        if taps == 9:
            y = finish(R.im2col(xs.double(), taps, stride, tpad=(0, 2)) @ m.double().t())
            e3, o3 = ((y - want).abs() / scale).max().item(), rel(y, want)
        print(f"{case}: no 2^-11 {e2:.2e} (old {o2:.2e}); shifted padding {e3:.2e} (old {o3:.2e})")
        assert e2 > c_gate and e3 > c_gate, case
