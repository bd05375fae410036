"""The mel-spectrogram ECAPA-TDNN (``HipEcapaMelEmbedding``) against its float64 restatement
(tests/ecapa_mel_ref.py), stage by stage through ``dz_ecm_peek``: 2 groups x 3 rows of 16 000 samples (63 frames), both
precisions.  The masks are per-sample, so the kept lengths are exact:

  group 0 (Lmax 16000, T 63): the full row | exactly 1024, every kept sample zero | 1023: too short, NaN
  group 1 (Lmax 15360, T 61): 15360, a multiple of 256 | 7680: float32(len / Lmax) * T = 30.5, the half-to-even edge,
      at amplitude 1e-3 | 15260 > Lmax - 512: its own samples appear in the right reflection

Gates.  Block 0, MFA, the pooled statistics and the embedding: the thresholds tests/test_gpu_ecapa.py applies to the same
stages of the same network (2e-5, 1e-4, 1e-4, 2e-4 relative L2; cosine > 0.99999).  Magnitude spectrum and log-mel
features: 10 x the deviation of the restatement evaluated in float32 by torch on the CPU from its float64 self on the
same inputs (the worst row of the case), relative L2 per row over its valid frames for the spectrum and max-abs for
the features — a 1024-term GEMM accumulation against an FFT's error growth, and the log turning relative error into
absolute error near the clamp.  Measured on an MI355X (worst row; yardstick = float32 torch):
  spectrum  f16x3 1.85e-7, f32 4.82e-7, yardstick 1.13e-7 (gate 1.13e-6)
  features  f16x3 2.63e-6, f32 2.63e-6, yardstick 1.39e-5 (gate 1.39e-4)"""
import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.synth import synth_ecapa_state

import ecapa_mel_ref as R

pytestmark = pytest.mark.gpu

S, K, TC = 16000, 3, 63
LENS = [[16000, 1024, 1023], [15360, 7680, 15260]]
START = [[0, 2000, 9000], [0, 0, 100]]          # first kept sample of each row (a contiguous run)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def bits(t):
    return t.contiguous().view(torch.int32)


def make_inputs(nan_at=None):
    """waves (2, S) float32, masks (2, 3, S): row (g, k) keeps LENS[g][k] samples from START[g][k] on."""
    g = torch.Generator().manual_seed(11)
    waves = 0.1 * torch.randn(2, S, generator=g)
    waves[0, 2000:3024] = 0.0                    # what row (0, 1) keeps: all zero
    waves[1, :7680] *= 0.01                      # what row (1, 1) keeps: amplitude 1e-3
    if nan_at is not None:
        waves[nan_at[0], nan_at[1]] = float("nan")
    masks = torch.zeros(2, K, S)
    for gi in range(2):
        for k in range(K):
            masks[gi, k, START[gi][k]:START[gi][k] + LENS[gi][k]] = 1.0
    return waves, masks


@pytest.fixture(scope="module")
def ref():
    return R.MelSpecEmbeddingRef(synth_ecapa_state(), dtype=torch.float64)


def reference(ref, waves, masks):
    """Per group: the geometry, the float64 stages, and the float32 restatement's spectrum and features."""
    out = []
    for gi in range(waves.shape[0]):
        x = waves[gi][None, None, :].repeat(K, 1, 1)
        geom = ref.geometry(x, masks[gi])
        st = ref.stages(geom)
        sig32 = geom["signals"].float()
        st["mag32"] = R.magnitude(sig32)
        st["feats32"] = R.sentence_mean_norm(R.log_mel(sig32), geom["rel"])
        out.append((geom, st))
    return out


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


@pytest.fixture(scope="module")
def want(ref, inputs):
    return reference(ref, *inputs)


@pytest.fixture(scope="module", params=["f16x3", "f32"])
def hip(gpu, request):
    return M.HipEcapaMelEmbedding(synth_ecapa_state(), max_batch=2 * K, precision=request.param).to(gpu)


def run_groups(hip, gpu, waves, masks):
    emb = hip.forward_groups(waves[:, None, :].to(gpu), masks.to(gpu)).cpu()
    peek = lambda which, width=None: (hip.peek(S, which)[0].cpu().view(2 * K, TC, width) if width else
                                      hip.peek(S, which)[0].cpu())
    return emb, peek


def test_geometry_is_exactly_the_restatements(gpu, hip, inputs, want):
    assert hip.num_frames(S) == TC
    _, peek = run_groups(hip, gpu, *inputs)
    assert hip.last_frames(S) == TC
    lens, nvalid, nmask, T, lmax = (peek(w).tolist() for w in (5, 6, 7, 8, 9))
    assert lens == LENS[0] + LENS[1]
    for gi, (geom, _) in enumerate(want):
        rows = slice(gi * K, (gi + 1) * K)
        assert geom["lens"].tolist() == LENS[gi]
        assert lmax[rows] == [max(LENS[gi])] * K and T[rows] == [geom["T"]] * K
        assert nvalid[rows] == geom["nvalid"].tolist() and nmask[rows] == geom["nmask"].tolist()
    assert T[0] == 63 and T[3] == 61
    assert nvalid[4] == 30 and nmask[4] == 31            # 30.5: round to even, ceil
    assert nvalid[2] == 63                               # the too-short row counts as full


def test_stages_against_float64(gpu, hip, inputs, want):
    emb, peek = run_groups(hip, gpu, *inputs)
    mag, feats = peek(10, 544), peek(0, 80)
    b0, mfa, pooled = peek(1, 1024), peek(3, 3072), peek(4).view(2 * K, 6144)
    assert not mag[:, :, 513:].any()
    spec_err, spec_yard, feat_err, feat_yard = [], [], [], []
    for gi, (geom, st) in enumerate(want):
        T = geom["T"]
        for k in range(K):
            r, nv = gi * K + k, int(geom["nvalid"][k])
            if st["mag"][k, :nv].norm() == 0:                                  # the all-zero row: exact zeros
                assert not mag[r, :nv, :513].any()
            else:
                spec_err.append(rel(mag[r, :nv, :513], st["mag"][k, :nv]))
                spec_yard.append(rel(st["mag32"][k, :nv], st["mag"][k, :nv]))
            feat_err.append((feats[r, :T].double() - st["feats"][k]).abs().max().item())
            feat_yard.append((st["feats32"][k].double() - st["feats"][k]).abs().max().item())
        rows = slice(gi * K, (gi + 1) * K)
        assert rel(b0[rows, :T], st["block0"]) < 2e-5
        assert rel(mfa[rows, :T], st["mfa"]) < 1e-4
        assert rel(pooled[rows], st["pooled"]) < 1e-4
        ok = ~geom["too_short"]
        assert torch.equal(torch.isnan(emb[gi]).any(dim=1), geom["too_short"])
        assert rel(emb[gi][ok], st["emb"][ok]) < 2e-4
        cos = torch.nn.functional.cosine_similarity(emb[gi][ok].double(), st["emb"][ok], dim=-1)
        assert cos.min().item() > 0.99999
    assert torch.isfinite(emb[0, 1]).all()                                     # the all-zero row is finite
    print(f"ecapa-mel {hip.precision}: spectrum rel L2 worst {max(spec_err):.3e} (float32 torch {max(spec_yard):.3e}), "
          f"features max-abs worst {max(feat_err):.3e} (float32 torch {max(feat_yard):.3e})")
    assert max(spec_err) <= 10 * max(spec_yard)
    assert max(feat_err) <= 10 * max(feat_yard)


def test_groups_rows_are_the_single_group_forward(gpu, hip, inputs):
    waves, masks = inputs
    emb, _ = run_groups(hip, gpu, waves, masks)
    for gi in range(2):
        x = waves[gi][None, None, :].repeat(K, 1, 1)
        one = hip(x.to(gpu), masks[gi].to(gpu)).cpu()
        assert torch.equal(bits(one), bits(emb[gi]))


def test_all_too_short_call_is_all_nan(gpu, hip, inputs):
    waves, _ = inputs
    masks = torch.zeros(1, K, S)
    masks[0, 0, :1023] = 1.0
    masks[0, 1, 5000:5600] = 1.0
    emb = hip.forward_groups(waves[:1, None, :].to(gpu), masks.to(gpu)).cpu()
    assert emb.shape == (1, K, 192) and torch.isnan(emb).all()
    assert hip.peek(S, 5)[0].tolist() == [1023, 600, 0]
    assert not any(hip.peek(S, w)[0].any() for w in (6, 7, 8))
    one = hip(waves[:1, None, :].repeat(K, 1, 1).to(gpu), masks[0].to(gpu)).cpu()
    assert torch.isnan(one).all()


def test_a_kept_nan_sample_is_a_nan_row_and_moves_nobody(gpu, hip, inputs):
    """Sample 15990 of chunk 0 is kept by the full row alone: that row is NaN, keeps its place in the geometry (it
    stays the group's longest row), and every other row keeps its bits."""
    clean, _ = run_groups(hip, gpu, *inputs)
    waves, masks = make_inputs(nan_at=(0, 15990))
    emb, peek = run_groups(hip, gpu, waves, masks)
    assert torch.isnan(emb[0, 0]).all() and torch.isfinite(emb[0, 1]).all() and torch.isnan(emb[0, 2]).all()
    assert peek(5).tolist() == [-(16000 + 1)] + LENS[0][1:] + LENS[1]
    assert peek(8).tolist() == [63] * 3 + [61] * 3
    assert torch.equal(bits(emb[0, 1]), bits(clean[0, 1])) and torch.equal(bits(emb[1]), bits(clean[1]))


def test_neither_precision_moves_the_other(gpu, inputs):
    waves, masks = inputs
    sd = synth_ecapa_state()
    a = M.HipEcapaMelEmbedding(sd, max_batch=2 * K, precision="f16x3").to(gpu)
    b = M.HipEcapaMelEmbedding(sd, max_batch=2 * K, precision="f32").to(gpu)
    run = lambda m: bits(m.forward_groups(waves[:, None, :].to(gpu), masks.to(gpu)).cpu())
    a1, b1, a2, b2 = run(a), run(b), run(a), run(b)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)
    assert not torch.equal(a1, b1)                       # (two arithmetics, not one)
