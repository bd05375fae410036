"""The float64 restatement of the config-3 embedding (oracle/ecapa_ref.py, ``dtype=torch.float64``) that the GPU
geometry tests measure the HIP path against: it agrees with the float32 restatement to fp32 round-off, and it
keeps the reference's float32 length arithmetic, so it selects the same frames — including at the lengths where
float32 and exact rounding part ways.  CPU only."""
import numpy as np
import pytest
import torch

from diart_amd.synth import synth_ecapa_state, synth_streams
from oracle.ecapa_ref import PretrainedSpeakerEmbeddingRef, frame_counts, rounding_edges

STAGES = ("feats", "block0", "mfa", "logits", "pooled", "emb")


def row_rel(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


@pytest.fixture(scope="module")
def oracles():
    sd = synth_ecapa_state()
    return PretrainedSpeakerEmbeddingRef(sd), PretrainedSpeakerEmbeddingRef(sd, dtype=torch.float64)


@pytest.mark.parametrize("lmax", [62340, 80000])
def test_rounding_edges_exist_and_float32_is_what_decides(lmax):
    """Every edge class is populated, and at the "differs" lengths the float32 frame counts are not the exact
    ones: a restatement that cast the relative lengths to float64 would select other frames there."""
    e = rounding_edges(lmax)
    T = e["T"]
    assert all(e[k] for k in ("int", "half", "near", "differs")), e
    lens = torch.tensor(sorted(set(e["int"] + e["half"] + e["near"] + e["differs"])))
    nvalid, nmask = frame_counts(lens.float() / lmax, T)
    v = np.float32(lens.numpy().astype(np.float32) / np.float32(lmax)) * np.float32(T)
    assert np.array_equal(nvalid.numpy(), np.rint(v).astype(np.int64))
    assert np.array_equal(nmask.numpy(), np.ceil(v).astype(np.int64))
    nv64, nm64 = torch.round(lens.double() / lmax * T).long(), torch.ceil(lens.double() / lmax * T).long()
    diff = torch.tensor([int(x) in set(e["differs"]) for x in lens])
    assert ((nvalid != nv64) | (nmask != nm64))[diff].all()
    # "differs" is complete: an exhaustive scan of [640, lmax] against exact rational rounding finds no other length
    every = np.arange(640, lmax + 1)
    v_all = (every.astype(np.float32) / np.float32(lmax)) * np.float32(T)
    num = every * T
    exact_ceil = -(-num // lmax)
    fl, rem2 = num // lmax, 2 * (num % lmax)
    exact_round = fl + ((rem2 > lmax) | ((rem2 == lmax) & (fl % 2 == 1)))
    scan = every[(np.rint(v_all).astype(np.int64) != exact_round) | (np.ceil(v_all).astype(np.int64) != exact_ceil)]
    assert scan.tolist() == e["differs"]
    frac = v - np.floor(v)
    assert (frac[np.isin(lens.numpy(), e["int"])] == 0).all() and (frac[np.isin(lens.numpy(), e["half"])] == 0.5).all()


def _batches():
    x = torch.from_numpy(synth_streams(4, 1.0, seed0=11))[:, None, :].contiguous()   # 16000 samples
    S = x.shape[-1]
    m = torch.zeros(4, S)                       # per-sample masks: exact kept lengths
    m[0, :8000] = 1.0
    m[1, 1000:5123] = 1.0
    m[2, :500] = 1.0                            # too short -> NaN row, rel = 1
    m[3, 3000:3800] = 1.0
    short = torch.zeros(3, S)                   # lmax = 640: T = 5, reflect padding at its limit
    short[0, :640] = 1.0
    short[1, 100:740] = 1.0
    short[2, 200:500] = 1.0
    return [(x[:2, :, :6400], None), (x, m), (x[:3], short)]


@pytest.mark.parametrize("case", range(3))
def test_float64_oracle_matches_float32_oracle(oracles, case):
    o32, o64 = oracles
    wav, masks = _batches()[case]
    g32, g64 = o32.geometry(wav, masks), o64.geometry(wav, masks)
    for k in ("lens", "nvalid", "nmask", "too_short"):
        assert torch.equal(g32[k], g64[k]), k
    assert g32["T"] == g64["T"]
    s32, s64 = o32.stages(g32), o64.stages(g64)
    assert s64["feats"].dtype == torch.float64 and s64["emb"].dtype == torch.float64
    ok = ~g32["too_short"]
    assert torch.isnan(s64["emb"][~ok]).all() and torch.isfinite(s64["emb"][ok]).all()
    nm = g32["nmask"]
    t = torch.arange(g32["T"])[None, :, None]
    errs = {}
    for k in STAGES:
        a, b = s32[k][ok], s64[k][ok]
        if k == "logits":                       # only the frames the softmax sees
            keep = (t < nm[ok][:, None, None]).to(b.dtype)
            a, b = a * keep, b * keep
        errs[k] = row_rel(a, b)
    print("float32 vs float64 oracle, worst row:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k in STAGES:                            # measured: <= 3.2e-6 (feats / block0), <= 1.9e-6 after
        assert errs[k] < 1e-5, (k, errs[k])
    # the public call is the same computation
    got = o64(wav, masks)
    assert np.array_equal(np.isnan(got), np.isnan(s64["emb"].numpy()))
    assert np.allclose(got[ok.numpy()], s64["emb"][ok].numpy(), rtol=0, atol=0)
