"""tests/xvector_ref.py on the CPU: run in float32 it is the oracle's XVectorSincNetRef, the float32 floor (e32) of every
case tests/test_gpu_xvector_f64.py gates, and that the measure catches each planted fault at the first exposed stage.
No GPU.  The input here is the oracle's float32 SincNet output; on the device it is the handle's own."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import xvector_ref as R  # noqa: E402

F32_ROUNDING = 2e-6            # five layers of float32 dot products in another order, the BatchNorm folded or not


@pytest.fixture(scope="module")
def oracle():
    from oracle.models_ref import XVectorSincNetRef
    m = XVectorSincNetRef().eval()
    m.load_state_dict(R._synth_state())
    return m


@pytest.fixture(scope="module")
def sincnet(oracle):
    """(P2, B) -> the oracle's float32 SincNet output (B, 60, P2), once per geometry"""
    cache = {}

    def get(P2, B):
        if (P2, B) not in cache:
            with torch.no_grad():
                cache[(P2, B)] = oracle.sincnet(R.audio(P2, B)[:, None, :])
            assert cache[(P2, B)].shape == (B, 60, P2)
        return cache[(P2, B)]
    return get


def test_geometry_is_the_library_s():
    from diart_amd import _lib
    lib = _lib.load()
    for P2 in sorted({g[0] for g in R.GEOMETRIES}):
        S = R.audio(P2, 1).shape[1]
        assert lib.dz_seg_frames_for(S) == P2 == R.seg_frames(S) and S % 4 == 0
        assert lib.dz_emb_frames_for(S) == R.valid_frames(P2)[4]
    S = R.samples_for(16)
    assert lib.dz_seg_frames_for(S - 4) == 15 and R.valid_frames(16) == [12, 8, 2, 2, 2]    # the shortest with two pooled frames
    assert R.valid_frames(293) == [289, 285, 279, 279, 279]
    # which geometries run tdnn5 with the pooling in its epilogue on the 256 compute units of the MI355X
    fused = [(P2, B) for P2, B in R.GEOMETRIES if R.fused_expected("f16x3", P2, B, 3)]
    assert fused == R.FUSED_GEOMETRIES and R.SPEAKER_GEOMETRY in fused and FUSED[:2] in fused
    assert not R.fused_expected("f16x3", 128, 10, 3) and not R.fused_expected("f16x3", 293, 7, 5)
    assert not any(R.fused_expected("f32", P2, B, 3) for P2, B in R.GEOMETRIES)
    for S in range(240, 6000, 7):
        assert lib.dz_seg_frames_for(S) == R.seg_frames(S), S


@pytest.mark.parametrize("P2,B", [(16, 3), (293, 2)])
def test_float32_restatement_is_the_oracle(oracle, sincnet, P2, B):
    x = sincnet(P2, B)
    p = R.params(dtype=R.F32)
    T = R.valid_frames(P2)[4]
    with torch.no_grad():
        frames = oracle.frames(R.audio(P2, B)[:, None, :])                   # (B, 1500, T)
    got = R.trunk(x, p)
    assert [got[k].shape[1] for k in R.LAYERS] == R.valid_frames(P2) and got["tdnn5"].dtype == torch.float32
    e = R.row_err(got["tdnn5"], frames.transpose(1, 2))
    print(f"\nP{P2}: frames {e:.2e}", end="")
    assert e <= F32_ROUNDING
    from oracle.models_ref import stats_pool_ref
    for K, mode in ((3, "linear"), (3, "nearest"), (None, "linear")):
        w = None if K is None else R.pool_weights(P2, B, K)
        h = R.head(got["tdnn5"], w, mode, p)
        with torch.no_grad():
            if K is None:
                pooled = stats_pool_ref(frames, None)
                emb = oracle(R.audio(P2, B)[:, None, :])
            else:
                pooled = stats_pool_ref(frames.repeat_interleave(K, 0), w.reshape(B * K, P2), interp_mode=mode)
                emb = oracle.forward_multi(R.audio(P2, B)[:, None, :], w.permute(0, 2, 1), interp_mode=mode).reshape(B * K, 512)
        # the std of the two-frame window carries the frames' rounding amplified by |x| / |x0 - x1|: held relative to
        # the pooled row (mean | std), as the Linear weighs it
        e = {"pooled": R.row_err(torch.cat([h["mean"], h["std"]], 1), pooled), "emb": R.row_err(h["emb"], emb)}
        e["mean"] = R.row_err(h["mean"], pooled[:, :1500])
        print(f"  K{K}-{mode} " + " ".join(f"{k} {v:.2e}" for k, v in e.items()), end="")
        assert T == (2 if P2 == 16 else 279)
        assert all(v <= F32_ROUNDING * (4 if T == 2 else 1) for v in e.values()), e
        assert torch.allclose(h["embn"].norm(dim=1), torch.ones(len(emb)), atol=1e-6)


@pytest.fixture(scope="module")
def cases(sincnet):
    """case -> R.Case on the oracle's SincNet output; one trunk per geometry"""
    trunks, out = {}, {}
    for c in R.case_list():
        P2, B, K, mode = c
        w = None if K is None else R.pool_weights(P2, B, K)
        if (P2, B) not in trunks:
            trunks[(P2, B)] = R.Case(sincnet(P2, B).double(), w, mode)
            out[c] = trunks[(P2, B)]
        else:
            out[c] = trunks[(P2, B)].with_head(w, mode)
    return out


def test_float32_floor_of_every_gpu_case(cases):
    """the e32 table: per stage, on every case the GPU test gates; no gate leaves what the embedding is held to already"""
    print("\n" + " " * 22 + " ".join(f"{s:>8}" for s in R.STAGES))
    for c, case in cases.items():
        print(f"{R.case_id(c):<22}" + " ".join(f"{case.e32[s]:8.1e}" for s in R.STAGES))
        for s in R.STAGES:
            assert case.e32[s] > 0 and R.gate(case.e32[s]) <= R.EMB_LIMIT, (c, s, case.e32[s])
        got = 1.0 - torch.nn.functional.cosine_similarity(case.f32["emb"].double(), case.ref["emb"], dim=1).min().item()
        assert got <= 1e-5 * 1e-3                                   # far inside cosine >= 0.99999


SMALLEST, FUSED = (16, 3, 3, "linear"), (128, R.MAX_BATCH, 3, "linear")


@pytest.mark.parametrize("fault", list(R.FAULTS), ids=[f"{n}-{i}" for n, i in R.FAULTS])
@pytest.mark.parametrize("geom", [SMALLEST, FUSED], ids=["P16", "P128"])
def test_measure_catches_the_planted_fault(cases, fault, geom):
    """each fault, planted into the float32 restatement, leaves its gate at the first stage the device exposes behind
    it (tdnn1 and tdnn2 are overwritten; where tdnn5 runs inside the pooling call, the pooled mean is that stage), on
    the smallest geometry and on the smallest fused one; every exposed stage in front of it stays inside"""
    case = cases[geom]
    w = R.pool_weights(*geom[:3])
    got = R.forward(case.x.float(), w, geom[3], R.params(dtype=R.F32), fault)
    stage = R.FAULTS[fault]
    err = {s: case.err(s, got[s]) for s in R.EXPOSED}
    print(f"\n{fault} P{geom[0]}: " + "  ".join(f"{s} {err[s]:.1e}/{case.gate(s):.1e}" for s in R.EXPOSED))
    for s in R.EXPOSED[:R.EXPOSED.index(stage)]:
        assert err[s] <= case.gate(s), (s, err[s])
    assert not err[stage] <= case.gate(stage), (stage, err[stage], case.gate(stage))
    if stage == "tdnn5":                          # fused: tdnn5 is not exposed, the pooled mean is
        assert not err["mean"] <= case.gate("mean"), (err["mean"], case.gate("mean"))
    if stage != "emb":                            # ... and it reaches the embedding
        assert not err["emb"] <= case.gate("emb"), (err["emb"], case.gate("emb"))


def test_sincnet_output_decodes_every_form():
    """``sincnet_output`` / ``decode_rows`` on buffers built here: planes, rows, raw + scale / shift, raw + partials"""
    from diart_amd.weights import kb_major, split_f16
    import front_ref
    g = torch.Generator().manual_seed(3)
    B, P2, nt = 2, 40, 2
    raw = torch.randn(B, P2, 64, generator=g)
    gamma, beta = torch.rand(60, generator=g) + 0.5, torch.randn(60, generator=g) * 0.1
    part = front_ref.tile_partials(raw.transpose(1, 2), 96, 3 * P2, torch.float32)        # (B, 2, 64, 2): 32 + 8 frames
    assert part.shape == (B, nt, 64, 2)
    sc, sh = front_ref.finalize_norm(part[:, :, :60], P2, gamma, beta)
    want = front_ref.activate(raw.double().transpose(1, 2)[:, :60], sc, sh)
    rec = dict(batch=B, P2=P2, nt2=nt, planes=1)
    sc64, sh64 = torch.zeros(B, 64), torch.zeros(B, 64)
    sc64[:, :60], sh64[:, :60] = sc.float(), sh.float()
    got2 = R.sincnet_output(dict(rec, form=2), raw.flatten(), sc64.flatten(), sh64.flatten())
    got3 = R.sincnet_output(dict(rec, form=3), raw.flatten(), part=part.flatten(), gamma=gamma, beta=beta)
    assert torch.equal(got3, want) and (got2 - want).abs().max() <= 1e-5
    norm = torch.zeros(B, P2, 64)
    norm[:, :, :60] = want.transpose(1, 2).float()
    got1 = R.sincnet_output(dict(rec, form=1), norm.flatten())
    planes = kb_major(split_f16(norm.view(B * P2, 64))).view(torch.float32).flatten()
    got0 = R.sincnet_output(dict(rec, form=0), planes)
    assert torch.equal(got1, norm[:, :, :60].transpose(1, 2).double())
    assert (got0 - got1).abs().max() <= got1.abs().max() * 2.0 ** -21
    assert torch.equal(R.decode_rows(rec, planes, 64)[:, :, :60], got0.transpose(1, 2))
    assert torch.equal(R.decode_rows(dict(rec, planes=0), norm.flatten(), 64), norm.double())
