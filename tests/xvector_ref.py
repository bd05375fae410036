"""The pyannote x-vector behind its SincNet — five TDNN layers, weighted statistics pooling, Linear(3000, 512), L2
normalisation — restated as plain tensor code in float64 (and float32), the measure its device stages are held to, the
planted faults that measure must catch, and the cases of tests/test_xvector_ref_host.py and
tests/test_gpu_xvector_f64.py.  Plain torch on the CPU; the pooling is tests/pool_ref.py's.

The input is the last SincNet stage AFTER its InstanceNorm and LeakyReLU, (B, 60, P2): on the device the handle's own
(``dz_emb_peek`` buffer 0, converted to float64 — ``sincnet_output``), on the CPU the oracle's float32 one.  The front
end has its own float64 test (tests/test_gpu_front_f64.py); its float32-against-float64 conditioning (1.5e-4 at this
point) would drown the trunk, which is why tests/lstm_ref.py::stack_reference_f64 starts behind it too.

Layer i: conv1d(dilation) -> leaky_relu(0.01) -> y * scale + shift, (scale, shift) the eval-mode BatchNorm folded as the
product folds it: 60 -> 512 k5 d1, 512 -> 512 k3 d2, 512 -> 512 k3 d3, 512 -> 512 k1, 512 -> 1500 k1.  A chunk of P2
frames keeps T = P2 - 4, - 8, - 14, - 14, - 14 frames.

The measure, one for every stage: relative L2 per ROW against float64, the worst row of the case — a row is one frame
of one chunk (512 or 1500 channels) for the layers, one (chunk, speaker) for the pooled mean, the pooled std and the
embedding.  Every valid frame t < T of every chunk counts; nothing is excluded.  The gate is pool_ref's:
max(1e-6, 4 e32), e32 the same measure of this restatement run in float32 on the same input (``Case.e32``) — the 22
operand bits of f16x3 against float32's 24, one rule for both precisions.  No gate may exceed EMB_LIMIT = 1e-4, what
tests/test_gpu_models.py asks of the embedding.
"""
import functools
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import front_ref  # noqa: E402
import pool_ref  # noqa: E402

F64, F32 = torch.float64, torch.float32
TDNN = [(60, 512, 5, 1), (512, 512, 3, 2), (512, 512, 3, 3), (512, 512, 1, 1), (512, 1500, 1, 1)]   # cin, cout, taps, dilation
SLOPE, BN_EPS = 0.01, 1e-5
SPLIT_K, POOL_LD = 16, 3008                  # the device's Linear(3000, 512): 16 slices of the 3008-column pooled row
EMB_LIMIT = 1e-4
LAYERS = ["tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5"]
HEAD = ["mean", "std", "emb", "embn"]
STAGES = LAYERS + HEAD
EXPOSED = ["tdnn3", "tdnn4", "tdnn5", "mean", "std", "emb", "embn"]       # what dz_emb_peek and the call's output show

gate = pool_ref.gate


def valid_frames(P2):
    """T[0 .. 4]: valid frames per chunk behind tdnn1 .. tdnn5"""
    out, t = [], P2
    for _, _, taps, dil in TDNN:
        t -= (taps - 1) * dil
        out.append(t)
    return out


def seg_frames(S):
    """frames of the SincNet output for S samples (the rule of dz_seg_frames_for), 0 when too short"""
    if S < 251:
        return 0
    t = ((S - 251) // 10 + 1) // 3
    for _ in range(2):
        t = (t - 4) // 3 if t > 4 else 0
    return t


def samples_for(P2):
    """the smallest sample count, a multiple of 4 (the row stride of a batch), whose window has P2 SincNet frames"""
    S = ((3 * (3 * (3 * P2 + 4) + 4)) - 1) * 10 + 251
    S += -S % 4
    assert seg_frames(S) == P2 and seg_frames(S - 4) < P2, (P2, S)
    return S


# --------------------------------------------------------------------------- the network
@functools.lru_cache(maxsize=None)
def _synth_state():
    from diart_amd.synth import synth_embedding_state
    return synth_embedding_state()


def params(sd=None, dtype=F64):
    """the state dict as the operands of the restatement, in `dtype`: per layer w (cout, cin, taps), b, scale, shift;
    the Linear's lw (512, 3000), lb"""
    sd = _synth_state() if sd is None else sd
    g = lambda k: sd[k].detach().to(dtype)
    p = dict(w=[], b=[], scale=[], shift=[], lw=g("embedding.weight"), lb=g("embedding.bias"), dtype=dtype)
    for i in range(5):
        bn = f"tdnns.{3 * i + 2}."
        scale = g(bn + "weight") / torch.sqrt(g(bn + "running_var") + BN_EPS)
        p["w"].append(g(f"tdnns.{3 * i}.weight"))
        p["b"].append(g(f"tdnns.{3 * i}.bias"))
        p["scale"].append(scale)
        p["shift"].append(g(bn + "bias") - g(bn + "running_mean") * scale)
    return p


def layer(x, p, i, fault=None):
    """x (B, cin, T) -> (B, cout, T - (taps - 1) dil).  ``fault``: None or (name, layer index) — see FAULTS"""
    _, _, taps, dil = TDNN[i]
    reach = (taps - 1) * dil
    T = x.shape[2] - reach
    w, shift = p["w"][i], p["shift"][i]
    name = fault[0] if fault is not None and fault[1] == i else None
    if name == "dilation":                       # one dilation less: the taps sit at 0, d - 1, 2 (d - 1)
        dil -= 1
    elif name == "cross_chunk":                  # the input packed at the OUTPUT's frame count: the last `reach` valid
        x = torch.cat([x[:, :, :T], x.roll(-1, 0)[:, :, :reach]], 2)      # frames read the next chunk's first frames
    elif name == "low_plane":                    # both operands lost their low plane: 11 bits
        x, w = front_ref.round_f16(x), front_ref.round_f16(w)
    elif name == "shift_tail":                   # the last, partly filled 64-column block of the 1500 channels without its shift
        shift = shift.clone()
        shift[1488:] = 0.0
    y = F.leaky_relu(F.conv1d(x, w, p["b"][i], dilation=dil), SLOPE)[:, :, :T]
    return y * p["scale"][i][None, :, None] + shift[None, :, None]


def trunk(x, p, fault=None):
    """x (B, 60, P2) -> {"tdnn1" .. "tdnn5": (B, T, C)} frame-major, as the device lays them out"""
    out, x = {}, x.to(p["dtype"])
    for i, name in enumerate(LAYERS):
        x = layer(x, p, i, fault)
        out[name] = x.transpose(1, 2)
    return out


def head(x5, w, mode, p, fault=None):
    """x5 (B, T, 1500); w (B, K, Fw) pooling weights or None (K = 1, unweighted); mode "linear" | "nearest" ->
    {"mean", "std": (B K, 1500), "emb", "embn": (B K, 512)}"""
    dtype = p["dtype"]
    B, T, _ = x5.shape
    K = 1 if w is None else w.shape[1]
    wr = None if w is None else pool_ref.resample(w.reshape(B * K, -1), T, mode, dtype)
    mean, std = pool_ref.pool(x5, wr, K, dtype)
    pooled = torch.cat([mean, std], 1)
    if fault is not None and fault[0] == "split_k":          # the sum over the 16 slices without slice fault[1]
        n = POOL_LD // SPLIT_K
        pp, lw = F.pad(pooled, (0, POOL_LD - 3000)), F.pad(p["lw"], (0, POOL_LD - 3000))
        emb = sum(pp[:, s * n:(s + 1) * n] @ lw[:, s * n:(s + 1) * n].t() for s in range(SPLIT_K) if s != fault[1]) + p["lb"]
    else:
        emb = pooled @ p["lw"].t() + p["lb"]
    return dict(mean=mean, std=std, emb=emb, embn=emb / emb.norm(dim=1, keepdim=True))


def forward(x, w, mode, p, fault=None):
    """every stage of one call: ``trunk`` and ``head``"""
    out = trunk(x, p, fault)
    out.update(head(out["tdnn5"], w, mode, p, fault))
    return out


# the planted faults of the host test: (name, layer or slice) -> the first exposed stage that must leave its gate
FAULTS = {
    ("dilation", 2): "tdnn3",                    # tdnn3 at dilation 2
    ("cross_chunk", 1): "tdnn3",                 # in hidden tdnn2: seen behind it
    ("cross_chunk", 2): "tdnn3",
    ("low_plane", 1): "tdnn3",
    ("low_plane", 2): "tdnn3",
    ("low_plane", 3): "tdnn4",
    ("low_plane", 4): "tdnn5",
    ("shift_tail", 4): "tdnn5",
    ("split_k", 7): "emb",
    ("split_k", 15): "emb",                      # the slice that holds the last 180 std columns and the padding
}


# --------------------------------------------------------------------------- the measure
def row_err(got, ref):
    """worst relative L2 over the rows (last dimension) of got against ref; NaN if anything is NaN"""
    got, ref = got.to(F64), ref.to(F64)
    e = (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)
    return float("nan") if torch.isnan(e).any() else e.max().item()


def sincnet_output(rec, buf0, scale=None, shift=None, part=None, gamma=None, beta=None):
    """dz_emb_peek's buffer 0 (a flat float32 CPU tensor) in the form its record names -> (B, 60, P2) float64: what
    tdnn1 consumes.  Forms 2 / 3 hold the raw stage; its normalisation is applied as the layer applies it on load, from
    the scale / shift the device computed (2) or from the tile partials with the InstanceNorm's gamma / beta (3)."""
    from diart_amd.weights import from_kb
    B, P2, form = rec["batch"], rec["P2"], rec["form"]
    if form == 0:
        pl = from_kb(buf0.view(torch.float16), B * P2, 64).double()
        x = pl[0] + pl[1] / 2048.0
    else:
        x = buf0.double().view(B * P2, 64)
    x = x.view(B, P2, 64)[:, :, :60].transpose(1, 2)
    if form == 2:
        x = front_ref.activate(x, scale.double().view(B, 64)[:, :60], shift.double().view(B, 64)[:, :60])
    elif form == 3:
        sc, sh = front_ref.finalize_norm(part.view(B, rec["nt2"], 64, 2)[:, :, :60], P2, gamma, beta, F64)
        x = front_ref.activate(x, sc, sh)
    return x.contiguous()


def decode_rows(rec, buf, n):
    """buffers 1 / 2 of dz_emb_peek (a flat float32 CPU tensor) -> (B, P2, n) float64, from planes (hi + lo / 2048) or
    f32 rows as the record says"""
    from diart_amd.weights import from_kb
    rows = rec["batch"] * rec["P2"]
    if rec["planes"]:
        pl = from_kb(buf.view(torch.float16), rows, n).double()
        return (pl[0] + pl[1] / 2048.0).view(rec["batch"], rec["P2"], n)
    return buf.double().view(rec["batch"], rec["P2"], n)


# --------------------------------------------------------------------------- the cases
MAX_BATCH = 11
FUSED_MIN_P2, FUSED_MAX_K = 128, 4           # the pooled tdnn5 epilogue: windows of >= 128 frames, <= 4 speakers


def fused_expected(precision, P2, B, K, compute_units=256):
    """does the handle run tdnn5 with the pooling in its epilogue (xvec_api.hip emb_frames, dz_gemm_pre_pool_ok)?  On
    the split-f16 path, with a chunk pitch of at least one 128-row tile, at most four speakers, and enough 128 x 128
    tiles (12 column tiles per row tile) that the GEMM would not run its 64 x 64 latency tiles: 4 tiles >= 2 per
    compute unit, i.e. from 11 row tiles (1281 rows) on the 256 compute units of the MI355X."""
    tiles = -(-B * P2 // 128) * (1536 // 128)
    return precision == "f16x3" and P2 >= FUSED_MIN_P2 and (K or 1) <= FUSED_MAX_K and 4 * tiles >= 2 * compute_units


# (P2, B): the smallest shape at which a path changes.  16: the shortest window with two pooled frames; 127 / 128 with
# 11 chunks: the fusion switch (11 row tiles: the fewest that fuse); 293 (5 s): B = 1 is two full 128-row tiles plus 37
# rows, 3 (unfused: 7 row tiles), 7 (fused), the handle's capacity; 589 (10 s), 2 chunks: 10 row tiles, unfused
GEOMETRIES = [(16, 3), (127, MAX_BATCH), (128, MAX_BATCH), (293, 1), (293, 3), (293, 7), (293, MAX_BATCH), (589, 2)]
FUSED_GEOMETRIES = [(128, MAX_BATCH), (293, 7), (293, MAX_BATCH)]             # ... in f16x3 with up to 4 speakers
SPEAKER_GEOMETRY = (293, 7)
# (K or None for the unweighted call, resampling mode) at SPEAKER_GEOMETRY; every other geometry runs (3, "linear")
SPEAKER_CASES = [(1, "linear"), (3, "linear"), (4, "linear"), (5, "linear"), (None, "linear"), (3, "nearest")]


def case_list():
    """every (P2, B, K, mode) the GPU test gates"""
    out = [(P2, B, 3, "linear") for P2, B in GEOMETRIES if (P2, B) != SPEAKER_GEOMETRY]
    return out + [SPEAKER_GEOMETRY + km for km in SPEAKER_CASES]


def case_id(c):
    P2, B, K, mode = c
    return f"P{P2}-B{B}-K{'none' if K is None else K}-{mode}"


def audio(P2, B, seed0=700):
    """(B, S) float32 windows of synthetic speech, S = samples_for(P2) (80000 / 160000 at 293 / 589 frames)"""
    from diart_amd.synth import synth_streams
    S = {293: 80000, 589: 160000}.get(P2) or samples_for(P2)
    assert seg_frames(S) == P2
    return torch.from_numpy(synth_streams(B, S / 16000.0 + 0.01, seed0=seed0 + P2))[:, :S].contiguous()


def pool_weights(P2, B, K, seed=0):
    """(B, K, Fw = P2) weights like the overlapped-speech penalty's: dense in [0, 1]; from 100 frames on one speaker is
    silent over the first third of the first chunk and one nearly so over the second half of the last (on the two
    pooled frames of the shortest window either would leave one frame: no std, or one that float32 cannot resolve)"""
    g = torch.Generator().manual_seed(1000 * P2 + 10 * B + K + 7919 * seed)
    w = torch.rand(B, K, P2, generator=g) ** 2 + 1e-8
    if P2 >= 100:
        w[0, 0, :P2 // 3] = 0.0
        w[-1, -1, P2 // 2:] *= 1e-3
    return w


class Case:
    """the float64 restatement of one call on input x (B, 60, P2) and the float32 restatement's distance from it"""

    def __init__(self, x, w, mode, trunk64=None, trunk32=None):
        self.x, self.w, self.mode = x, w, mode
        p64, p32 = params(dtype=F64), params(dtype=F32)
        self.trunk64 = trunk(x, p64) if trunk64 is None else trunk64
        self.trunk32 = trunk(x.to(F32), p32) if trunk32 is None else trunk32
        self.ref = dict(self.trunk64, **head(self.trunk64["tdnn5"], w, mode, p64))
        self.f32 = dict(self.trunk32, **head(self.trunk32["tdnn5"], None if w is None else w.to(F32), mode, p32))
        self.e32 = {k: row_err(self.f32[k], self.ref[k]) for k in STAGES}

    def with_head(self, w, mode):
        """the same trunk under other pooling weights"""
        return Case(self.x, w, mode, self.trunk64, self.trunk32)

    def gate(self, stage):
        return gate(self.e32[stage])

    def err(self, stage, got):
        return row_err(got, self.ref[stage])
