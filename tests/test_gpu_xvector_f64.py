"""The pyannote x-vector trunk and tail on the device, stage by stage, against the float64 restatement of
tests/xvector_ref.py, as the handle launches them (``HipEmbedding`` / ``dz_emb_*``), in both precisions.

What is held.  Through ``dz_emb_peek``: tdnn3's and tdnn4's outputs (the handle's two ping-pong buffers as a forward
leaves them), tdnn5's where it ran on its own (windows under 128 frames, exact f32, more than 4 speakers, or with the
option ``pool_fuse`` = 0, which every fused case is run with a second time), the pooled mean and std; from the call: the
embedding, plain and normalised.  tdnn1's and tdnn2's outputs are overwritten by the ping-pong before a forward returns
and are NOT exposed (no buffer is added to the handle for a test's sake): they are held through tdnn3, and
tests/test_xvector_ref_host.py shows that a fault planted in either leaves tdnn3's gate.  The reference's input is the
device's own SincNet output (peek buffer 0 in the form its record names, converted to float64).

Every comparison runs over ALL valid frames t < T of every chunk; rows t >= T of a chunk are documented garbage that no
valid row reads, and are never read here either.  Measure and gate: xvector_ref's relative L2 per row, worst row, <=
max(1e-6, 4 e32) with e32 the float32 restatement's error on the same input — one rule for both precisions.

Equalities, bit for bit: a small call after a full-capacity call on the same handle against the same call on a fresh
handle; a chunk's valid rows through tdnn4 whatever its neighbours hold, and alone against inside a batch (a row's
k-loop in k_gemm_pre.hip / k_gemm_f32.hip runs over the 32-wide k-tiles in the same order in every tile shape and at
every tile position); a rolling-window view against its contiguous copy; ``dz_emb_frames`` + ``dz_emb_pool`` against
``dz_emb_forward_multi``, pooled again with other weights, refused with another chunk count, and past the 4-speaker
limit of the fused epilogue.  (``__call__`` with repeated rows, ``forward_multi`` and ``repeated_rows="share"`` agree as
tests/test_gpu_models.py states.)

Which cases fuse: the handle runs tdnn5 with the pooling in its epilogue on the split-f16 path from 128 frames per chunk
AND from 11 row tiles of 128 (1281 rows) on, below which the GEMM runs its 64 x 64 latency tiles
(xvector_ref.fused_expected).  So 127 / 128 frames run with 11 chunks, 293 with 7 and 11 fuses, 293 with 1 and 3 and
589 with 2 chunks do not, and the speaker counts run at 293 x 7.

``pytest -s`` prints ``XVEC|precision|case|stage|error|gate`` for every stage of every case.  Measured on the MI355X,
235 lines, the worst row of the worst case per stage (gates 1.0e-6 .. 5.3e-6):
             tdnn3    tdnn4    tdnn5    mean     std      emb      normalised
    f16x3    4.7e-7   5.1e-7   5.5e-7   6.8e-7   1.3e-6   8.7e-7   8.7e-7
    f32      1.3e-6   1.3e-6   1.3e-6   8.1e-7   2.7e-6   1.3e-6   1.2e-6
Closest to its gate: f16x3 0.35 (293 x 11, tdnn3: 4.7e-7 of 1.33e-6); f32 0.95 (293 x 7, tdnn3: 1.30e-6 of 1.37e-6).
The exact-f32 layers are 3 - 4 times the float32 restatement's error throughout (f16x3: 1 - 1.5 times): k_gemm_f32.hip
adds each product into ONE running f32 accumulator over the 1536-deep contraction, where the CPU's float32 GEMM sums
in blocks; the split-f16 kernel accumulates the same way but its products are exact and its operands carry 22 bits.
Every equality held bit for bit on the first run, alone against inside a batch included; nothing here found a defect.
"""
import sys
from pathlib import Path

import pytest
import torch

from diart_amd import _lib
from diart_amd.models import HipEmbedding

sys.path.insert(0, str(Path(__file__).resolve().parent))
import xvector_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16x3", "f32")


# --------------------------------------------------------------------------- running and reading a call
@pytest.fixture(scope="module")
def models(gpu):
    """(precision, weight_interp) -> the model under test, made on first use"""
    made = {}

    def get(precision, interp="linear"):
        if (precision, interp) not in made:
            made[(precision, interp)] = fresh(gpu, precision, interp)
        return made[(precision, interp)]
    return get


def fresh(gpu, precision, interp="linear"):
    return HipEmbedding(R._synth_state(), max_batch=R.MAX_BATCH, precision=precision, weight_interp=interp).to(gpu)


def snapshot(model, S, out):
    """everything the handle for S samples exposes after a call, on the CPU; valid frames only"""
    rec = model.peek_record(S)
    B, P2 = rec["batch"], rec["P2"]
    T = [rec[f"T{i}"] for i in range(1, 6)]
    peek = lambda which: model.peek(S, which)[0].cpu()
    snap = dict(rec=rec, T=T, out=out.cpu().reshape(-1, 512), buf0=peek(0))
    if rec["form"] == 2:
        snap["scale"], snap["shift"] = peek(5), peek(6)
    if rec["form"] == 3:
        snap["part"] = peek(7)
    snap["tdnn3"] = R.decode_rows(rec, peek(1), 512)[:, :T[2]]
    snap["tdnn4"] = R.decode_rows(rec, peek(2), 512)[:, :T[3]]
    assert model.peek(S, 1)[1] == T[2] and model.peek(S, 2)[1] == T[3]
    ptr, cnt, fr = model._peek_raw(model._handles[S][0], 3)
    assert fr == T[4]
    if rec["x5_valid"]:
        assert rec["pending"] == 0 and cnt == B * P2 * 1536
        snap["tdnn5"] = peek(3).double().view(B, P2, 1536)[:, :T[4], :1500]
    else:                                              # pending at tdnn4's output: the peek says so, no stale rows
        assert rec["pending"] == B and ptr.value is None and cnt == 0
    pooled = peek(4).view(rec["pooled_rows"], rec["pooled_ld"])
    snap["mean"], snap["std"] = pooled[:, :1500], pooled[:, 1500:3000]
    return snap


def run(model, x, w, normalize=False):
    """x (B, S) on the CPU (or a (B, S) device view), w (B, K, Fw) or None: one call -> its snapshot"""
    xd = x[:, None].to(model.device)
    out = model(xd, None) if w is None else model.forward_multi(xd, w.to(model.device), normalize=normalize)
    torch.cuda.synchronize()
    _lib.range_check(model.device.index or 0)
    return snapshot(model, x.shape[1], out)


def device_input(model, snap):
    sd = R._synth_state()
    return R.sincnet_output(snap["rec"], snap["buf0"], snap.get("scale"), snap.get("shift"), snap.get("part"),
                            sd["sincnet.norm1d.2.weight"], sd["sincnet.norm1d.2.bias"])


BITS = ["tdnn3", "tdnn4", "tdnn5", "mean", "std", "out"]


def same_bits(a, b, stages=BITS, chunks=None):
    """the stages both snapshots hold, equal bit for bit (of ``chunks`` only: the per-chunk stages)"""
    for s in stages:
        if (s in a) != (s in b):
            return f"{s} in one only"
        if s in a:
            u, v = (a[s], b[s]) if chunks is None else (a[s][chunks], b[s][chunks])
            if not torch.equal(u, v):
                return s
    return None


# --------------------------------------------------------------------------- stages against float64
_trunks = {}


def reference(key, x_in, w, mode):
    """the Case of this input; the trunk (float64 and float32) once per (precision, geometry), shared by every head"""
    base = _trunks.get(key)
    if base is None or not torch.equal(base.x, x_in):
        base = _trunks[key] = R.Case(x_in, w, mode)
        return base
    return base.with_head(w, mode)


def gate_stages(tag, case, snap, stages):
    lines = []
    for s in stages:
        got = snap["out"] if s in ("emb", "embn") else snap[s]
        lines.append((s, case.err(s, got), case.gate(s)))
        print(f"XVEC|{tag}|{s}|{lines[-1][1]:.3e}|{lines[-1][2]:.3e}")
    for s, err, g in lines:
        assert g <= R.EMB_LIMIT and err <= g, (tag, s, err, g)


def check_case(model, precision, c, tag_suffix=""):
    P2, B, K, mode = c
    x = R.audio(P2, B)
    w = None if K is None else R.pool_weights(P2, B, K)
    snap = run(model, x, w)
    rec = snap["rec"]
    assert rec["P2"] == P2 == _lib.load().dz_seg_frames_for(x.shape[1]) and snap["T"] == R.valid_frames(P2)
    assert rec["batch"] == B and rec["pooled_rows"] == B * (K or 1)
    assert rec["form"] == (0 if precision == "f16x3" else (1 if _lib.get_option("f32_gemm") else 2))
    assert rec["planes"] == int(precision == "f16x3")
    cus = torch.cuda.get_device_properties(model.device).multi_processor_count
    fused = R.fused_expected(precision, P2, B, K, cus) and _lib.get_option("pool_fuse") != 0
    assert rec["x5_valid"] == int(not fused), rec
    case = reference((precision, P2, B), device_input(model, snap), w, mode)
    tag = f"{precision}|{R.case_id(c)}{tag_suffix}"
    gate_stages(tag, case, snap, ["tdnn3", "tdnn4"] + (["tdnn5"] if not fused else []) + ["mean", "std", "emb"])
    if w is not None:
        normed = run(model, x, w, normalize=True)
        assert same_bits(snap, normed, BITS[:-1]) is None
        gate_stages(tag, case, normed, ["embn"])
    return fused, snap


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.case_list(), ids=R.case_id)
def test_stages_against_float64(gpu, models, precision, c):
    model = models(precision, c[3])
    assert model.weight_interp == c[3]
    fused, snap = check_case(model, precision, c)
    if fused:                                          # the same case with tdnn5 on its own: its output is exposed
        _lib.set_option("pool_fuse", 0)
        try:
            again, unfused = check_case(model, precision, c, "|pool_fuse=0")
        finally:
            _lib.set_option("pool_fuse", 1)
        assert not again and same_bits(snap, unfused, ["tdnn3", "tdnn4"]) is None
    if c[2] == 5:                                      # past the fused limit the pending state is gone ...
        assert snap["rec"]["pending"] == 0 and snap["rec"]["x5_valid"] == 1
        P2, B, _, mode = c
        nxt = run(model, R.audio(P2, B), R.pool_weights(P2, B, 3))
        assert nxt["rec"]["pending"] == (B if precision == "f16x3" else 0)      # ... and the next call ran its own frames
        assert (P2, B) in R.FUSED_GEOMETRIES


@pytest.mark.parametrize("P2,B", [(16, 3), (293, 3)])
def test_tdnn1_normalising_on_load(gpu, models, P2, B):
    """exact f32 without the f32 matrix-core GEMM: tdnn1 runs per chunk on the raw SincNet stage and applies its
    InstanceNorm on load (the record's form 2); the reference gets that stage through front_ref.activate"""
    _lib.set_option("f32_gemm", 0)
    try:
        _, snap = check_case(models("f32"), "f32", (P2, B, 3, "linear"), "|f32_gemm=0")
    finally:
        _lib.set_option("f32_gemm", 1)
    assert snap["rec"]["form"] == 2


# --------------------------------------------------------------------------- equalities
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("P2,B", [(293, 1), (293, 3), (293, 7), (16, 3)])
def test_small_call_after_a_full_one_on_the_same_handle(gpu, models, precision, P2, B):
    """no valid row reads what an earlier, larger call left behind its own rows"""
    used, new = models(precision), fresh(gpu, precision)
    run(used, R.audio(P2, R.MAX_BATCH, seed0=900), R.pool_weights(P2, R.MAX_BATCH, 4, seed=1))
    x, w = R.audio(P2, B), R.pool_weights(P2, B, 3)
    a, b = run(used, x, w), run(new, x, w)
    assert torch.equal(a["buf0"], b["buf0"]) and same_bits(a, b) is None, same_bits(a, b)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("P2", [16, 127, 293])
def test_a_chunk_does_not_see_its_neighbours(gpu, models, precision, P2):
    model, B = models(precision), 3
    x, w = R.audio(P2, B), R.pool_weights(P2, B, 3)
    base = run(model, x, w)
    other = x.clone()
    other[1] = R.audio(P2, 1, seed0=950)[0]
    swapped = run(model, other, w)
    assert same_bits(base, swapped, ["tdnn3", "tdnn4"], chunks=[0, 2]) is None
    assert not torch.equal(base["tdnn3"][1], swapped["tdnn3"][1])
    for c in range(B):                                 # alone: other tiles, other positions in them, the same bits
        alone = run(model, x[c:c + 1].contiguous(), w[c:c + 1])
        for s in ("tdnn3", "tdnn4"):
            assert torch.equal(alone[s][0], base[s][c]), (s, c)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rolling_window_view_equals_its_copy(gpu, models, precision):
    model, B, S, hop = models(precision), 3, 80000, 8000
    from diart_amd.synth import synth_streams
    long = torch.from_numpy(synth_streams(1, (S + hop * B) / 16000.0, seed0=970))[0].to(gpu)
    view = long.unfold(0, S, hop)[:B]
    assert view.stride() == (hop, 1) and not view.is_contiguous()
    w = R.pool_weights(293, B, 3)
    a, b = run(model, view, w), run(model, view.contiguous(), w)
    assert torch.equal(a["buf0"], b["buf0"]) and same_bits(a, b) is None, same_bits(a, b)


# --------------------------------------------------------------------------- dz_emb_frames / dz_emb_pool, directly
class Split:
    """the two halves on the model's own handle for x (B, S)"""

    def __init__(self, model, x):
        self.model, self.lib, self.S, self.B = model, _lib.load(), x.shape[1], x.shape[0]
        self.x = x.to(model.device).contiguous()
        self.handle = model._need(self.S, self.B)
        self.stream = torch.cuda.current_stream(model.device).cuda_stream

    def frames(self):
        _lib.check(self.lib.dz_emb_frames(self.handle, self.x.data_ptr(), self.x.stride(0), self.B, self.stream), "dz_emb_frames")

    def pool_rc(self, w, batch=None):
        wd = w.to(self.model.device).contiguous()
        out = torch.full((wd.shape[0], wd.shape[1], 512), float("nan"), device=self.model.device)
        rc = self.lib.dz_emb_pool(self.handle, wd.data_ptr(), self.B if batch is None else batch, wd.shape[1], wd.shape[2], 0,
                                  out.data_ptr(), self.stream)
        torch.cuda.synchronize()
        return rc, out

    def pool(self, w):
        rc, out = self.pool_rc(w)
        _lib.check(rc, "dz_emb_pool")
        return snapshot(self.model, self.S, out)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("P2,B", [(16, 3), (293, 7)])
def test_frames_then_pool_is_forward_multi(gpu, models, precision, P2, B):
    model = models(precision)
    x = R.audio(P2, B)
    w3, w3b, w5 = R.pool_weights(P2, B, 3), R.pool_weights(P2, B, 3, seed=2), R.pool_weights(P2, B, 5)
    whole = {k: run(model, x, w) for k, w in (("w3", w3), ("w3b", w3b), ("w5", w5))}
    fused = whole["w3"]["rec"]["pending"] == B
    assert fused == (precision == "f16x3" and (P2, B) in R.FUSED_GEOMETRIES)
    sp = Split(model, x)
    sp.frames()
    rec = model.peek_record(sp.S)
    assert rec["pending"] == (B if fused else 0) and rec["pooled_rows"] == 0
    assert same_bits(sp.pool(w3), whole["w3"]) is None
    # the same frames under other weights: what a whole forward with those weights gives
    assert same_bits(sp.pool(w3b), whole["w3b"]) is None
    if fused:
        # another chunk count than the pending one: refused, nothing launched, the next correct call intact
        rc, out = sp.pool_rc(w3[:2], batch=2)
        assert rc != 0 and "pending" in _lib.load().dz_last_error().decode() and torch.isnan(out).all()
        with pytest.raises(_lib.DiartAmdError):
            _lib.check(rc, "dz_emb_pool")
        assert model.peek_record(sp.S)["pending"] == B
        assert same_bits(sp.pool(w3), whole["w3"]) is None
    # five speakers: plain tdnn5 + the stand-alone pooling; nothing is pending behind it
    five = sp.pool(w5)
    assert five["rec"]["pending"] == 0 and five["rec"]["x5_valid"] == 1 and same_bits(five, whole["w5"]) is None
    # three again: the fused result needs new frames, and a new dz_emb_frames gives it
    sp.frames()
    assert model.peek_record(sp.S)["pending"] == (B if fused else 0)
    assert same_bits(sp.pool(w3), whole["w3"]) is None
