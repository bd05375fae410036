"""Weighted statistics pooling on the device against the float64 restatement of tests/pool_ref.py, on both paths the
embedding handle takes (``dz_k_tdnn_pool``): the pooled epilogue of tdnn5 + ``pool_combine_kernel`` (fused), and the
plain layer + ``stats_pool_reg_kernel`` at the handle's chunk stride, pitch > frames (stand-alone).

Features exact by construction (pool_ref.features): one-hot rows times a power of two against non-negative weights that
are exact on the 22-bit planes, bias 0, e0 = +-1, e1 = 0 — the layer's float32 output is known bit for bit, asserted
on the stand-alone run's Y, and both paths pool the same numbers.  One random-operand case sends the real k-loop
through the epilogue (pool_ref.random_case).

Measure and gate: pool_ref's err_mean / err_std, per element, <= max(1e-6, 4 e32) with e32 the float32 restatement's
error on the same case; the two paths against each other <= 2 gates.  Excluded, by a condition on the weights only: the
std of a row with fewer than two non-zero weights (device: NaN or 0) and both halves of a row with no weight (device:
NaN) — exactly the rows the "degenerate" family is built to hold (asserted on the CPU, test_pool_ref_host.py).

Every output is pre-filled with NaN: guard rows behind the last row and columns 2 C .. ldo - 1 stay NaN, part / s0 (NaN
as well: piece slots behind a chunk's last tile are never written and never read) keep their guard, Y keeps its padding
columns and guard rows.

Measured on the MI355X, 2103 cell lines (``pytest -s`` prints ``POOL|path|geometry|family|err_mean|err_std|gate``):
                                     stand-alone  err_mean  err_std     fused  err_mean  err_std    between  mean     std
    nearest / identity / unweighted               2.5e-6    7.9e-7             8.1e-7    5.9e-7             2.7e-6   7.8e-7
    linear (Fw 293 -> 279)                        1.5e-5    2.0e-5             1.6e-5    1.6e-5             4.6e-7   2.9e-7
    random operands (Cin 512)                     9.0e-8    1.1e-7             9.2e-8    1.1e-7             1.3e-8   9.4e-9
The linear rows are the float32 source position of the resampling (e32 up to 2.0e-5 there, on the "peaky" weights: the
gate follows it; the two paths, which share it, agree to 5e-7).  Closest to its gate: stand-alone 0.67 (P589-T575,
dominant frame, K = 3: err_mean 2.5e-6 of 3.7e-6), fused 0.38, the two paths against each other 0.38 of 2 gates.
Before pool_combine_kernel wrote NaN for the mean of a row without weight it wrote 0 there (21 of 21 cases failed on
the "degenerate" family, fused path only); nothing else disagreed.
"""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

from diart_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pool_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3                                   # rows behind the last one in out and Y; floats behind part and s0: GUARD * 64
LDO = 2 * R.CHANNELS + 8                    # 8 columns behind mean | std
NAN = float("nan")


def _ctx(dev):
    return _lib.context(dev.index or 0)


def _kb(x):
    from diart_amd.weights import kb_major, split_f16
    return kb_major(split_f16(x))


class Layer:
    """the layer's operands on the device and its descriptor; Y (NaN-filled, guarded) for the stand-alone path"""

    def __init__(self, gpu, geom, X, W, bias, e0, e1):
        P, T, nx = geom
        self.gpu, self.geom, self.rows = gpu, geom, nx * P
        self.keep = [_kb(X).to(gpu), _kb(W).to(gpu), bias.to(gpu), e0.to(gpu), e1.to(gpu)]
        self.Y = torch.full((self.rows + GUARD, R.NPAD), NAN, device=gpu)

    def desc(self, with_y):
        dX, dW, db, de0, de1 = self.keep
        d = _lib.ConvGemmDesc()
        d.Xsplit, d.xplane, d.Wsplit = dX.data_ptr(), self.rows * R.CIN, dW.data_ptr()
        d.bias, d.e0, d.e1 = db.data_ptr(), de0.data_ptr(), de1.data_ptr()
        if with_y:
            d.Y = self.Y.data_ptr()
        d.B, d.Tin, d.Tout, d.Tstore, d.Cin, d.taps, d.dil = 1, self.rows, self.rows, self.rows, R.CIN, 1, 1
        d.K, d.Kpad, d.Npad, d.Nstore, d.ldx, d.ldy, d.epi = R.CIN, R.CIN, R.NPAD, R.CHANNELS, R.CIN, R.NPAD, _lib.EPI_TDNN
        return d

    def pool(self, w, Fw, K, fused, pitch=None, frames=None, rows=None):
        """one call of dz_k_tdnn_pool into fresh NaN-filled buffers -> (rc, out on the CPU, part, s0 on the CPU or None)"""
        P, T, nx = self.geom
        pitch, frames = pitch or P, frames or T
        d = self.desc(not fused)
        if rows is not None:
            d.Tin = d.Tout = d.Tstore = rows
        out = torch.full((nx * K + GUARD, LDO), NAN, device=self.gpu)
        part = s0 = None
        if fused:
            npc = _lib.load().dz_k_pool_pieces(pitch)
            part = torch.full((nx * npc * K * R.NPAD * 2 + GUARD * 64,), NAN, device=self.gpu)
            s0 = torch.full((nx * npc * K * 2 + GUARD * 64,), NAN, device=self.gpu)
        dw = None if w is None else w.to(self.gpu)
        rc = _lib.load().dz_k_tdnn_pool(_ctx(self.gpu), C.byref(d), None if dw is None else dw.data_ptr(), Fw, K, pitch, frames,
                                        R.CHANNELS, int(fused), None if part is None else part.data_ptr(),
                                        None if s0 is None else s0.data_ptr(), out.data_ptr(), LDO, None)
        torch.cuda.synchronize()
        return rc, out.cpu(), None if part is None else part.cpu(), None if s0 is None else s0.cpu()


def _run(layer, w, Fw, K, fused):
    """a run that must succeed -> (mean, std) on the CPU, guards and padding checked"""
    P, T, nx = layer.geom
    rc, out, part, s0 = layer.pool(w, Fw, K, fused)
    _lib.check(rc, "dz_k_tdnn_pool")
    _lib.range_check(layer.gpu.index or 0)
    assert torch.isnan(out[nx * K:]).all(), "wrote behind the last row of out"
    assert torch.isnan(out[:, 2 * R.CHANNELS:]).all(), "wrote behind column 2 C of out"
    if fused:
        assert torch.isnan(part[-GUARD * 64:]).all() and torch.isnan(s0[-GUARD * 64:]).all(), "wrote behind part / s0"
    return out[:nx * K, :R.CHANNELS], out[:nx * K, R.CHANNELS:2 * R.CHANNELS]


def _check_y(layer, want):
    """the stand-alone run's Y: the layer's output bit for bit, padding columns and guard rows untouched"""
    Y = layer.Y.cpu()
    assert torch.isnan(Y[layer.rows:]).all(), "wrote behind the last row of Y"
    assert torch.isnan(Y[:, R.CHANNELS:]).all(), "wrote behind column Nstore of Y"
    if want is not None:
        assert torch.equal(Y[:layer.rows, :R.CHANNELS], want.reshape(layer.rows, R.NPAD)[:, :R.CHANNELS])
    layer.Y.fill_(NAN)


def _gate_cell(tag, ref, e32, got, fused_got=None):
    """print the cell's line(s), then assert: the gate, the degenerate rows' condition, the two paths against each other"""
    g = R.gate(e32)
    results = [("standalone", got)] + ([("fused", fused_got)] if fused_got is not None else [])
    lines = []
    for path, (mean, std) in results:
        em, es = ref.errors(mean, std)
        lines.append((path, em, es))
        print(f"POOL|{path}|{tag}|{em:.3e}|{es:.3e}|{g:.3e}")
    if fused_got is not None:
        bm, bs = ref.between(got, fused_got)
        print(f"POOL|between|{tag}|{bm:.3e}|{bs:.3e}|{2 * g:.3e}")
    for path, (mean, std) in results:
        empty, single = ~ref.mean_ok, ref.mean_ok & ~ref.std_ok
        assert torch.isnan(mean[empty]).all() and torch.isnan(std[empty]).all(), f"{path} {tag}: a row without weight is not NaN"
        assert (torch.isnan(std[single]) | (std[single] == 0)).all(), f"{path} {tag}: std of a single-frame row"
        assert not torch.isnan(mean[ref.mean_ok]).any() and not torch.isnan(std[ref.std_ok]).any(), f"{path} {tag}: NaN"
    for path, em, es in lines:
        assert em <= g and es <= g, (path, tag, em, es, g)
    if fused_got is not None:
        assert bm <= 2 * g and bs <= 2 * g, (tag, bm, bs, g)
    return lines


CASES = [pytest.param(geom, feat, id=f"{R.geom_id(geom)}-{feat}") for geom in R.GEOMETRIES for feat in R.FEATURES]


@pytest.mark.parametrize("geom,feat", CASES)
def test_pooling_against_float64(gpu, geom, feat):
    P, T, nx = geom
    f = R.features(geom, feat)
    from diart_amd.weights import split_f16
    for name in ("X", "W"):                  # the operands are exact on the planes the kernel reads
        p = split_f16(f[name]).view(torch.float16).double()
        assert torch.equal(p[0] + p[1] / 2048.0, f[name].double())
    zeros = torch.zeros(R.NPAD)
    layer = Layer(gpu, geom, f["X"], f["W"], zeros, f["e0"], zeros)
    want_y = f["y"]
    worst = {}
    for K, mode, Fw, fam in R.cells(geom):
        w, ref, e32 = R.cell_ref(geom, feat, K, mode, Fw, fam)
        assert e32 <= R.E32_CAP
        arg_fw = 0 if w is None else (-Fw if mode == "nearest" else Fw)
        got = _run(layer, w, arg_fw, K, fused=False)
        _check_y(layer, want_y)
        want_y = None                        # (bit for bit once per case; guards and padding after every run)
        fused_got = _run(layer, w, arg_fw, K, fused=True) if K <= R.FUSED_MAX_K else None
        tag = f"{R.geom_id(geom)}-{feat}-K{K}-{mode}{Fw}|{fam}"
        for path, em, es in _gate_cell(tag, ref, e32, got, fused_got):
            a = worst.setdefault(path, [0.0, 0.0])
            a[0], a[1] = max(a[0], em), max(a[1], es)
    for path, (em, es) in worst.items():
        print(f"POOL_WORST|{path}|{R.geom_id(geom)}-{feat}|{em:.3e}|{es:.3e}")


def test_random_operands_through_the_real_k_loop(gpu):
    c = R.random_case()
    layer = Layer(gpu, R.RANDOM_GEOM, c["X"], c["W"], c["bias"], c["e0"], c["e1"])
    got = _run(layer, c["w"], R.RANDOM_FW, R.RANDOM_K, fused=False)
    _check_y(layer, None)
    fused_got = _run(layer, c["w"], R.RANDOM_FW, R.RANDOM_K, fused=True)
    _gate_cell(f"{R.geom_id(R.RANDOM_GEOM)}-gemm-K{R.RANDOM_K}-{R.RANDOM_MODE}{R.RANDOM_FW}|dense", c["ref"], c["e32"], got, fused_got)


def test_two_launches_give_the_same_bits(gpu):
    """fixed summation order on both paths: the same case twice, the same bits"""
    geom = (129, 129, 9)
    f = R.features(geom, "randn")
    zeros = torch.zeros(R.NPAD)
    layer = Layer(gpu, geom, f["X"], f["W"], zeros, f["e0"], zeros)
    w = R.weights("peaky", geom, 3, "identity", 129)
    for fused in (False, True):
        a, b = _run(layer, w, 129, 3, fused), _run(layer, w, 129, 3, fused)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), fused


def test_refused_arguments_come_back_as_errors(gpu):
    """what the launchers refuse is an error code with a message and no launch: out stays NaN"""
    geom = (129, 129, 9)
    f = R.features(geom, "randn")
    zeros = torch.zeros(R.NPAD)
    layer = Layer(gpu, geom, f["X"], f["W"], zeros, f["e0"], zeros)
    w5, w3 = R.weights("dense", geom, 5, "identity", 129), R.weights("dense", geom, 3, "identity", 129)
    refused = [
        ("five speakers, fused", dict(w=w5, Fw=129, K=5, fused=True)),
        ("pitch below a tile, fused", dict(w=None, Fw=0, K=3, fused=True, pitch=127, frames=100, rows=127 * 9)),
        ("one frame, fused", dict(w=None, Fw=0, K=3, fused=True, frames=1)),
        ("one frame, stand-alone", dict(w=None, Fw=0, K=3, fused=False, frames=1)),
        ("rows no multiple of the pitch, fused", dict(w=w3, Fw=129, K=3, fused=True, rows=129 * 9 - 1)),
        ("rows no multiple of the pitch, stand-alone", dict(w=w3, Fw=129, K=3, fused=False, rows=129 * 9 - 1)),
        ("one weight frame", dict(w=w3, Fw=1, K=3, fused=True)),
    ]
    for what, kw in refused:
        rc, out, part, s0 = layer.pool(**kw)
        assert rc != 0, what
        assert _lib.load().dz_last_error().decode(), what
        with pytest.raises(_lib.DiartAmdError):
            _lib.check(rc, "dz_k_tdnn_pool")
        assert torch.isnan(out).all(), what
        assert part is None or (torch.isnan(part).all() and torch.isnan(s0).all()), what
        assert torch.isnan(layer.Y).all(), what
    assert _lib.load().dz_k_pool_pieces(128) == 2 and _lib.load().dz_k_pool_pieces(129) == 2
    assert _lib.load().dz_k_pool_pieces(293) == 4 and _lib.load().dz_k_pool_pieces(589) == 6
