"""``repeated_rows="share"`` on the GPU: the verdict of ``dz_rows_repeat`` against a few lines of numpy on built
batches, and the reference-shaped ``(batch spk)`` call of ``HipEmbedding`` / ``HipWeSpeakerEmbedding`` against
``forward_multi`` on the un-repeated windows (bit for bit), against ``"each"`` and against the oracle.

Gates are the ones the suite already has: ``torch.equal`` where ``forward_multi`` and the rows call are known to agree
bit for bit (WeSpeaker: tests/test_gpu_wespeaker.py::test_forward_multi_equals_repeated_rows), max |d| < 1e-5 for
``pyannote/embedding``'s two forms and cosine >= 0.99999 / relative L2 < 1e-4 against the oracle
(tests/test_gpu_models.py::test_embedding_forward_both_forms)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from diart_amd import _lib
from diart_amd import models as M
from diart_amd.synth import synth_embedding_state, synth_streams, synth_wespeaker_state

pytestmark = pytest.mark.gpu

EMB_COS = 0.99999                       # tests/test_gpu_models.py
S5 = 80000
PRECISIONS = ["f32", "f16x3"]
ARCHS = {"xvector": (M.HipEmbedding, synth_embedding_state), "wespeaker": (M.HipWeSpeakerEmbedding, synth_wespeaker_state)}


# --------------------------------------------------------------------------- #
# the detector
# --------------------------------------------------------------------------- #
def repeat_of(t: torch.Tensor) -> int:
    """``dz_rows_repeat`` of a (n, S) float32 device tensor, addressed in place."""
    assert t.ndim == 2 and t.dtype == torch.float32 and t.is_cuda and (t.shape[1] == 1 or t.stride(1) == 1)
    r = C.c_int(-1)
    _lib.check(_lib.load().dz_rows_repeat(_lib.context(t.device.index), t.data_ptr(), t.stride(0), t.shape[0], t.shape[1],
                                          torch.cuda.current_stream(t.device).cuda_stream, C.byref(r)), "dz_rows_repeat")
    return r.value


def want_repeat(x: np.ndarray) -> int:
    """The definition: gcd of n and the lengths of the runs of bitwise-equal rows (run boundaries sit at 0, n and every
    row that differs from its predecessor)."""
    bits = np.ascontiguousarray(x).view(np.uint32)
    g = len(bits)
    for i in range(1, len(bits)):
        if not np.array_equal(bits[i], bits[i - 1]):
            g = math.gcd(g, i)
    return g


def runs(lengths, S, seed=0):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.repeat(rng.standard_normal((1, S), dtype=np.float32), n, axis=0) for n in lengths])


def flip(x, row, col):
    x = x.copy()
    x.view(np.uint32)[row, col] ^= 1
    return x


def detector_cases(S):
    zeros = np.zeros((6, S), np.float32)
    negzero = zeros.copy()
    negzero[3, S // 2] = -0.0
    nans = runs([3, 3], S, seed=5)
    nans[:, S // 3] = np.float32("nan")
    nans.view(np.uint32)[3:, 0] = 0x7FC00123                     # a NaN payload: equal bits stay equal
    base = runs([3, 3, 3, 3], S, seed=1)
    return [("4 x 3 repeats", base, 3),
            ("6 identical rows", runs([6], S, seed=2), 6),
            ("runs of 6, 3, 3", runs([6, 3, 3], S, seed=3), 3),
            ("runs of 2, 3", runs([2, 3], S, seed=4), 1),
            ("one row", runs([1], S, seed=6), 1),
            ("bit flipped in the first sample", flip(base, 4, 0), 1),
            ("bit flipped in the last sample", flip(base, 7, S - 1), 1),
            ("bit flipped in the last sample of the last row", flip(base, 11, S - 1), 1),
            ("-0.0 against +0.0", negzero, 1),                    # runs of 3, 1, 2
            ("all zeros", zeros, 6),
            ("bit-identical NaN rows", nans, 3),
            ("nothing repeats", runs([1] * 9, S, seed=7), 1),
            ("pairs", runs([2] * 5, S, seed=8), 2)]


def layouts(x: np.ndarray, dev):
    """The batch as a contiguous tensor, as a view whose row stride is not a multiple of 4 samples, and as a view with a
    16-byte aligned stride behind a base that is not (rows 4 bytes off)."""
    n, S = x.shape
    t = torch.from_numpy(x)
    yield "contiguous", t.to(dev)
    stride = S + 3 if (S + 3) % 4 else S + 2
    buf = torch.zeros(n * stride + 8, dtype=torch.float32, device=dev)
    view = buf.as_strided((n, S), (stride, 1))
    view.copy_(t)
    assert view.stride(0) % 4 != 0
    yield "odd stride", view
    stride = (S + 3) // 4 * 4
    buf2 = torch.zeros(n * stride + 8, dtype=torch.float32, device=dev)
    view2 = buf2.as_strided((n, S), (stride, 1), 1)
    view2.copy_(t)
    assert view2.data_ptr() % 16 == 4 and view2.stride(0) % 4 == 0
    yield "unaligned base", view2


@pytest.mark.parametrize("S", [S5, 1683, 7, 2])
def test_rows_repeat_verdicts(gpu, S):
    """Every case in every layout; S = 80000 (whole 16-byte words), 1683 and 7 (a tail of 3 samples), 2 (no whole word).
    After each call a batch of 12 identical rows must answer 12: a flag left behind by the previous case would break it."""
    same12 = torch.full((12, 16), 0.5, device=gpu)
    for name, x, stated in detector_cases(S):
        want = want_repeat(x)
        assert want == stated, (name, want, stated)                  # the numpy definition and the stated verdict agree
        for layout, t in layouts(x, gpu):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32))      # NaN payloads survived the copy
            got = repeat_of(t)
            assert got == want, (S, name, layout, got, want)
            assert repeat_of(same12) == 12, (S, name, layout, "flags were not cleared")
            assert repeat_of(t) == want, (S, name, layout, "second call")


def test_rows_repeat_many_rows_rolling_view_and_streams(gpu):
    """192 rows of 80 000 samples (the reference-shaped call of 64 chunks x 3 speakers); more rows than one workgroup of
    the second kernel has threads; an expanded view (stride 0); the in-place rolling window other tests use (stride
    8000: neighbouring windows overlap and differ); a side stream."""
    x = np.repeat(runs([1] * 64, S5, seed=11), 3, axis=0)
    assert repeat_of(torch.from_numpy(x).to(gpu)) == 3
    assert repeat_of(torch.from_numpy(flip(x, 190, S5 - 1)).to(gpu)) == 1
    many = runs([5] * 200, 33, seed=12)
    assert repeat_of(torch.from_numpy(many).to(gpu)) == 5
    assert repeat_of(torch.from_numpy(flip(many, 998, 32)).to(gpu)) == 1
    assert repeat_of(torch.from_numpy(many[:1]).to(gpu).expand(7, 33)) == 7
    stream = torch.from_numpy(synth_streams(1, 12.0, seed0=3)[0]).to(gpu)
    view = stream.unfold(0, S5, 8000)[:6]
    assert view.stride(0) == 8000 and repeat_of(view) == 1
    hop = stream[1:].unfold(0, S5, 8001)[:6]                         # neither the base nor the stride is aligned
    assert repeat_of(hop) == want_repeat(hop.cpu().numpy()) == 1
    side = torch.cuda.Stream(gpu)
    t = torch.from_numpy(x).to(gpu)
    torch.cuda.synchronize(gpu)
    with torch.cuda.stream(side):
        assert repeat_of(t) == 3
    assert repeat_of(t) == 3


def test_rows_repeat_refuses_bad_arguments(gpu):
    t = torch.zeros(4, 16, device=gpu)
    r = C.c_int()
    fn, ctx = _lib.load().dz_rows_repeat, _lib.context(gpu.index)
    assert fn(ctx, t.data_ptr(), 16, 0, 16, None, C.byref(r)) == 2
    assert fn(ctx, t.data_ptr(), 16, 4, 0, None, C.byref(r)) == 2
    assert fn(ctx, t.data_ptr(), -16, 4, 16, None, C.byref(r)) == 2
    assert fn(ctx, None, 16, 4, 16, None, C.byref(r)) == 2
    assert repeat_of(t) == 4


# --------------------------------------------------------------------------- #
# the models
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def windows():
    return torch.from_numpy(synth_streams(32, 5.01, seed0=500))[:, None, :S5].contiguous()       # (32,1,80000)


@pytest.fixture(scope="module")
def model(gpu):
    made = {}

    def get(arch, precision, mode, max_batch=128):
        key = (arch, precision, mode, max_batch)
        if key not in made:
            cls, synth = ARCHS[arch]
            made[key] = cls(synth(), max_batch=max_batch, precision=precision, repeated_rows=mode).to(gpu)
        return made[key]

    yield get
    made.clear()


def pool_weights(B, K, seed, F=293):
    return torch.rand(B, F, K, generator=torch.Generator().manual_seed(seed)) ** 2 + 1e-8       # (B,F,K) like OSP output


def reference_call(x, w):
    """What the reference's SpeakerEmbedding hands the model: ``repeat(1, K, 1)`` rows, "(batch spk) frame" weights."""
    B, _, K = w.shape
    return x.repeat(1, K, 1).reshape(B * K, 1, -1), w.permute(0, 2, 1).reshape(B * K, -1)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("B", [1, 4, 32])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_share_equals_forward_multi(gpu, windows, model, arch, precision, B, K):
    x, w = windows[:B].to(gpu), pool_weights(B, K, seed=10 * B + K).to(gpu)
    rows, wrows = reference_call(x, w)
    shared = model(arch, precision, "share")
    got = shared(rows, wrows)
    assert shared.last_shared == (B, K)
    assert got.shape == (B * K, shared.dimension)
    want = model(arch, precision, "each").forward_multi(x, w.permute(0, 2, 1).contiguous())
    assert torch.equal(got.view(B, K, -1), want)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_share_against_each(gpu, windows, model, arch, precision):
    B, K = 4, 3
    x, w = windows[:B].to(gpu), pool_weights(B, K, seed=1).to(gpu)
    rows, wrows = reference_call(x, w)
    each, shared = model(arch, precision, "each"), model(arch, precision, "share")
    a, b = each(rows, wrows), shared(rows, wrows)
    assert each.last_shared is None and shared.last_shared == (B, K)
    d = (a - b).abs().max().item()
    print(arch, precision, "share vs each max|d|", d)
    if arch == "wespeaker":
        assert torch.equal(a, b)
    else:
        assert d < 1e-5


@pytest.mark.parametrize("precision", PRECISIONS)
def test_share_against_the_oracle(gpu, windows, model, precision):
    from oracle.models_ref import XVectorSincNetRef
    ref_m = XVectorSincNetRef().eval()
    ref_m.load_state_dict(synth_embedding_state())
    B, K = 4, 3
    x, w = windows[:B], pool_weights(B, K, seed=0)
    with torch.no_grad():
        ref = ref_m.forward_multi(x, w)                             # (B,K,512)
    rows, wrows = reference_call(x.to(gpu), w.to(gpu))
    shared = model("xvector", precision, "share")
    got = shared(rows, wrows).cpu().view(B, K, 512)
    assert shared.last_shared == (B, K)
    cos = torch.nn.functional.cosine_similarity(got.double(), ref.double(), dim=-1)
    rel = ((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    print(precision, "share vs oracle: cos min", cos.min().item(), "rel", rel)
    assert cos.min().item() >= EMB_COS and rel < 1e-4


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_fallback_when_nothing_repeats(gpu, windows, model, arch, precision):
    """Distinct rows, rows whose runs have no common length, no weights, one row: today's path, bit for bit."""
    each, shared = model(arch, precision, "each"), model(arch, precision, "share")
    x = windows[:6].to(gpu)
    w = torch.rand(6, 293, generator=torch.Generator().manual_seed(3)).to(gpu)
    assert torch.equal(shared(x, w), each(x, w)) and shared.last_shared is None
    ragged = x[[0, 0, 1, 1, 1]]                                      # runs of 2, 3
    assert torch.equal(shared(ragged, w[:5]), each(ragged, w[:5])) and shared.last_shared is None
    rows, wrows = reference_call(x[:2], pool_weights(2, 3, seed=4).to(gpu))
    shared(rows, wrows)
    assert shared.last_shared == (2, 3)
    assert torch.equal(shared(rows), each(rows)) and shared.last_shared is None          # weights None
    assert torch.equal(shared(x[:1], w[:1]), each(x[:1], w[:1])) and shared.last_shared is None


@pytest.mark.parametrize("arch", list(ARCHS))
def test_identical_neighbouring_windows_share_more(gpu, windows, model, arch):
    """Two chunks of digital silence x 3 speakers: six identical rows, R = 6 — more than the speaker count, and right,
    because identical waveforms have identical trunks."""
    each, shared = model(arch, "f16x3", "each"), model(arch, "f16x3", "share")
    for x in (torch.zeros(2, 1, S5, device=gpu), windows[:1].repeat(2, 1, 1).to(gpu)):
        w = pool_weights(2, 3, seed=6).to(gpu)
        rows, wrows = reference_call(x, w)
        got = shared(rows, wrows)
        assert shared.last_shared == (1, 6)
        want = each.forward_multi(x, w.permute(0, 2, 1).contiguous()).view(6, -1)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))       # (bits: whatever silence embeds to)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_nan_window(gpu, windows, model, arch, precision):
    B, K = 4, 3
    clean = windows[:B].clone()
    bad = clean.clone()
    bad[1, 0, 40000] = float("nan")
    w = pool_weights(B, K, seed=8).to(gpu)
    shared = model(arch, precision, "share")
    got = shared(*reference_call(bad.to(gpu), w)).view(B, K, -1)
    assert shared.last_shared == (B, K)                              # the K copies of the NaN window are bit-identical
    ref = shared(*reference_call(clean.to(gpu), w)).view(B, K, -1)
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[[0, 2, 3]], ref[[0, 2, 3]]) and torch.isfinite(ref).all()
    _lib.range_check(gpu.index)


class _Hidden:
    """A loaded callable that offers ``__call__`` and ``to`` only: the blocks take their generic (batch spk) branch."""

    def __init__(self, inner):
        self._inner = inner

    def to(self, device):
        self._inner.to(device)
        return self

    def __call__(self, waveform, weights=None):
        return self._inner(waveform, weights)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_through_the_blocks_with_forward_multi_hidden(gpu, windows, arch, precision):
    from diart_amd.blocks import SpeakerEmbedding
    cls, synth = ARCHS[arch]
    inner = cls(synth(), max_batch=16, precision=precision, repeated_rows="share")
    hidden = SpeakerEmbedding(M.EmbeddingModel(lambda: _Hidden(inner)), gpu)
    exposed = SpeakerEmbedding(M.EmbeddingModel(lambda: cls(synth(), max_batch=16, precision=precision)), gpu)
    assert not hasattr(hidden.model.model, "forward_multi") and hasattr(exposed.model.model, "forward_multi")
    B, K = 4, 3
    wave = windows[:B].transpose(1, 2).contiguous()                  # (b, s, 1)
    w = pool_weights(B, K, seed=9)                                   # (b, f, k)
    got, want = hidden(wave, w), exposed(wave, w)
    assert inner.last_shared == (B, K)
    assert got.shape == want.shape == (B, K, inner.dimension)
    d = (got - want).abs().max().item()
    print(arch, precision, "blocks: hidden vs exposed max|d|", d)
    if arch == "wespeaker":
        assert torch.equal(got, want)
    else:
        assert d < 1e-5


@pytest.mark.parametrize("arch", list(ARCHS))
def test_max_batch_32_with_a_96_row_call(gpu, windows, model, arch):
    B, K = 32, 3
    x, w = windows[:B].to(gpu), pool_weights(B, K, seed=12).to(gpu)
    rows, wrows = reference_call(x, w)
    small = model(arch, "f16x3", "share", max_batch=32)
    got = small(rows, wrows)
    assert small.last_shared == (32, 3) and small._handles[S5][1] == 32          # the handle did not have to grow
    assert torch.equal(got.view(B, K, -1), model(arch, "f16x3", "each").forward_multi(x, w.permute(0, 2, 1).contiguous()))


@pytest.mark.parametrize("arch", list(ARCHS))
def test_alternating_shared_and_unshared_calls(gpu, windows, arch):
    """One model through shared, unshared (a larger batch: the handle grows), shared, unweighted and shared calls gives
    the bits a fresh model gives for each of them."""
    cls, synth = ARCHS[arch]
    x = windows[:8].to(gpu)
    w3 = pool_weights(4, 3, seed=13).to(gpu)
    rows, wrows = reference_call(x[:4], w3)
    wflat = torch.rand(8, 293, generator=torch.Generator().manual_seed(14)).to(gpu)
    calls = [(rows, wrows, (4, 3)), (x, wflat, None), (rows, wrows, (4, 3)), (x[:3], None, None), (rows, wrows, (4, 3)),
             (x[[0, 0, 1, 1]], wflat[:4], (2, 2))]
    one = cls(synth(), max_batch=4, repeated_rows="share").to(gpu)
    for i, (a, b, seen) in enumerate(calls):
        got = one(a, b)
        assert one.last_shared == seen, (i, one.last_shared)
        fresh = cls(synth(), max_batch=4, repeated_rows="share").to(gpu)
        assert torch.equal(got, fresh(a, b)), i
        del fresh


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch", list(ARCHS))
def test_repetition_beyond_what_forward_multi_pools(gpu, windows, model, arch, precision):
    """``forward_multi`` pools at most 8 rows per window.  Identical neighbouring chunks repeat more often than that:
    three identical chunks x 3 speakers are 9 equal rows, an all-silent batch of 32 chunks x 3 speakers 96.  Every
    divisor of a repetition is a repetition, so the model runs with the largest divisor <= 8 (9 -> 3, 96 -> 8, 12 -> 6,
    10 speakers -> 5) and takes the ordinary path when that is 1 (11 equal rows) — never an error, and the bits of
    ``forward_multi`` on the grouping that ran."""
    each, shared = model(arch, precision, "each"), model(arch, precision, "share")
    assert shared.MAX_MULTI == 8
    speech, silence = windows[:1].to(gpu), torch.zeros(1, 1, S5, device=gpu)
    for name, x, K, seen in [("3 identical speech chunks x 3", speech.repeat(3, 1, 1), 3, (3, 3)),
                             ("3 silent chunks x 3", silence.repeat(3, 1, 1), 3, (3, 3)),
                             ("4 silent chunks x 3", silence.repeat(4, 1, 1), 3, (2, 6)),
                             ("32 silent chunks x 3", silence.repeat(32, 1, 1), 3, (12, 8)),
                             ("2 distinct chunks x 10 speakers", windows[:2].to(gpu), 10, (4, 5)),
                             ("silence then speech, 9 rows each", torch.cat([silence.repeat(3, 1, 1), speech.repeat(3, 1, 1)]), 3, (6, 3))]:
        B = x.shape[0]
        w = pool_weights(B, K, seed=20 + B + K).to(gpu)
        rows, wrows = reference_call(x, w)
        N = B * K
        got = shared(rows, wrows)
        assert shared.last_shared == seen, (name, shared.last_shared)
        Bs, R = seen
        want = each.forward_multi(rows[::R], wrows.view(Bs, R, -1)).view(N, -1)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), name
    # 11 equal rows: no divisor in 2 .. 8 — today's path, bit for bit
    rows, wrows = reference_call(speech, pool_weights(1, 11, seed=31).to(gpu))
    assert repeat_of(rows[:, 0, :]) == 11
    got = shared(rows, wrows)
    assert shared.last_shared is None and torch.equal(got, each(rows, wrows))


def test_rows_repeat_refuses_a_capturing_stream_and_stays_usable(gpu):
    """The call waits for its answer, so it cannot be captured: it refuses before it enqueues anything, the capture
    itself stays valid and later callers on other streams are not affected."""
    t = torch.full((6, 64), 0.25, device=gpu)
    side = torch.cuda.Stream(gpu)
    fn, ctx = _lib.load().dz_rows_repeat, _lib.context(gpu.index)      # (made before the capture: it allocates)
    assert repeat_of(t) == 6
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    out = torch.zeros(6, 64, device=gpu)
    with torch.cuda.graph(graph, stream=side):
        r = C.c_int(-1)
        rc = fn(ctx, t.data_ptr(), t.stride(0), 6, 64, torch.cuda.current_stream(gpu).cuda_stream, C.byref(r))
        out.copy_(t)
    assert rc == 2 and r.value == -1 and b"captured" in _lib.load().dz_last_error()
    graph.replay()
    torch.cuda.synchronize(gpu)
    assert torch.equal(out, t)
    assert repeat_of(t) == 6
    with torch.cuda.stream(side):
        assert repeat_of(t) == 6
