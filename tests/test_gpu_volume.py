"""The volume adjustment on the GPU (DESIGN.md "Volume adjustment"): ``dz_adjust_volume`` against the float64
restatement of the reference's block (tests/test_volume.py) over the row counts, lengths, channel counts, strides and
targets at which the kernel takes another path; the rows the reference turns into NaN; bit-for-bit independence of
alignment, batch and call; the argument checks; and the functional form and the ``AdjustVolume`` block on top of it."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import _lib
from diart_amd.blocks import AdjustVolume
from diart_amd.features import SlidingWindow, SlidingWindowFeature
from diart_amd.functional import adjust_volume, adjust_volume_rows

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_volume as V  # noqa: E402  (the float64 restatement)

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 65)
SAMPLES = (1, 3, 255, 256, 257, 1031)
PADS = (0, 1, 3)                      # row stride = the row, + 1 and + 3 floats
TARGETS = (-20.0, 0.0, 6.0)
AMPLITUDES = (0.01, 0.3, 2.0)
# four float32 roundings of 2^-24 each (gain, peak, product, quotient): twice their sum, plus the smallest normal
REL, TINY = 5e-7, float(np.finfo(np.float32).tiny)


def signals(rows, samples, channels, seed):
    """(rows, samples, channels) float32 Gaussian noise, row r at amplitude AMPLITUDES[r % 3]."""
    rng = np.random.default_rng(seed)
    amp = np.array([AMPLITUDES[r % 3] for r in range(rows)])[:, None, None]
    return (rng.standard_normal((rows, samples, channels)) * amp).astype(np.float32)


def strided(x3, pad, dev, fill=0.0):
    """x3 (rows, samples, channels) on the host -> a device view (rows, samples * channels) whose rows are
    samples * channels + pad floats apart (the padding holds ``fill``)."""
    R, S, C = x3.shape
    buf = torch.full((R, S * C + pad), fill, dtype=torch.float32, device=dev)
    view = buf[:, :S * C]
    view.copy_(torch.from_numpy(x3.reshape(R, S * C)))
    return buf, view


def run(x3, db, pad, in_place, dev):
    R, S, C = x3.shape
    buf, view = strided(x3, pad, dev, fill=7.0)
    if in_place:
        out = adjust_volume_rows(view, db, out=view, channels=C)
        assert out is view
        obuf = buf
    else:
        obuf, oview = strided(np.zeros_like(x3), pad, dev, fill=7.0)
        out = adjust_volume_rows(view, db, out=oview, channels=C)
        kept = buf.cpu().numpy()[:, :S * C]
        assert np.array_equal(kept.view(np.uint32), x3.reshape(R, -1).view(np.uint32)), "the input was written"
    assert bool((obuf[:, S * C:] == 7.0).all()), "the kernel wrote between two rows"
    return out.cpu().numpy().reshape(R, S, C)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, x3, db, want, where):
    """The per-sample bound, the volume of the plain rows and the peak of the saturating rows."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    err = np.abs(got.astype(np.float64) - want)
    bound = REL * np.abs(want) + TINY
    worst = float(np.max(err / bound))
    assert worst <= 1.0, (where, worst)
    top = np.max(np.abs(want), axis=1)                                                    # (rows, channels)
    gain = 10.0 ** ((db - V.volumes_f64(x3)[:, 0]) / 20.0)
    scaled_peak = gain * np.max(np.abs(x3.astype(np.float64)), axis=1)                    # before the clamp
    plain, sat = scaled_peak < 1.0 - 1e-5, scaled_peak > 1.0 + 1e-5
    vol = V.volumes_f64(got)[:, 0]
    if plain.any():
        assert np.max(np.abs(vol[plain] - db)) <= 1e-5, (where, "volume of the plain rows")
    if sat.any():
        assert np.all(np.max(np.abs(got), axis=1)[sat] == 1.0), (where, "peak of the saturating rows")
        assert np.all(top[sat] <= 1.0 + 1e-12)
    return worst, int(plain.sum()), int(sat.sum())


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_kernel_matches_the_float64_restatement(gpu, channels):
    """Every (rows, samples, stride, in place / out of place, target) of the lists above, and 3 rows of 80 000
    samples.  Bound per sample: 5e-7 |expected| + the smallest normal float32."""
    worst, n_plain, n_sat = 0.0, 0, 0
    shapes = [(r, s) for r in ROWS for s in SAMPLES] + [(3, 80000)]
    for i, (rows, samples) in enumerate(shapes):
        x3 = signals(rows, samples, channels, 100 * i + channels)
        for db in TARGETS:
            want = V.adjust_volume_f64(x3, db)                  # once per input and target
            for pad in PADS:
                for in_place in (False, True):
                    got = run(x3, db, pad, in_place, gpu)
                    w, p, s = check(got, x3, db, want, (rows, samples, channels, db, pad, in_place))
                    worst, n_plain, n_sat = max(worst, w), n_plain + p, n_sat + s
    print(f"channels {channels}: worst error / bound {worst:.3f}; {n_plain} plain and {n_sat} saturating signals")
    assert n_plain > 0 and n_sat > 0


SPECIAL = ("zeros", "nan_first", "nan_middle", "nan_last", "inf")


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("kind", SPECIAL)
def test_special_rows_come_out_nan_and_leave_the_others_alone(gpu, kind, channels):
    """Row 2 of a 5-row batch is all zeros, or holds one NaN (first, middle, last sample) or one +Inf: that signal comes
    out all NaN, every other signal is bit-equal to the call without the special row (with two channels only the
    special row's channel 1 is touched: its channel 0 stays an ordinary signal)."""
    S, ch = 1031, channels - 1
    base = signals(5, S, channels, 4242)
    x3 = base.copy()
    if kind == "zeros":
        x3[2, :, ch] = 0.0
    else:
        at = {"nan_first": 0, "nan_middle": S // 2, "nan_last": S - 1, "inf": 17}[kind]
        x3[2, at, ch] = np.inf if kind == "inf" else np.nan
    for pad in (0, 1):
        got = run(x3, -20.0, pad, False, gpu)
        assert np.isnan(got[2, :, ch]).all(), kind
        keep = np.ones((5, channels), bool)
        keep[2, ch] = False
        others = run(np.delete(base, 2, axis=0), -20.0, pad, False, gpu)
        plain = run(base, -20.0, pad, False, gpu)
        assert np.isfinite(plain).all()
        assert np.array_equal(bits(np.delete(got, 2, axis=0)), bits(others))
        for r in range(5):
            for c in range(channels):
                if keep[r, c]:
                    assert np.array_equal(bits(got[r, :, c]), bits(plain[r, :, c])), (kind, r, c)


@pytest.mark.parametrize("channels", [1, 3])
def test_a_row_does_not_depend_on_its_batch_its_alignment_or_the_call(gpu, channels):
    for samples in (257, 1031, 20483):     # 20 483: the unrolled loop, the plain loop and the tail
        x3 = signals(65, samples, channels, 9000 + samples)
        first = run(x3, 0.0, 0, False, gpu)
        assert np.array_equal(bits(first), bits(run(x3, 0.0, 0, False, gpu)))             # two calls
        for pad in (1, 3):                                                              # rows at every float alignment
            assert np.array_equal(bits(first), bits(run(x3, 0.0, pad, True, gpu)))
        for r in (0, 17, 64):                                                           # alone == inside the batch
            alone = run(x3[r:r + 1], 0.0, 0, False, gpu)
            assert np.array_equal(bits(alone[0]), bits(first[r])), (samples, r)
        # and at a base that is only 4-byte aligned
        buf = torch.zeros(samples * channels + 1, device=gpu)
        view = buf[1:].view(1, -1)
        view.copy_(torch.from_numpy(x3[5].reshape(1, -1)))
        off = adjust_volume_rows(view, 0.0, channels=channels).cpu().numpy().reshape(samples, channels)
        assert np.array_equal(bits(off), bits(first[5]))


def test_bad_arguments_return_the_library_error_and_launch_nothing(gpu):
    lib, ctx = _lib.load(), _lib.context(gpu.index)
    x = torch.ones((4, 64), device=gpu)
    y = torch.full((4, 64), 7.0, device=gpu)
    st = torch.cuda.current_stream(gpu).cuda_stream

    def call(ctx=ctx, src=x.data_ptr(), in_stride=64, dst=y.data_ptr(), out_stride=64, rows=4, samples=64, channels=1,
             db=-20.0):
        return lib.dz_adjust_volume(ctx, src, in_stride, dst, out_stride, rows, samples, channels, db, st)

    bad = [dict(ctx=None), dict(src=None), dict(dst=None), dict(rows=0), dict(rows=-1), dict(samples=0),
           dict(channels=0), dict(channels=9), dict(in_stride=63), dict(out_stride=63),
           dict(samples=32, channels=3, in_stride=64), dict(db=float("nan")), dict(db=float("inf")),
           dict(db=float("-inf"))]
    for kw in bad:
        assert call(**kw) == 2, kw
        assert b"dz_adjust_volume" in lib.dz_last_error()
    torch.cuda.synchronize(gpu)
    assert bool((y == 7.0).all()) and bool((x == 1.0).all())
    assert call() == 0                                               # and the same call with good arguments runs
    torch.cuda.synchronize(gpu)
    assert bool(torch.isfinite(y).all()) and not bool((y == 7.0).any())
    with pytest.raises(ValueError):
        adjust_volume_rows(x, -20.0, channels=3)                     # 64 values are no whole number of 3-channel frames
    with pytest.raises(ValueError):
        adjust_volume_rows(x, float("nan"))


# ---------------------------------------------------------------------------------------- functional form and block
def test_functional_keeps_kind_and_device(gpu):
    x = signals(3, 1031, 1, 77)[:, :, 0]                             # (3, samples)
    want = V.adjust_volume_f64(x[:, :, None], -20.0)[:, :, 0]
    on_host = adjust_volume(torch.from_numpy(x), -20.0)
    assert isinstance(on_host, torch.Tensor) and on_host.device.type == "cpu" and on_host.dtype == torch.float32
    on_gpu = adjust_volume(torch.from_numpy(x).to(gpu), -20.0)
    assert on_gpu.device == gpu
    arr = adjust_volume(x, -20.0)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == x.shape
    assert np.array_equal(bits(arr), bits(on_host.numpy())) and np.array_equal(bits(arr), bits(on_gpu.cpu().numpy()))
    assert np.all(np.abs(arr - want) <= REL * np.abs(want) + TINY)
    # leading axes and a non-contiguous last axis
    lead = adjust_volume(torch.from_numpy(x).reshape(3, 1, 1031).to(gpu), -20.0)
    assert tuple(lead.shape) == (3, 1, 1031) and np.array_equal(bits(lead.cpu().numpy()[:, 0]), bits(arr))
    col = torch.from_numpy(np.ascontiguousarray(x.T)).to(gpu).T      # (3, samples) with stride (1, 3)
    assert np.array_equal(bits(adjust_volume(col, -20.0).cpu().numpy()), bits(arr))
    one = adjust_volume(x[0], -20.0)                                 # a single signal
    assert one.shape == (1031,) and np.array_equal(bits(one), bits(arr[0]))


def test_block_restores_the_input_type_and_equals_the_functional_form(gpu):
    x3 = signals(3, 1031, 2, 78)                                     # (batch, samples, channels)
    block = AdjustVolume(-20.0, gpu)
    fn = adjust_volume(np.ascontiguousarray(x3.transpose(0, 2, 1)), -20.0).transpose(0, 2, 1)
    # tensors: on the device they came on
    t_host = block(torch.from_numpy(x3))
    assert isinstance(t_host, torch.Tensor) and t_host.device.type == "cpu" and tuple(t_host.shape) == x3.shape
    t_gpu = block(torch.from_numpy(x3).to(gpu))
    assert t_gpu.device == gpu
    arr = block(x3)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == x3.shape
    for got in (t_host.numpy(), t_gpu.cpu().numpy(), arr):
        assert np.array_equal(bits(got), bits(fn))
    want = V.adjust_volume_f64(x3, -20.0)
    assert np.all(np.abs(arr - want) <= REL * np.abs(want) + TINY)
    # (samples, channels): an array gains the batch axis (the formatter's rule), a SlidingWindowFeature does not
    two = block(x3[1])
    assert two.shape == (1,) + x3[1].shape and np.array_equal(bits(two[0]), bits(fn[1]))
    sw = SlidingWindow(start=2.5, duration=1 / 16384, step=1 / 16384)
    swf = block(SlidingWindowFeature(x3[1], sw))
    assert isinstance(swf, SlidingWindowFeature) and swf.data.shape == x3[1].shape
    assert np.array_equal(bits(swf.data), bits(fn[1]))
    got_sw = swf.sliding_window
    assert (got_sw.start, got_sw.duration, got_sw.step) == (sw.start, sw.duration, sw.step)
    # get_volumes of the output: the plain signals sit at the target
    vols = AdjustVolume.get_volumes(torch.from_numpy(arr)).numpy()
    assert vols.shape == (3, 1, 2)
    assert np.all(np.abs(vols[0] + 20.0) < 1e-4) and np.all(vols <= -20.0 + 1e-4)
