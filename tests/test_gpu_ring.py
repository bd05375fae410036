"""The audio ring's one push path and one gather kernel (``csrc/ring.hip``): lock-step pushes, per-row pushes across the
64-rows-per-launch boundary, their interplay, and the alternation and growth of the landing blocks.

Every expectation is a block history kept in numpy, compared bit for bit; float blocks are random 32-bit patterns (NaNs
with payloads, denormals), which a push must copy as they are."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd.pipeline import AudioRing

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_ingest_formats import restate, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

PLACES = ("pageable", "pinned", "device")


def any_bits(rng, shape):
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def place(a: np.ndarray, where: str, gpu, pad: int = 0) -> torch.Tensor:
    """``a`` (rows, values) as a pageable / pinned host tensor or a device tensor; ``pad`` > 0: as the leading columns
    of a tensor that many values wider, so that its rows are strided."""
    t = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.from_numpy(a[:0]).dtype)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    t = t.pin_memory() if where == "pinned" else t.to(gpu) if where == "device" else t
    return t[:, :a.shape[1]]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hop", [4, 1028, 8000])
def test_lock_step_push_on_an_aligned_ring(gpu, hop, n):
    """hop 4: one lane; 1 028: one full block of 1 024 frames plus one lane; 8 000: a ragged last block (832 frames).
    Pageable, pinned and device blocks in turn, one block in three a strided view; ``snapshot()`` and ``gather`` of all
    rows after every push from the first complete window on."""
    W = 4 * hop
    ring = AudioRing(n, W, hop, slack_blocks=2, device=gpu)
    rng = np.random.default_rng(hop + n)
    hist = np.zeros((n, 0), dtype=np.float32)
    out = torch.empty(n, W, device=gpu)
    keep = []                                   # pinned blocks are read in place: alive until the stream has passed
    for t in range(3 * W // hop + 2):
        a = any_bits(rng, (n, hop))
        blk = place(a, PLACES[t % 3], gpu, pad=4 if t % 3 == (t // 3) % 3 else 0)
        keep.append(blk)
        full = ring.push(blk)
        hist = np.concatenate([hist, a], axis=1)[:, -W:]
        assert full == (hist.shape[1] == W) and ring.filled == hist.shape[1]
        if full:
            assert same_bits(ring.snapshot(), hist), t
            assert same_bits(ring.gather(list(range(n)), out), hist), t


def encoded(rng, fmt, channels, k, hop):
    """(the block as pushed (k, hop * channels), its float32 mono (k, hop))"""
    if (fmt, channels) == ("f32", 1):
        a = any_bits(rng, (k, hop))
        return a, a
    if fmt == "f32":
        a = rng.uniform(-1, 1, size=(k, hop, channels)).astype(np.float32)
    elif fmt == "s16":
        a = rng.integers(-32768, 32768, size=(k, hop, channels), dtype=np.int16)
    else:
        a = rng.integers(0, 256, size=(k, hop, channels), dtype=np.uint8)
    return a.reshape(k, -1), restate(a, fmt, channels)


@pytest.mark.parametrize("fmt,channels", [("f32", 1), ("s16", 2), ("ulaw", 1)])
@pytest.mark.parametrize("hop", [1028, 1030])
def test_pushes_and_gathers_across_the_64_row_boundary(gpu, hop, fmt, channels):
    """130 rows: a lock-step push (one launch), then per-row pushes and gathers of 65 and of 130 scrambled rows (two
    and three launches of 64 rows).  hop 1 030: an unaligned ring, single-frame pushes and 4-byte gathers."""
    n, W = 130, 2 * hop
    ring = AudioRing(n, W, hop, slack_blocks=1, device=gpu)
    rng = np.random.default_rng(hop + channels)
    first = any_bits(rng, (n, hop))
    blocks = [place(first, "pinned", gpu)]
    ring.push(blocks[0])
    hist = [first[r] for r in range(n)]
    kw = {} if fmt == "f32" else {"channels": channels, "format": fmt}
    for k, where in ((65, "pageable"), (130, "device")):
        rows = rng.permutation(n)[:k].tolist()
        raw, mono = encoded(rng, fmt, channels, k, hop)
        blocks.append(place(raw, where, gpu))
        ring.push_rows(blocks[-1], rows, **kw)
        for j, r in enumerate(rows):
            hist[r] = np.concatenate([hist[r], mono[j]])[-W:]
    assert [ring.filled_row(r) for r in range(n)] == [W] * n
    out = torch.empty(n, W, device=gpu)
    for k in (65, 130):
        rows = rng.permutation(n)[:k].tolist()
        assert same_bits(ring.gather(rows, out), np.stack([hist[r] for r in rows])), k


def test_lock_step_and_per_row_pushes_interplay(gpu):
    """The ring's state rules, as a host model.  The ring has one common write position ``pos`` and, per row, a write
    position and a block count.  A per-row push writes the listed rows at their own positions and advances those
    (position + hop modulo P, count + 1); ``pos`` stays.  A lock-step push writes EVERY row at ``pos`` — wherever the
    row's own position was — advances ``pos``, sets every row's position to the new ``pos`` and adds one to every
    count.  ``filled_row`` is min(W, count x hop); ``filled`` is min(W, pushes x hop) over the push calls of either
    kind.  A row's window is the W samples in front of its position, modulo P (never-written samples are 0)."""
    n, hop = 3, 1028
    W, slack = 4 * hop, 2
    P = W + slack * hop
    ring = AudioRing(n, W, hop, slack_blocks=slack, device=gpu)
    rng = np.random.default_rng(5)
    model = np.zeros((n, P), dtype=np.float32)
    pos, rpos, count, pushes = 0, [0] * n, [0] * n, 0
    out = torch.empty(1, W, device=gpu)
    for rows in ([2], [2], None, [0], None, None, None, None):
        a = any_bits(rng, (n if rows is None else len(rows), hop))
        if rows is None:
            ring.push(place(a, "pageable", gpu))
            model[:, pos:pos + hop] = a
            pos = (pos + hop) % P
            rpos, count = [pos] * n, [c + 1 for c in count]
        else:
            ring.push_rows(place(a, "pageable", gpu), rows)
            for j, r in enumerate(rows):
                model[r, rpos[r]:rpos[r] + hop] = a[j]
                rpos[r], count[r] = (rpos[r] + hop) % P, count[r] + 1
        pushes += 1
        assert [ring.filled_row(r) for r in range(n)] == [min(W, c * hop) for c in count]
        assert ring.filled == min(W, pushes * hop)
        for r in range(n):
            if count[r] * hop >= W:
                want = model[r, (rpos[r] - W + np.arange(W)) % P]
                assert same_bits(ring.gather([r], out), want[None]), (rows, r)
    assert min(count) * hop >= W


@pytest.mark.parametrize("where", ["pageable", "pinned"])
def test_landing_blocks_alternate_and_grow(gpu, where):
    """Six pushes of host blocks with no synchronisation between them: each must be read from its own landing block
    (or in place, pinned) after the next one has been queued, and the second push (float32, 5 channels) outgrows the
    landing blocks the ring was created with."""
    n, hop = 4, 4112
    W = 6 * hop
    ring = AudioRing(n, W, hop, slack_blocks=0, device=gpu)
    rng = np.random.default_rng(9)
    hist = [np.zeros(0, dtype=np.float32) for _ in range(n)]
    keep = []
    for fmt, channels in (("u8", 1), ("f32", 5), ("s16", 2), ("f32", 1), ("f32", 1), ("f32", 1)):
        rows = rng.permutation(n).tolist()
        raw, mono = encoded(rng, fmt, channels, n, hop)
        keep.append(place(raw, where, gpu))
        ring.push_rows(keep[-1], rows, channels=channels, format=fmt)
        for j, r in enumerate(rows):
            hist[r] = np.concatenate([hist[r], mono[j]])
    torch.cuda.synchronize()
    got = ring.gather(list(range(n)), torch.empty(n, W, device=gpu))
    assert same_bits(got, np.stack(hist))
