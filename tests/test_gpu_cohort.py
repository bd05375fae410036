"""The cohort on the GPU: adaptive s-norm of the gallery match (``csrc/k_cohort.hip``).  The yardstick is
torch on float64 CPU tensors,

    d = 1 - (x @ c.T) / (x.norm(dim=1, keepdim=True) * c.norm(dim=1)[None])
    near = d.topk(top_n, dim=1, largest=False).values
    mean, std = near.mean(dim=1), near.std(dim=1, unbiased=False).clamp_min(1e-3)
    dn = 0.5 * ((d_xg - mu_g[None]) / sd_g[None] + (d_xg - mu_x[:, None]) / sd_x[:, None])

With eps = (D + 8) 2^-24, the project's bound of one distance, a mean and a deviation must be within eps + 2^-22 of the
float64 values (order statistics and the population deviation are 1-Lipschitz in the largest perturbation of the values,
the sums run in float64, the rest is the float32 rounding of the stored results), and a normalised distance within

    tol = 0.5 * sum over both sides s of [(2 eps + 2^-22) / sd_s + |d - mu_s| (eps + 2^-22) / (sd_s (sd_s - eps - 2^-22))]
          + 8 * 2^-24 * (1 + |dn|)

computed per element from the float64 values.  Both bounds are derived, not measured.  Synthetic weights and audio."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import _lib, functional
from diart_amd import models as M
from diart_amd.gallery import SpeakerGallery
from diart_amd.pipeline import StreamBatch
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream, synth_streams

pytestmark = pytest.mark.gpu

R = 65
W, HOP = 80000, 8000
FLOOR = 1e-3


def eps(D):
    return (D + 8) * 2.0 ** -24


def names_of(E):
    return [f"v{e}" for e in range(E)]


def strided(x, gpu, pad=4, offset=0):
    """``x`` (R, D) on the GPU as rows ``D + pad`` floats apart, the first ``offset`` floats into a 16-byte aligned
    buffer; the gaps hold NaN, which nothing may read."""
    r, D = x.shape
    buf = torch.full((r * (D + pad) + 8,), float("nan"), dtype=torch.float32, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (r, D), (D + pad, 1), offset)
    view.copy_(x)
    return view


def bits(t):
    t = t.cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32)


def dist64(x, c):
    x, c = x.double(), c.double()
    return 1 - (x @ c.T) / (x.norm(dim=1, keepdim=True) * c.norm(dim=1)[None])


def stats64(sorted_d, top_n):
    near = sorted_d[:, :top_n]
    return near.mean(dim=1), near.std(dim=1, unbiased=False).clamp_min(FLOOR)


_cases = {}


def case(D, M):
    """Inputs and float64 reference of one shape, computed once: x (R, D), g (257, D), c (M, D) standard normal, and
    the sorted float64 distances of x and of g to the cohort."""
    if (D, M) not in _cases:
        gen = torch.Generator().manual_seed(100000 * D + M)
        x, g, c = torch.randn(R, D, generator=gen), torch.randn(257, D, generator=gen), torch.randn(M, D, generator=gen)
        _cases[(D, M)] = (x, g, c, dist64(x, c).sort(dim=1).values, dist64(g, c).sort(dim=1).values)
    return _cases[(D, M)]


def top_ns(M):
    return sorted({n for n in (1, 2, 300, M) if n <= M})


# ------------------------------------------------------------------------------------------- statistics against float64
@pytest.mark.parametrize("M", [1, 2, 65, 129, 300, 8192])
@pytest.mark.parametrize("D", [64, 192])
def test_statistics_against_float64(gpu, D, M):
    x, g, c, sx, sg = case(D, M)
    dx = strided(x.to(gpu), gpu)
    bound = eps(D) + 2.0 ** -22
    for top_n in top_ns(M):
        gallery = SpeakerGallery(names_of(2), g[:2], gpu, cohort=c, top_n=top_n)
        mean, std = (t.cpu() for t in gallery.cohort_stats(dx))
        assert mean.dtype == std.dtype == torch.float32 and mean.shape == std.shape == (R,)
        want_mean, want_std = stats64(sx, top_n)
        e_mean = (mean.double() - want_mean).abs().max().item()
        e_std = (std.double() - want_std).abs().max().item()
        print(f"cohort_stats D={D} M={M} top_n={top_n}: max |mean - float64| = {e_mean:.3e}, |std - float64| = "
              f"{e_std:.3e} (bound {bound:.3e})")
        assert e_mean <= bound and e_std <= bound
        if top_n == 1:
            assert (std == np.float32(FLOOR)).all()
        # the voiceprints' own statistics, computed when the cohort was set
        e_mean, e_std = (torch.from_numpy(a) for a in gallery.entry_stats())
        want_mean, want_std = stats64(sg[:2], top_n)
        assert (e_mean.double() - want_mean).abs().max().item() <= bound
        assert (e_std.double() - want_std).abs().max().item() <= bound
        assert _lib.load().dz_gallery_cohort_size(gallery._handle.h) == M
    one = SpeakerGallery(names_of(1), g[:1], gpu, cohort=c, top_n=top_ns(M)[-1])
    mean1, std1 = one.cohort_stats(x[7:8].to(gpu))                     # R = 1
    assert (mean1.cpu().double() - stats64(sx[7:8], top_ns(M)[-1])[0]).abs().item() <= bound


def test_functional_runs_the_kernels(gpu):
    x, g, c, sx, _ = case(64, 129)
    mean, std = functional.cohort_stats(x.to(gpu).reshape(5, 13, 64), c.to(gpu), 65)
    assert mean.is_cuda and mean.shape == std.shape == (5, 13)
    want = SpeakerGallery(names_of(1), g[:1], gpu, cohort=c, top_n=65).cohort_stats(x.to(gpu))
    assert torch.equal(bits(mean.reshape(-1)), bits(want[0])) and torch.equal(bits(std.reshape(-1)), bits(want[1]))
    got = functional.gallery_match_normalised(x.to(gpu), g[:9].to(gpu), c, top_n=65)
    want = SpeakerGallery(names_of(9), g[:9], gpu, cohort=c, top_n=65).match_normalised(x.to(gpu))
    for a, b in zip(got, want):
        assert a.is_cuda and torch.equal(bits(a), bits(b))
    cpu = functional.gallery_match_normalised(x, g[:9], c, top_n=65)   # the statement itself, for comparison
    assert (got[1].cpu() - cpu[1]).abs().max().item() <= 0.05


# ---------------------------------------------------------------------------------- normalised distance against float64
@pytest.mark.parametrize("D, M, top_n, E, rows", [(64, 8192, 300, 257, R), (192, 300, 300, 129, R), (64, 129, 129, 2, R),
                                                  (192, 65, 65, 1, 1)])
def test_normalised_distance_against_float64(gpu, D, M, top_n, E, rows):
    x, g, c, _, sg = case(D, M)
    x, g = x[:rows].clone(), g[:E]
    planted = [E - 1, 0] if E >= 2 and rows >= 2 else []
    gen = torch.Generator().manual_seed(5)
    for r, e in enumerate(planted):                                    # a voiceprint plus 1 % noise
        x[r] = g[e] + 0.01 * torch.randn(D, generator=gen)
    mu_x, sd_x = stats64(dist64(x, c).sort(dim=1).values, top_n)
    mu_g, sd_g = stats64(sg[:E], top_n)
    assert sd_x.min() > 0.01 and sd_g.min() > 0.01                     # Gaussian rows: far from the floor
    if (D, top_n) == (64, 300):
        assert 0.02 < sd_x.median() < 0.06                             # about 0.03
    d = dist64(x, g)
    dn = 0.5 * ((d - mu_g[None]) / sd_g[None] + (d - mu_x[:, None]) / sd_x[:, None])
    a, b = eps(D) + 2.0 ** -22, 2 * eps(D) + 2.0 ** -22
    tol = 0.5 * (b / sd_g[None] + (d - mu_g[None]).abs() * a / (sd_g * (sd_g - a))[None]
                 + b / sd_x[:, None] + (d - mu_x[:, None]).abs() * a / (sd_x * (sd_x - a))[:, None]) \
        + 8 * 2.0 ** -24 * (1 + dn.abs())

    gallery = SpeakerGallery(names_of(E), g, gpu, cohort=c, top_n=top_n)
    index, dist, second = (t.cpu() for t in gallery.match_normalised(strided(x.to(gpu), gpu)))
    assert index.dtype == torch.int32 and index.shape == dist.shape == second.shape == (rows,)
    assert (index >= 0).all() and (index < E).all()
    at = torch.arange(rows), index.long()
    err = (dist.double() - dn[at]).abs()
    print(f"match_norm D={D} M={M} top_n={top_n} E={E}: max |dn - float64| = {err.max().item():.3e}, the largest "
          f"share of its tolerance {(err / tol[at]).max().item():.3f}; tolerance up to {tol.max().item():.3e}")
    assert (err <= tol[at]).all()
    best = dn.min(dim=1)
    assert (dn[at] <= best.values + 2 * torch.maximum(tol[at], tol[torch.arange(rows), best.indices])).all()
    for r, e in enumerate(planted):
        assert index[r].item() == e and dist[r].item() < -5            # a true match: several units below zero
    if E == 1:
        assert torch.isinf(second).all() and (second > 0).all()
    else:
        assert (second >= dist).all()
        others = dn.clone()
        others[at] = float("inf")
        assert ((second.double() - others.min(dim=1).values).abs() <= tol.max(dim=1).values).all()


# ----------------------------------------------------------------------------------------------------------------- ties
def test_ties_across_the_top_n_th_place_and_between_voiceprints(gpu):
    D, M, top_n = 64, 65, 20
    x, g, c, _, _ = case(D, M)
    c, g = c.clone(), g[:9].clone()
    order = dist64(x[:1], c)[0].argsort()
    for j in (top_n - 3, top_n - 2, top_n, top_n + 1):                 # five equal distances straddle the 20th place of row 0
        c[order[j]] = c[order[top_n - 1]]
    g[5] = g[1]                                                        # one voiceprint under two names
    x = x.clone()
    x[10:20] = 2.0 * g[1] + 0.05 * x[10:20]
    sx = dist64(x, c).sort(dim=1).values
    assert (sx[0, top_n - 3:top_n + 2].max() - sx[0, top_n - 3:top_n + 2].min()) < 1e-15
    gallery = SpeakerGallery(names_of(9), g, gpu, cohort=c, top_n=top_n)
    mean, std = (t.cpu() for t in gallery.cohort_stats(x.to(gpu)))
    want_mean, want_std = stats64(sx, top_n)
    bound = eps(D) + 2.0 ** -22
    assert (mean.double() - want_mean).abs().max().item() <= bound
    assert (std.double() - want_std).abs().max().item() <= bound
    e_mean, e_std = gallery.entry_stats()
    assert e_mean[5].tobytes() == e_mean[1].tobytes() and e_std[5].tobytes() == e_std[1].tobytes()
    index, dist, second = (t.cpu() for t in gallery.match_normalised(x.to(gpu)))
    assert (index[10:20] == 1).all()                                   # the lower index wins
    assert torch.equal(bits(dist[10:20]), bits(second[10:20]))         # the runner-up is the duplicate: the same bits
    assert (index != 5).all()


# ----------------------------------------------------------------------------------------------------------------- bits
def test_bits_depend_on_the_vector_the_cohort_and_top_n_only(gpu):
    D, M, top_n, E = 192, 300, 300, 129
    x, g, c, _, _ = case(D, M)
    g = g[:E]
    gallery = SpeakerGallery(names_of(E), g, gpu, cohort=c, top_n=top_n)
    dx = x.to(gpu)
    assert R == 65
    mean, std = gallery.cohort_stats(dx)
    index, dist, second = gallery.match_normalised(dx)
    # row 64 of 65, and alone
    for got, want in zip(gallery.cohort_stats(dx[64:65]) + gallery.match_normalised(dx[64:65]),
                         (mean, std, index, dist, second)):
        assert torch.equal(bits(got), bits(want[64:65]))
    # row bases 4 and 8 bytes off a 16-byte boundary, and an odd stride
    for pad, offset in ((4, 1), (4, 2), (1, 0), (3, 3)):
        view = strided(dx, gpu, pad, offset)
        assert pad % 4 or view.data_ptr() % 16 == 4 * offset
        for got, want in zip(gallery.cohort_stats(view) + gallery.match_normalised(view),
                             (mean, std, index, dist, second)):
            assert torch.equal(bits(got), bits(want)), (pad, offset)
    # a second call, and another device copy
    again = SpeakerGallery(names_of(E), g, gpu, cohort=c, top_n=top_n)
    for got, want in zip(gallery.cohort_stats(dx) + again.match_normalised(dx), (mean, std, index, dist, second)):
        assert torch.equal(bits(got), bits(want))
    # inside match_norm the statistics are those of cohort_stats: dn is the documented float32 sequence on the raw
    # distance of the same pair, the row's (mean, std) and the voiceprint's
    one = SpeakerGallery(names_of(1), g[7:8], gpu, cohort=c, top_n=top_n)
    raw = one.match(dx)[1].cpu().numpy()
    got = one.match_normalised(dx)[1].cpu().numpy()
    mu_g, sd_g = one.entry_stats()
    mu_x, sd_x = mean.cpu().numpy(), std.cpu().numpy()
    f = np.float32
    want = f(0.5) * ((raw - mu_g[0]) * (f(1) / sd_g[0]) + (raw - mu_x) * (f(1) / sd_x))
    assert want.dtype == np.float32 and want.tobytes() == got.tobytes()
    assert e_bits(gallery.entry_stats(), 7) == e_bits((mu_g, sd_g), 0)  # ... whatever the voiceprint's place


def e_bits(stats, e):
    return stats[0][e].tobytes() + stats[1][e].tobytes()


# ------------------------------------------------------------------------- the two tile kernels give the same d
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("D", [64, 192])
def test_cohort_tile_and_gallery_tile_give_the_same_d(gpu, D, aligned):
    """A cohort equal to the gallery's own voiceprints, top_n = 1: a row's cohort mean is the float64 mean of its ONE
    smallest distance to a member, a division by 1.0 that rounds back to the same float32, so it must be the row's
    smallest raw distance to a voiceprint bit for bit.  The first comes from ``cohort_tile_kernel``'s distances, the
    second from ``gallery_tile_kernel``'s fold: the two copies of the tile's loop must leave the same accumulator bits,
    which is what 4.20's error bound and determinism argument rest on.  E = M = 129 (two gallery tiles, the second with
    one member), R = 65 (two row tiles, the second with one row), the aligned and the single-float loads, one unusable
    row."""
    E = 129
    x, g, _, _, _ = case(D, 129)
    x, g = x.clone(), g[:E]
    x[3] = 0.0                                                         # of zero norm: NaN on both sides
    gallery = SpeakerGallery(names_of(E), g, gpu, cohort=g, top_n=1)
    dx = x.to(gpu) if aligned else strided(x.to(gpu), gpu, pad=3, offset=1)
    assert (dx.data_ptr() % 16 == 0 and dx.stride(0) % 4 == 0) == aligned
    mean = gallery.cohort_stats(dx)[0].cpu().numpy()
    dist = gallery.match(dx)[1].cpu().numpy()
    assert mean.dtype == dist.dtype == np.float32 and mean.shape == dist.shape == (R,)
    assert np.isnan(mean[3]) and np.isnan(dist[3])
    usable = np.arange(R) != 3
    assert np.isfinite(mean[usable]).all() and np.isfinite(dist[usable]).all()
    assert np.array_equal(mean.view(np.uint32), dist.view(np.uint32))


# -------------------------------------------------------------------------------------------------------- unusable rows
def test_unusable_rows_get_nan_and_touch_nobody(gpu):
    x, g, c, _, _ = case(64, 129)
    gallery = SpeakerGallery(names_of(33), g[:33], gpu, cohort=c, top_n=65)
    clean = [t.cpu() for t in gallery.cohort_stats(x[:8].to(gpu)) + gallery.match_normalised(x[:8].to(gpu))]
    y = x[:8].clone()
    y[1, 40], y[2, 0], y[4], y[6, 63] = float("nan"), float("inf"), 0.0, float("-inf")
    bad = torch.tensor([False, True, True, False, True, False, True, False])
    mean, std = (t.cpu() for t in gallery.cohort_stats(y.to(gpu)))
    index, dist, second = (t.cpu() for t in gallery.match_normalised(y.to(gpu)))
    assert torch.isnan(mean[bad]).all() and torch.isnan(std[bad]).all()
    assert (index[bad] == -1).all() and torch.isnan(dist[bad]).all() and torch.isnan(second[bad]).all()
    for got, want in zip((mean, std, index, dist, second), clean):
        assert torch.equal(bits(got[~bad]), bits(want[~bad]))
    huge = torch.full((1, 64), 3e38)                                   # finite elements, a norm beyond float32
    assert gallery.match_normalised(huge.to(gpu))[0].item() == -1
    assert torch.isnan(gallery.cohort_stats(huge.to(gpu))[0]).all()


# ------------------------------------------------------------------------------------------------------------ raw path
def test_raw_match_is_untouched_by_a_cohort(gpu):
    x, g, c, _, _ = case(192, 300)
    plain = SpeakerGallery(names_of(257), g, gpu)
    with_cohort = plain.with_cohort(c, top_n=300)
    dx = strided(x.to(gpu), gpu, pad=3, offset=1)
    with_cohort.match_normalised(dx)                                   # the cohort's scratch has been used
    for a, b in zip(with_cohort.match(dx), plain.match(dx)):
        assert torch.equal(bits(a), bits(b))
    normalised = with_cohort.match_normalised(dx)[1]
    assert not torch.equal(bits(normalised), bits(plain.match(dx)[1]))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_function(gpu):
    x, g, c, _, _ = case(64, 65)
    lib = _lib.load()
    plain = SpeakerGallery(names_of(4), g[:4], gpu)
    plain.match(x.to(gpu))
    h = plain._handle.h
    rows = torch.zeros(4, 64, device=gpu)
    out = torch.zeros(3, 4, dtype=torch.int32, device=gpu)
    o = [out[i].data_ptr() for i in range(3)]
    host = np.zeros(4, np.float32)

    def refused(rc, start, word=""):
        msg = lib.dz_last_error().decode()
        assert rc == 2 and msg.startswith(start) and word in msg, (rc, msg)

    # a handle without a cohort
    assert lib.dz_gallery_cohort_size(h) == 0
    refused(lib.dz_gallery_match_norm(h, rows.data_ptr(), 64, 4, *o, None), "dz_gallery_match_norm:", "no cohort")
    refused(lib.dz_gallery_cohort_stats(h, rows.data_ptr(), 64, 4, o[0], o[1], None), "dz_gallery_cohort_stats:", "no cohort")
    refused(lib.dz_gallery_entry_stats(h, host.ctypes.data, host.ctypes.data), "dz_gallery_entry_stats:", "no cohort")
    # set_cohort
    cn = np.ascontiguousarray(c.numpy())
    big = np.ones((8193, 64), np.float32)
    refused(lib.dz_gallery_set_cohort(h, big.ctypes.data, 8193, 300), "dz_gallery_set_cohort:", "8193 rows")
    refused(lib.dz_gallery_set_cohort(h, cn.ctypes.data, -1, 1), "dz_gallery_set_cohort:", "-1 rows")
    refused(lib.dz_gallery_set_cohort(h, cn.ctypes.data, 65, 0), "dz_gallery_set_cohort:", "top_n = 0")
    refused(lib.dz_gallery_set_cohort(h, cn.ctypes.data, 65, 66), "dz_gallery_set_cohort:", "top_n = 66")
    for value, word in ((np.nan, "cohort row 3 is not finite"), (np.inf, "cohort row 3 is not finite"),
                        (None, "cohort row 3 is of zero norm")):
        broken = cn.copy()
        if value is None:
            broken[3] = 0
        else:
            broken[3, 11] = value
        refused(lib.dz_gallery_set_cohort(h, broken.ctypes.data, 65, 5), "dz_gallery_set_cohort:", word)
    assert lib.dz_gallery_cohort_size(h) == 0                          # nothing was set
    # with a cohort: the row, stride and alignment checks of the raw match, under the new names
    assert lib.dz_gallery_set_cohort(h, cn.ctypes.data, 65, 5) == 0 and lib.dz_gallery_cohort_size(h) == 65
    p = rows.data_ptr()
    for args, word in [((p, 64, 0, *o), "0 rows"), ((p, 64, 4097, *o), "4097 rows"),
                       ((p, 63, 4, *o), "row stride 63 below the dimension 64"), ((None, 64, 4, *o), "NULL rows or output"),
                       ((p, 64, 4, o[0], None, o[2]), "NULL"), ((p + 2, 64, 4, *o), "aligned")]:
        refused(lib.dz_gallery_match_norm(h, *args, None), "dz_gallery_match_norm:", word)
        refused(lib.dz_gallery_cohort_stats(h, *args[:3], args[3], args[4], None), "dz_gallery_cohort_stats:", word)
    refused(lib.dz_gallery_entry_stats(h, None, host.ctypes.data), "dz_gallery_entry_stats:", "NULL")
    # NULL / M = 0 removes it again
    assert lib.dz_gallery_set_cohort(h, None, 0, 0) == 0 and lib.dz_gallery_cohort_size(h) == 0
    refused(lib.dz_gallery_match_norm(h, p, 64, 4, *o, None), "dz_gallery_match_norm:", "no cohort")
    with pytest.raises(ValueError, match="dimension"):
        plain.with_cohort(c, 5).match_normalised(torch.zeros(4, 128, device=gpu))


# --------------------------------------------------------------------------------------------------------------- engine
def _plain_names():
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gallery_host import PlainNames
    return PlainNames


def _run(pipe, d_audio, steps):
    """-> per step (emb, assign, the ticket's match, names, match_normalised), copies."""
    out = []
    for t in range(steps):
        ticket = pipe.launch(d_audio[:, t * HOP:t * HOP + W])
        _, emb, _, assign = pipe.finish(ticket, want_scores=False)
        match = tuple(m.copy() for m in ticket["match"]) if "match" in ticket else None
        out.append((emb.copy(), assign.copy(), match, ticket.get("names"), ticket.get("match_normalised")))
    return out


def _plant(first, n, D, seed):
    """A gallery of one assigned, finite embedding per stream (from step 2 or the first later step that has one, so
    the name arrives mid-stream) + 100 random distractors -> (names, rows, {stream: (step, g)})."""
    names, rows, where = [], [], {}
    for i in range(n):
        for t in list(range(2, len(first))) + [1, 0]:
            emb, assign = first[t][:2]
            ks = [k for k in range(assign.shape[1]) if assign[i, k] >= 0 and np.isfinite(emb[i, k]).all()]
            if ks:
                names.append(f"plant{i}")
                rows.append(emb[i, ks[0]].copy())
                where[i] = (t, int(assign[i, ks[0]]))
                break
    assert len(where) >= 1, "no stream had an assigned speaker: the synthetic audio changed"
    noise = np.random.default_rng(seed).standard_normal((100, D)).astype(np.float32)
    return names + [f"distractor{j}" for j in range(100)], np.concatenate([np.stack(rows), noise]), where


def test_engine_names_planted_speakers_by_the_normalised_distance(gpu):
    steps, n = 6, 4
    pipe = StreamBatch(M.HipSegmentation(synth_segmentation_state(), max_batch=n),
                       M.HipEmbedding(synth_embedding_state(), max_batch=n), n, device=gpu, tail=True)
    D = pipe.emb.dimension
    d_audio = torch.from_numpy(synth_streams(n, (W + HOP * steps) / 16000.0, seed0=300)).to(gpu)
    first = _run(pipe, d_audio, steps)
    assert all(s[2] is None and s[3] is None and s[4] is None for s in first)
    names, rows, where = _plant(first, n, D, seed=11)
    cohort = np.random.default_rng(12).standard_normal((300, D)).astype(np.float32)
    gallery = SpeakerGallery(names, rows, gpu, cohort=cohort)
    assert gallery.top_n == 300
    # the threshold: half way from the float64 dn of the planted pairs to zero
    index, dn, _ = functional.gallery_match_normalised(rows[:len(where)], rows, cohort)
    assert index.tolist() == list(range(len(where))) and dn.max() < -2
    delta = 0.5 * float(dn.max())
    # The synthetic streams' embeddings lie close to one another, so a planted voiceprint may rank below ANOTHER
    # stream's, whose deviation against the cohort is narrower: that is the normalisation at work.  What is fixed is
    # the rule: the names are those of its plain restatement, and the speaker whose embedding was enrolled is within
    # the threshold of a planted voiceprint in that very step.
    P = len(where)
    cross = np.stack([functional.gallery_match_normalised(rows[:P], rows[j:j + 1], cohort)[1] for j in range(P)], axis=1)
    print(f"float64 dn of the planted rows against the planted voiceprints:\n{cross}\ndelta_id = {delta:.3f}")

    pipe.set_gallery(gallery, delta)
    pipe.reset()
    second = _run(pipe, d_audio, steps)
    lowest = np.inf
    plain = _plain_names()(n, pipe.max_speakers, delta)
    for t, (emb, assign, match, got_names, normalised) in enumerate(second):
        assert emb.tobytes() == first[t][0].tobytes() and assign.tobytes() == first[t][1].tobytes()
        assert normalised is True
        for a, b in zip(match, gallery.match_normalised(emb)):
            assert a.shape == (n, emb.shape[1]) and bits(a).equal(bits(b)), t
        lowest = min(lowest, np.nanmin(match[1]))
        plain.update(assign, match[0], match[1], range(n))
        assert got_names == plain.labels(gallery.names, range(n)), t
        for i, (t0, g) in where.items():
            if t >= t0:                                                # named from the step its embedding occurs in
                assert got_names[i] and all(name.startswith("plant") for name in got_names[i].values()), (t, i)
            if t == t0:
                k = int(np.nonzero(assign[i] == g)[0][0])
                assert names[match[0][i, k]].startswith("plant") and match[1][i, k] <= dn[list(where).index(i)] + 1e-3
    # a threshold below every normalised distance of the run: nobody is named
    pipe.set_gallery(gallery, float(lowest) - 1.0)
    pipe.reset()
    assert all(not any(step[3]) for step in _run(pipe, d_audio, steps))
    # the same gallery without its cohort takes the raw path and refuses that threshold
    raw = gallery.with_cohort(None)
    with pytest.raises(ValueError, match="set_gallery.*delta_id"):
        pipe.set_gallery(raw, delta)
    pipe.set_gallery(raw, 0.3)
    pipe.reset()
    for (emb, _, match, _, normalised) in _run(pipe, d_audio, 2):
        assert normalised is False
        for a, b in zip(match, raw.match(emb)):
            assert bits(a).equal(bits(b))


# --------------------------------------------------------------------------------------------------------------- server
def _serve(gpu, states, audio, gallery, delta, ticks=18):
    """Two streams from tick 0 -> (the labels seen per stream, the log of every engine step: slots, emb, assign)."""
    from diart_amd.serve import StreamServer
    srv = StreamServer(M.HipSegmentation(states[0], max_batch=2), M.HipEmbedding(states[1], max_batch=2), max_streams=2,
                       device=gpu)
    if gallery is not None:
        srv.set_gallery(gallery, delta)
    log, finish = [], srv.batch.finish

    def logged(ticket, want_scores=True):
        res = finish(ticket, want_scores)
        if not srv.batch._warming:
            log.append((list(ticket["slots"]), res[1].copy(), res[3].copy(), ticket.get("match_normalised")))
        return res

    srv.batch.finish = logged
    seen = {k: set() for k in audio}
    for k in audio:
        srv.open(k)
    for tick in range(ticks):
        for k in audio:
            srv.push(k, audio[k][tick * HOP:(tick + 1) * HOP])
        for k, ann in srv.step().items():
            seen[k] |= {lab for _, _, lab in ann.itertracks(yield_label=True)}
    for k in audio:
        srv.close(k)
    return seen, log


def test_server_labels_the_turns_with_a_cohort_gallery(gpu):
    states = synth_segmentation_state(), synth_embedding_state()
    audio = {"ann": synth_stream(300, 9.0), "ben": synth_stream(301, 9.0)}
    seen, log = _serve(gpu, states, audio, None, None)
    assert all(lab.startswith("speaker") for labs in seen.values() for lab in labs) and any(seen.values())
    # per stream the first embedding assigned to a speaker that was heard: that is its voiceprint
    names, rows = [], []
    for slot, k in enumerate(audio):
        heard = {int(lab[len("speaker"):]) for lab in seen[k]}
        found = next((emb[s.index(slot), q] for s, emb, assign, _ in log if slot in s
                      for q in range(assign.shape[1])
                      if assign[s.index(slot), q] in heard and np.isfinite(emb[s.index(slot), q]).all()), None)
        if found is not None:
            names.append(f"plant-{k}")
            rows.append(found.copy())
    assert names, "no stream had a turn: the synthetic audio changed"
    rng = np.random.default_rng(5)
    rows = np.concatenate([np.stack(rows), rng.standard_normal((50, 512)).astype(np.float32)])
    cohort = rng.standard_normal((300, 512)).astype(np.float32)
    gallery = SpeakerGallery(names + [f"distractor{j}" for j in range(50)], rows, gpu, cohort=cohort)
    dn = gallery.match_normalised(rows[:len(names)])[1]
    assert dn.max() < -2
    named, named_log = _serve(gpu, states, audio, gallery, 0.5 * float(dn.max()))
    assert all(entry[3] is True for entry in named_log)
    for (_, emb, assign, _), (_, emb2, assign2, _) in zip(log, named_log):     # the gallery changes nothing it reads
        assert emb.tobytes() == emb2.tobytes() and assign.tobytes() == assign2.tobytes()
    for name in names:
        assert name in named[name[len("plant-"):]], named
