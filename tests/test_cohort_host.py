"""The cohort (adaptive s-norm of the gallery match) without a GPU: the float64 statements of
``functional.cohort_stats`` / ``gallery_match_normalised`` against a plain per-row numpy loop (sort, slice, ``mean``,
``std``), the signed threshold of ``SpeakerNames``, the save / load round trip of a cohort, and every refusal that
needs no GPU, ``TuneCache.with_gallery`` included."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cases as tc  # noqa: E402

from diart_amd import _lib, functional  # noqa: E402
from diart_amd.gallery import SpeakerGallery, SpeakerNames, check_delta_id  # noqa: E402
from diart_amd.optim import TuneCache  # noqa: E402

FLOOR = 1e-3


def _rows(n, D, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def plain_stats(x, c, top_n):
    """Row by row: the cosine distances to the cohort sorted, the first top_n of them, their mean and std."""
    x, c = x.astype(np.float64), c.astype(np.float64)
    mean, std = np.empty(len(x)), np.empty(len(x))
    for r, row in enumerate(x):
        d = np.array([1 - row @ m / (np.linalg.norm(row) * np.linalg.norm(m)) for m in c])
        near = np.sort(d)[:top_n]
        mean[r], std[r] = near.mean(), max(near.std(), FLOOR)
    return mean, std


def plain_dn(x, g, c, top_n):
    mu_x, sd_x = plain_stats(x, c, top_n)
    mu_g, sd_g = plain_stats(g, c, top_n)
    x, g = x.astype(np.float64), g.astype(np.float64)
    dn = np.empty((len(x), len(g)))
    for r, row in enumerate(x):
        for e, v in enumerate(g):
            d = 1 - row @ v / (np.linalg.norm(row) * np.linalg.norm(v))
            dn[r, e] = 0.5 * ((d - mu_g[e]) / sd_g[e] + (d - mu_x[r]) / sd_x[r])
    return dn


# ----------------------------------------------------------------------------------------------- the float64 statements
@pytest.mark.parametrize("M, top_n", [(1, 1), (40, 1), (40, 7), (40, 40), (301, 300)])
def test_cohort_stats_on_cpu_is_the_plain_loop(M, top_n):
    x, c = _rows(9, 64, 1), _rows(M, 64, 2)
    mean, std = functional.cohort_stats(torch.from_numpy(x), torch.from_numpy(c), top_n)
    assert mean.dtype == std.dtype == torch.float32 and mean.shape == std.shape == (9,)
    want_mean, want_std = plain_stats(x, c, top_n)
    assert np.abs(mean.numpy() - want_mean).max() <= 2.0 ** -23       # float64 both ways, then one float32 rounding
    assert np.abs(std.numpy() - want_std).max() <= 2.0 ** -23
    if top_n == 1:
        assert (std == np.float32(FLOOR)).all()                        # one value has no deviation: the floor


def test_cohort_stats_numpy_shapes_and_unusable_rows():
    x, c = _rows(6, 64, 3).reshape(2, 3, 64), _rows(30, 64, 4)
    x[0, 1, 5], x[1, 0], x[1, 2, 63] = np.nan, 0.0, np.inf
    mean, std = functional.cohort_stats(x, c, 10)
    assert isinstance(mean, np.ndarray) and mean.shape == std.shape == (2, 3) and mean.dtype == np.float32
    bad = np.array([[False, True, False], [True, False, True]])
    assert np.isnan(mean[bad]).all() and np.isnan(std[bad]).all()
    want = plain_stats(x.reshape(6, 64)[~bad.reshape(-1)], c, 10)
    assert np.abs(mean[~bad] - want[0]).max() <= 2.0 ** -23 and np.abs(std[~bad] - want[1]).max() <= 2.0 ** -23


@pytest.mark.parametrize("E", [1, 2, 17])
def test_match_normalised_on_cpu_is_the_plain_loop(E):
    x, g, c = _rows(11, 64, 5), _rows(E, 64, 6), _rows(50, 64, 7)
    index, dist, second = functional.gallery_match_normalised(torch.from_numpy(x), torch.from_numpy(g),
                                                              torch.from_numpy(c), top_n=20)
    assert index.dtype == torch.int32 and dist.dtype == second.dtype == torch.float32
    dn = plain_dn(x, g, c, 20)
    assert np.array_equal(index.numpy(), dn.argmin(axis=1))
    tol = 1e-9 + 2.0 ** -23 * np.abs(dn).max()
    assert np.abs(dist.numpy() - dn.min(axis=1)).max() <= tol
    if E == 1:
        assert torch.isinf(second).all() and (second > 0).all()
    else:
        assert np.abs(second.numpy() - np.sort(dn, axis=1)[:, 1]).max() <= tol
    assert (dn.min(axis=1) < dn.mean(axis=1) + 1e-12).all()


def test_match_normalised_is_signed_and_finds_planted_rows():
    g, c = _rows(8, 64, 8), _rows(200, 64, 9)
    x = g[[3, 6]] + 0.01 * _rows(2, 64, 10)
    index, dist, second = functional.gallery_match_normalised(x, g, c, top_n=50)
    assert index.tolist() == [3, 6]
    assert (dist < -5).all() and (second > dist + 5).all()            # a true match: several units below zero


def test_match_normalised_unusable_rows_ties_and_default_top_n():
    g, c = _rows(4, 64, 11), _rows(300, 64, 12)
    g[2] = g[0]                                                        # equal values: the lowest index
    x = np.stack([g[0] * 2, np.full(64, np.nan, np.float32), np.zeros(64, np.float32), g[3]])
    index, dist, second = functional.gallery_match_normalised(x, g, c)        # top_n = 300 = M
    assert index.tolist() == [0, -1, -1, 3]
    assert np.isnan(dist[1:3]).all() and np.isnan(second[1:3]).all()
    assert dist[0] == second[0]                                        # the duplicate is the runner-up
    with pytest.raises(ValueError, match="gallery_match_normalised: top_n=300"):
        functional.gallery_match_normalised(x, g, c[:299])
    with pytest.raises(ValueError, match="cohort_stats: top_n=0"):
        functional.cohort_stats(x, c, 0)
    with pytest.raises(ValueError, match="gallery_match_normalised.*cohort of shape"):
        functional.gallery_match_normalised(x, g, _rows(10, 128, 0), 5)


# ------------------------------------------------------------------------------------------------- the signed threshold
def test_signed_threshold():
    assert check_delta_id(-2.5, "who", signed=True) == -2.5
    for bad in (float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="who: delta_id"):
            check_delta_id(bad, "who", signed=True)
    with pytest.raises(ValueError, match=">= 0"):
        check_delta_id(-2.5, "who")
    with pytest.raises(ValueError, match="SpeakerNames: delta_id=-1"):
        SpeakerNames(1, 4, -1)
    with pytest.raises(ValueError, match="SpeakerNames: delta_id=-1"):
        SpeakerNames(1, 4, -1, signed=False)


def test_speaker_names_follow_the_rule_below_zero():
    names = SpeakerNames(1, 4, -3.0, signed=True)
    assert names.delta_id == -3.0
    assign = np.array([[0, 1, 2]])
    names.update(assign, np.array([[5, 6, 7]]), np.array([[-2.9, -3.0, -8.0]], np.float32))
    assert names.best_e.tolist() == [[-1, 6, 7, -1]]                   # d <= delta_id: -2.9 is too far, -3.0 counts
    names.update(assign, np.array([[5, 9, 9]]), np.array([[-3.5, -3.0, -7.0]], np.float32))
    assert names.best_e.tolist() == [[5, 6, 7, -1]]                    # only a strictly closer match replaces
    assert names.best_d.tolist() == [[-3.5, -3.0, -8.0, np.inf]]
    names.update(assign, np.array([[7, -1, 7]]), np.array([[-9.0, np.nan, -8.0]], np.float32))
    assert names.holders().tolist() == [[7, 6, -1, -1]]                # two hold voiceprint 7: the closer keeps the name
    assert names.labels([f"v{e}" for e in range(10)]) == [{0: "v7", 1: "v6"}]


# ---------------------------------------------------------------------------------------------------- SpeakerGallery
def test_gallery_holds_and_round_trips_a_cohort(tmp_path):
    v, c = _rows(3, 64, 13), _rows(20, 64, 14)
    plain = SpeakerGallery(["a", "b", "c"], v)
    assert plain.cohort is None and plain.top_n == 300
    g = plain.with_cohort(c, top_n=5)
    assert g is not plain and plain.cohort is None
    assert g.names == plain.names and np.array_equal(g.voiceprints, v)
    assert g.cohort.dtype == np.float32 and np.array_equal(g.cohort, c) and g.top_n == 5
    assert g.device is None                                            # nothing has touched a GPU
    g.save(tmp_path / "g.npz")
    back = SpeakerGallery.load(tmp_path / "g.npz")
    assert back.names == g.names and np.array_equal(back.voiceprints, v)
    assert np.array_equal(back.cohort, c) and back.top_n == 5
    assert g.with_cohort(None).cohort is None
    same = SpeakerGallery(["a", "b", "c"], v, cohort=torch.from_numpy(c), top_n=20)
    assert np.array_equal(same.cohort, c) and same.top_n == 20


def test_gallery_without_a_cohort_keeps_the_file_format(tmp_path):
    v = _rows(2, 64, 15)
    SpeakerGallery(["a", "b"], v).save(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as z:
        assert sorted(z.files) == ["names", "voiceprints"]
    with open(tmp_path / "old.npz", "wb") as f:                        # a file of the two keys, as written so far
        np.savez(f, names=np.asarray(["a", "b"], dtype=np.str_), voiceprints=v)
    old = SpeakerGallery.load(tmp_path / "old.npz")
    assert old.names == ("a", "b") and np.array_equal(old.voiceprints, v) and old.cohort is None


def _bad_row(value):
    c = _rows(6, 64, 16)
    if value is None:
        c[4] = 0
    else:
        c[4, 9] = value
    return c


@pytest.mark.parametrize("cohort, top_n, word", [
    (_rows(5, 128, 0), 2, "(5, 128)"),
    (_rows(5, 64, 0)[0], 2, "(64,)"),
    (np.zeros((0, 64), np.float32), 1, "0 rows"),
    (np.ones((8193, 64), np.float32), 300, "8193 rows"),
    (_rows(5, 64, 0), 0, "top_n=0"),
    (_rows(5, 64, 0), 6, "top_n=6"),
    (_rows(5, 64, 0), 2.5, "top_n=2.5"),
    (_rows(299, 64, 0), 300, "top_n=300"),
    (_bad_row(np.nan), 2, "cohort row 4 is not finite"),
    (_bad_row(np.inf), 2, "cohort row 4 is not finite"),
    (_bad_row(None), 2, "cohort row 4 has zero norm"),
])
def test_gallery_refuses_a_bad_cohort(cohort, top_n, word):
    v = _rows(2, 64, 17)
    with pytest.raises(ValueError, match="SpeakerGallery") as err:
        SpeakerGallery(["a", "b"], v, cohort=cohort, top_n=top_n)
    assert word in str(err.value)
    with pytest.raises(ValueError, match="SpeakerGallery"):
        SpeakerGallery(["a", "b"], v).with_cohort(cohort, top_n)


@pytest.mark.parametrize("method", ["match_normalised", "cohort_stats", "entry_stats"])
def test_gallery_without_a_cohort_refuses_the_normalised_methods(method):
    g = SpeakerGallery(["a", "b"], _rows(2, 64, 18))
    args = () if method == "entry_stats" else (_rows(3, 64, 19),)
    with pytest.raises(ValueError, match=f"SpeakerGallery.{method}: the gallery has no cohort"):
        getattr(g, method)(*args)
    assert g.device is None


# ----------------------------------------------------------------------------------------------------- C entry points
def test_c_entry_points_refuse_bad_arguments_by_name():
    lib = _lib.load()
    rows, out = _rows(4, 64, 20), np.zeros(4, np.float32)
    p, o = rows.ctypes.data, out.ctypes.data

    def refused(rc, word):
        msg = lib.dz_last_error().decode()
        assert rc == 2 and msg.startswith(word), (rc, msg)

    refused(lib.dz_gallery_set_cohort(None, p, 4, 2), "dz_gallery_set_cohort: NULL handle")
    refused(lib.dz_gallery_cohort_stats(None, p, 64, 4, o, o, None), "dz_gallery_cohort_stats: NULL handle")
    refused(lib.dz_gallery_entry_stats(None, o, o), "dz_gallery_entry_stats: NULL handle")
    refused(lib.dz_gallery_match_norm(None, p, 64, 4, o, o, o, None), "dz_gallery_match_norm: NULL handle")
    assert lib.dz_gallery_cohort_size(None) == 0


# ------------------------------------------------------------------------------------------------------------ the tuner
def test_with_gallery_refuses_a_cohort_by_name():
    seg, emb = tc.random_outputs(3, 12, 32, 3, 64)
    cache = TuneCache.from_arrays([tc.file_of(seg, emb)], tc.config_of(0.5, 0.3, 1.0, 4, 2.5))
    v, c = _rows(3, 64, 21), _rows(10, 64, 22)
    with pytest.raises(ValueError, match="TuneCache.with_gallery: the gallery has a cohort"):
        cache.with_gallery(SpeakerGallery(["a", "b", "c"], v, cohort=c, top_n=3))
