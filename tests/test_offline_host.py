"""Whole-file diarization without a GPU: the float64 yardstick (tests/offline_ref.py) against scipy, and the host side
of the package -- backend="core" linkage (the kernels' text, csrc/agglo_core.h), the cut, the assignment and the
reconstruction (csrc/agglo.cpp), ``OfflineDiarization.from_cache`` -- against the yardstick.

Identical merges are demanded only of inputs whose margin (the smallest gap between a chosen merge and its runner-up,
by the yardstick alone) is at least 100 times the height tolerance 32 N 2^-52 / max(h, 1e-3); each test asserts that
its input is such an input."""
import numpy as np
import pytest

import offline_cases as cases
import offline_ref as ref
from diart_amd import functional
from diart_amd.offline import OfflineDiarization
from diart_amd.optim import TuneCache

# (N, D, clusters, noise, threshold), drawn in sequence from default_rng(0)
SETTINGS = [(40, 64, 4, 0.05, 0.7), (60, 64, 5, 0.08, 0.7), (48, 128, 3, 0.12, 0.9), (33, 64, 6, 0.03, 0.5),
            (50, 64, 4, 0.15, 0.6)]


@pytest.fixture(scope="module")
def generated():
    rng = np.random.default_rng(0)
    out = []
    for n, d, s, noise, threshold in SETTINGS:
        x = ref.clustered_rows(rng, n, d, s, noise)
        Z, gaps = ref.linkage(x)
        out.append((x, Z, gaps, threshold))
    return out


def same_partition(a, b):
    return np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])


def check_against_yardstick(Z, Z_ref, gaps):
    """Heights within the bound; pairs and sizes identical, the input's margin asserted first."""
    bound = ref.height_bound(Z_ref)
    assert Z.shape == Z_ref.shape and Z.dtype == np.float64
    print("margin / bound", (gaps / bound).min() if len(gaps) else np.inf, "height error / bound",
          (np.abs(Z[:, 2] - Z_ref[:, 2]) / bound).max() if len(gaps) else 0.0)
    assert (gaps >= 100 * bound).all(), "weak input: a merge of the yardstick is within 100 bounds of its runner-up"
    assert np.array_equal(Z[:, [0, 1, 3]], Z_ref[:, [0, 1, 3]])
    assert (np.abs(Z[:, 2] - Z_ref[:, 2]) <= bound).all()


def test_yardstick_equals_scipy(generated):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    for x, Z, gaps, threshold in generated:
        Zs = hierarchy.linkage(x, "centroid")
        assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
        assert np.abs(Z[:, 2] - Zs[:, 2]).max() < 1e-12
        assert np.abs(Z[:, 2] - threshold).min() > 1e-4
        assert same_partition(ref.flat_clusters(Z, x.shape[0], threshold), hierarchy.fcluster(Zs, threshold, "distance"))


def test_core_linkage_equals_yardstick(generated):
    for x, Z, gaps, threshold in generated:
        check_against_yardstick(functional.linkage_centroid(x), Z, gaps)
        labels, G = functional.cut_linkage(Z, threshold)
        assert (labels >= 0).all() and G == labels.max() + 1
        assert same_partition(labels, ref.flat_clusters(Z, x.shape[0], threshold))
    x = ref.clustered_rows(np.random.default_rng(7), 257, 64, 6, 0.1)
    Z, gaps = ref.linkage(x)
    import torch
    check_against_yardstick(functional.linkage_centroid(torch.from_numpy(x.astype(np.float64))), Z, gaps)
    assert ref.is_dendrogram(functional.linkage_centroid(x), 257)


def test_linkage_of_several_files_and_of_none():
    rng = np.random.default_rng(11)
    xs = [ref.clustered_rows(rng, n, 32, 3, 0.1) for n in (7, 1, 0, 30)]
    xs[2] = np.zeros((0, 32))
    Zs = functional.linkage_centroid(xs)
    assert [z.shape for z in Zs] == [(6, 4), (0, 4), (0, 4), (29, 4)]
    for x, Z in zip(xs, Zs):
        assert np.array_equal(Z, functional.linkage_centroid(x))
    # files that do not fit the budget together run in later groups, with the same result
    again = functional.linkage_centroid(xs, memory_budget=8 * 30 * 30)
    assert all(np.array_equal(a, b) for a, b in zip(Zs, again))
    labels, G = functional.cut_linkage(np.zeros((0, 4)), 0.5)
    assert labels.tolist() == [0] and G == 1
    labels, G = functional.cut_linkage(np.zeros((0, 4)), 0.5, n=0)
    assert labels.shape == (0,) and G == 0


def test_duplicates_merge_at_height_zero():
    x = ref.clustered_rows(np.random.default_rng(5), 20, 16, 2, 0.2)
    x[[4, 9, 15]] = x[2]
    Z = functional.linkage_centroid(x)
    assert ref.is_dendrogram(Z, 20) and np.array_equal(Z, functional.linkage_centroid(x))
    assert (Z[:3, 2] == 0).all() and Z[3, 2] > 0
    labels, _ = functional.cut_linkage(Z, 1e-9)
    assert len({labels[i] for i in (2, 4, 9, 15)}) == 1 and (np.bincount(labels) > 1).sum() == 1


# ------------------------------------------------------------------------------------------------------ the cut rules
def sized_file(sizes, on_frames=None, seed=2, noise=0.05):
    """One local speaker per chunk, chunk c's voice from group sizes[...]: every row usable, a row is a train row when its
    speaker is on in enough frames (on_frames per chunk, default: all)."""
    rng = np.random.default_rng(seed)
    which = np.concatenate([np.full(n, g) for g, n in enumerate(sizes)])
    rng.shuffle(which)
    C, F, D = which.shape[0], 20, 32
    centres = rng.standard_normal((len(sizes), D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    emb = (centres[which] + noise * rng.standard_normal((C, D)))[:, None, :].astype(np.float32)
    seg = np.full((C, F, 1), 0.1, dtype=np.float32)
    for c in range(C):
        seg[c, :F if on_frames is None else on_frames[c], 0] = 0.9
    return dict(uri="sized", seg=seg, emb=emb, starts=0.5 * np.arange(C), res=0.05, shift=0.0, reference=[]), which


def offline_vs_yardstick(f, threshold, min_cluster_size, max_speakers=20, min_clean_ratio=0.2):
    turns, info = ref.diarize(f["seg"], f["emb"], f["starts"], f["res"], f["shift"], threshold, cases.TAU, min_clean_ratio,
                              min_cluster_size, max_speakers)
    print("margins", info["merge_ratio"], info["threshold_gap"], info["assign_gap"])
    assert info["merge_ratio"] >= 100 and info["threshold_gap"] > 1e-6 and info["assign_gap"] > 1e-6, "weak input"
    od = OfflineDiarization(cases.config(max_speakers), threshold, min_cluster_size, min_clean_ratio, backend="core")
    cache = TuneCache.from_arrays([f], cases.config(max_speakers))
    (assign, G), = od.clusters(cache)
    assert G == info["G"] and np.array_equal(assign, info["assign"])
    ann, = od.from_cache(cache)
    assert sorted((s.start, s.end, l) for s, _, l in ann.itertracks(yield_label=True)) == turns
    return assign[:, 0], G, info


def test_small_clusters_dissolve_into_the_nearest_kept_one():
    f, which = sized_file((20, 14, 4, 3))
    assign, G, info = offline_vs_yardstick(f, 0.7, min_cluster_size=12)
    assert G == 2 and (assign >= 0).all()
    assert len(set(assign[which == 0])) == 1 and len(set(assign[which == 1])) == 1 and assign[which == 0][0] != assign[which == 1][0]
    assert len(np.unique(ref.flat_clusters(info["Z"], 41, 0.7))) == 4          # the cut itself found the four voices
    assign, G, _ = offline_vs_yardstick(f, 0.7, min_cluster_size=1)
    assert G == 4


def test_max_speakers_caps_the_kept_clusters_by_size():
    f, which = sized_file((9, 20, 14))
    assign, G, _ = offline_vs_yardstick(f, 0.7, min_cluster_size=2, max_speakers=2)
    assert G == 2 and len(set(assign[which == 1])) == 1 and len(set(assign[which == 2])) == 1
    assign, G, _ = offline_vs_yardstick(f, 0.7, min_cluster_size=2, max_speakers=1)
    assert G == 1 and (assign == 0).all()


def test_largest_cluster_is_kept_when_none_qualifies():
    f, which = sized_file((5, 8, 6))
    assign, G, _ = offline_vs_yardstick(f, 0.7, min_cluster_size=12)
    assert G == 1 and (assign == 0).all()


def test_no_train_row_and_one_train_row():
    f, _ = sized_file((6, 5), on_frames=[10] * 11)
    assign, G, info = offline_vs_yardstick(f, 0.7, min_cluster_size=12, min_clean_ratio=1.0)
    assert G == 1 and (assign == 0).all() and info["train"].shape[0] == 0
    f, _ = sized_file((6, 5), on_frames=[10] * 4 + [20] + [10] * 6)
    assign, G, info = offline_vs_yardstick(f, 0.7, min_cluster_size=12, min_clean_ratio=1.0)
    assert G == 1 and (assign == 0).all() and info["train"].shape[0] == 1
    f, _ = sized_file((6, 5), on_frames=[0] * 11)                  # nobody ever speaks: no usable row, no turn
    od = OfflineDiarization(cases.config(), 0.7, backend="core")
    cache = TuneCache.from_arrays([f], cases.config())
    assert od.clusters(cache)[0][1] == 0 and len(od.from_cache(cache)[0]) == 0
    assert ref.diarize(f["seg"], f["emb"], f["starts"], f["res"], f["shift"], 0.7, cases.TAU)[0] == []


# ---------------------------------------------------------------------------------------------------- reconstruction
def test_reconstruction_frame_for_frame():
    f = cases.crafted_file()
    turns, info = ref.diarize(f["seg"], f["emb"], f["starts"], f["res"], f["shift"], 0.7, cases.TAU)
    assert info["merge_ratio"] >= 100 and info["threshold_gap"] > 1e-6 and info["assign_gap"] > 1e-6, "weak input"
    # the corners are in the input
    assert info["G"] == 3 and (info["assign"][cases.NAN_CHUNK] == -1).all()
    twin = info["assign"][cases.TWIN_CHUNK]
    assert sorted(twin)[1:] == [twin.max()] * 2 and twin.max() >= 0                 # two local speakers, one cluster
    mean, A = info["mean"], info["A"]
    assert (mean - np.floor(mean) == 0.5).any()                                    # a mean count of exactly x.5
    top = -np.sort(-A, axis=1)
    tie = np.flatnonzero((top[:, 0] == top[:, 1]) & (top[:, 0] > 0))
    assert tie.size and (info["active"][tie].sum(axis=1) == 1).any()                # equal A, and only one of them on
    cache = TuneCache.from_arrays([f], cases.config())
    od = OfflineDiarization(cases.config(), 0.7, backend="core")
    active, = od.activity(cache)
    assert active.shape == info["active"].shape == (254, 3) and np.array_equal(active, info["active"])
    ann, = od.from_cache(cache)
    assert ann.uri == "crafted"
    assert sorted((s.start, s.end, l) for s, _, l in ann.itertracks(yield_label=True)) == turns and len(turns) >= 3
    # one dendrogram serves every threshold
    Z, = od.linkage(cache)
    assert np.array_equal(Z[:, [0, 1, 3]], info["Z"][:, [0, 1, 3]])
    assert functional.cut_linkage(Z, 0.7, 12, 20)[1] == 3 and functional.cut_linkage(Z, 5.0, 12, 20)[1] == 1


def test_two_files_are_each_their_own():
    a, b = cases.crafted_file(), cases.crafted_file(seed=9)
    b["uri"] = "second"
    od = OfflineDiarization(cases.config(), 0.7, backend="core")
    both = od.activity(TuneCache.from_arrays([a, b], cases.config()))
    for f, got in zip((a, b), both):
        assert np.array_equal(got, od.activity(TuneCache.from_arrays([f], cases.config()))[0])


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    cfg = cases.config()
    for bad in (float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="threshold"):
            OfflineDiarization(cfg, bad)
    with pytest.raises(ValueError, match="min_cluster_size"):
        OfflineDiarization(cfg, 0.7, min_cluster_size=0)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_clean_ratio"):
            OfflineDiarization(cfg, 0.7, min_clean_ratio=bad)
    with pytest.raises(ValueError, match="max_speakers"):
        OfflineDiarization(cases.config(max_speakers=0), 0.7)
    with pytest.raises(ValueError, match="backend"):
        OfflineDiarization(cfg, 0.7, backend="torch")
    x = ref.clustered_rows(np.random.default_rng(1), 12, 8, 2, 0.1)
    for value in (np.nan, np.inf):
        y = x.copy()
        y[3, 2] = value
        with pytest.raises(ValueError, match="not finite or has zero norm"):
            functional.linkage_centroid(y)
    y = x.copy()
    y[5] = 0
    with pytest.raises(ValueError, match="not finite or has zero norm"):
        functional.linkage_centroid(y)
    with pytest.raises(ValueError, match="dimension 1025"):
        functional.linkage_centroid(np.ones((3, 1025)))
    with pytest.raises(ValueError, match="memory_budget"):
        functional.linkage_centroid(x, memory_budget=8 * 12 * 12 - 1)
    f = cases.crafted_file()
    with pytest.raises(ValueError, match="memory_budget"):
        OfflineDiarization(cfg, 0.7, backend="core", memory_budget=1000).from_cache(TuneCache.from_arrays([f], cfg))
    Z = functional.linkage_centroid(x)
    with pytest.raises(ValueError, match="threshold"):
        functional.cut_linkage(Z, float("nan"))
    with pytest.raises(ValueError, match="min_cluster_size"):
        functional.cut_linkage(Z, 0.5, min_cluster_size=0)
    with pytest.raises(ValueError, match="max_speakers"):
        functional.cut_linkage(Z, 0.5, max_speakers=0)
    broken = Z.copy()
    broken[4, 0] = broken[3, 0]                                      # a node merged twice
    from diart_amd import _lib
    with pytest.raises(_lib.DiartAmdError, match="dendrogram"):
        functional.cut_linkage(broken, 0.5)


# ------------------------------------------------------------------------- the yardstick's own pieces, and the row rules
def test_fast_yardstick_equals_the_plain_one(generated):
    """tests/test_gpu_offline.py uses `linkage_fast` above 2 048 rows: the same Z and the same gaps, ties included."""
    for x, Z, gaps, _ in generated:
        Zf, gf = ref.linkage_fast(x)
        assert np.array_equal(Zf, Z) and np.array_equal(gf, gaps)
    x = ref.clustered_rows(np.random.default_rng(3), 300, 32, 5, 0.1)
    x[[7, 100, 250]] = x[1]
    (Z, gaps), (Zf, gf) = ref.linkage(x), ref.linkage_fast(x)
    assert np.array_equal(Zf, Z) and np.array_equal(gf, gaps) and (gaps[:2] == 0).all() and (Z[:3, 2] < 1e-12).all()


def test_row_rules_on_a_hand_made_file():
    """Which (chunk, local speaker) is usable and which is clustered, stated by hand: F = 10, min_clean_ratio = 0.25, so a
    train row needs ceil(2.5) = 3 clean frames."""
    F, K, D = 10, 2, 4
    seg = np.full((5, F, K), 0.1, dtype=np.float32)
    emb = np.tile(np.array([1.0, 2.0, 0.0, -1.0], dtype=np.float32), (5, K, 1))
    emb[:, 1] = [0.0, 1.0, 1.0, 3.0]
    seg[0, 0:5, 0] = 0.9        # chunk 0: k = 0 alone in frames 0, 1 only: usable, two clean frames, not clustered
    seg[0, 2:10, 1] = 0.9       #          k = 1 alone in frames 5 .. 9: clustered
    seg[1, 0:3, 0] = 0.9        # chunk 1: k = 0 alone in exactly 3 frames: clustered; k = 1 never on: not usable
    seg[2, 0, :] = 0.9          # chunk 2: both on in one frame, never alone: usable, not clustered
    seg[3, :, :] = 0.9          # chunk 3: both always on, but k = 0 has a zero embedding and k = 1 a NaN in it
    emb[3, 0] = 0.0
    emb[3, 1, 2] = np.nan
    seg[4, :, 0] = 0.9          # chunk 4: one NaN score makes the chunk invalid
    seg[4, 9, 1] = np.nan
    seg[1, 5, 0] = 0.5          # exactly tau_active is not on
    usable = np.array([[1, 1], [1, 0], [1, 1], [0, 0], [0, 0]], dtype=bool)
    train = [1, 2]              # indices into the usable rows in (c, k) order: (0, 1) and (1, 0)
    x, got_usable, got_train, on, valid = ref.rows_of(seg, emb, 0.5, 0.25)
    assert np.array_equal(got_usable, usable) and got_train.tolist() == train and valid.tolist() == [1, 1, 1, 1, 0]
    assert not on[1, 5, 0] and not on[4].any() and x.shape == (5, D) and np.allclose((x * x).sum(axis=1), 1.0)
    f = dict(uri="hand", seg=seg, emb=emb, starts=0.5 * np.arange(5), res=0.05, shift=0.0, reference=[])
    od = OfflineDiarization(cases.config(tau_active=0.5), 0.5, min_cluster_size=1, min_clean_ratio=0.25, backend="core")
    px, p_usable, p_train = od._rows(f)
    assert np.array_equal(p_usable, usable) and p_train.tolist() == train and np.array_equal(px, x)
    cache = TuneCache.from_arrays([f], cases.config())
    (assign, G), = od.clusters(cache)
    assert np.array_equal(assign >= 0, usable) and od.linkage(cache)[0].shape == (1, 4)
    assert OfflineDiarization(cases.config(tau_active=0.5), 0.5, min_clean_ratio=0.31, backend="core")._rows(f)[2].tolist() == [1]


# ------------------------------------------------------------------------------------------------------ command line
def test_command_line_from_a_stored_cache(tmp_path, capsys):
    """--cache FILE that exists: no model is loaded; one RTTM per file, and the error rate against --reference."""
    from diart_amd import offline
    from diart_amd.features import load_rttm
    files = [cases.crafted_file(), cases.crafted_file(seed=9)]
    files[1]["uri"] = "second"
    cache = TuneCache.from_arrays(files, cases.config())
    cache.save(tmp_path / "cache.npz")
    want = OfflineDiarization(cases.config(), 0.7, backend="core").from_cache(cache)
    refs, out = tmp_path / "refs", tmp_path / "out"
    refs.mkdir()
    for ann in want:
        (refs / f"{ann.uri}.rttm").write_text(ann.to_rttm())
    args = offline.parser().parse_args([str(tmp_path), "--output", str(out), "--threshold", "0.7", "--tau-active",
                                        str(cases.TAU), "--cache", str(tmp_path / "cache.npz"), "--reference", str(refs),
                                        "--backend", "core"])
    got = offline.run(args)
    assert [a.uri for a in got] == ["crafted", "second"]
    for ann in want:
        assert (out / f"{ann.uri}.rttm").read_text() == ann.to_rttm() and len(load_rttm(out / f"{ann.uri}.rttm")[ann.uri]) == len(ann)
    assert "[offline] 2 files, DER 0.00 %" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        offline.parser().parse_args([str(tmp_path), "--output", str(out)])            # --threshold has no default
