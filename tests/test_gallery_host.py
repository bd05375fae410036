"""The speaker gallery without a GPU: ``SpeakerGallery``'s refusals and its save / load round trip,
``functional.gallery_match`` on CPU input against the float64 statement, the C entry points' refusals, ``SpeakerNames``
against a plain-Python restatement, ``BatchedOutputTail.annotation(names=)`` and ``StreamServer.set_gallery`` on the
pipelines that have no speakers."""
import ctypes as C

import numpy as np
import pytest
import torch

from diart_amd import _lib, functional
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.gallery import SpeakerGallery, SpeakerNames


def _prints(E, D, seed=0):
    return np.random.default_rng(seed).standard_normal((E, D)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- SpeakerGallery
def test_gallery_holds_what_it_was_given():
    v = _prints(5, 192)
    g = SpeakerGallery(["ann", "ben", "cy", "di", "ed"], v)
    assert g.names == ("ann", "ben", "cy", "di", "ed") and g.dimension == 192 and len(g) == 5
    assert g.voiceprints.dtype == np.float32 and np.array_equal(g.voiceprints, v)
    assert g.device is None                                   # nothing has touched a GPU


@pytest.mark.parametrize("names, rows, word", [
    (["a", "b", "a"], _prints(3, 64), "duplicate name 'a'"),
    (["a", "speaker12"], _prints(2, 64), "speaker12"),
    (["a", "b"], _prints(3, 64), "2 names for 3"),
    (["a", ""], _prints(2, 64), "non-empty"),
    (["a"], _prints(1, 100), "dimension 100"),
    (["a"], _prints(1, 32), "dimension 32"),
    (["a"], _prints(1, 576), "dimension 576"),
    ([], np.zeros((0, 64), np.float32), "0 voiceprints"),
    (["a"], np.zeros(64, np.float32), "shape (64,)"),
])
def test_gallery_refusals(names, rows, word):
    with pytest.raises(ValueError, match="SpeakerGallery") as err:
        SpeakerGallery(names, rows)
    assert word in str(err.value)


def test_gallery_refuses_too_many_voiceprints():
    with pytest.raises(ValueError, match="65537 voiceprints"):
        SpeakerGallery([str(i) for i in range(65537)], np.ones((65537, 64), np.float32))


@pytest.mark.parametrize("bad, word", [(np.nan, "not finite"), (np.inf, "not finite"), (None, "zero norm")])
def test_gallery_refuses_unusable_voiceprints(bad, word):
    v = _prints(4, 64)
    if bad is None:
        v[2] = 0
    else:
        v[2, 17] = bad
    with pytest.raises(ValueError, match=word) as err:
        SpeakerGallery(["a", "b", "c", "d"], v)
    assert "'c'" in str(err.value)


def test_gallery_accepts_names_that_only_contain_the_reserved_form():
    SpeakerGallery(["speaker", "speaker1a", "my speaker3"], _prints(3, 64))


def test_gallery_save_load_round_trip(tmp_path):
    v = _prints(7, 256, seed=3) * 3.5                          # not normalised: the rows come back as given
    names = [f"person {i} é" for i in range(7)]
    path = tmp_path / "gallery.npz"
    SpeakerGallery(names, v).save(path)
    back = SpeakerGallery.load(path)
    assert back.names == tuple(names) and back.voiceprints.dtype == np.float32
    assert back.voiceprints.tobytes() == v.tobytes()
    with np.load(path, allow_pickle=False) as z:               # an .npz of names and float32 rows, nothing pickled
        assert sorted(z.files) == ["names", "voiceprints"]


def test_enrol_windows_with_a_callable_model():
    """The windowing of ``enrol`` with a stand-in model on the CPU: consecutive windows, the remainder dropped, short
    audio as one row of its own length, the model called without weights; a non-finite embedding names the speaker."""
    calls = []

    def model(rows):
        calls.append(tuple(rows.shape))
        return rows[:, 0, :64] * rows[:, 0, 3:67] + 0.5

    rng = np.random.default_rng(9)
    audio = {"ann": rng.standard_normal(250).astype(np.float32), "ben": torch.from_numpy(rng.standard_normal((1, 70))).float()}
    g = SpeakerGallery.enrol(model, audio, sample_rate=100, duration=1.0)
    assert calls == [(2, 1, 100), (1, 1, 70)] and g.names == ("ann", "ben") and g.dimension == 64
    for row, wave, n in ((g.voiceprints[0], audio["ann"], 2), (g.voiceprints[1], audio["ben"].numpy()[0], 1)):
        w = torch.from_numpy(np.asarray(wave)).double()
        rows = w[:200].reshape(2, 100) if n == 2 else w.reshape(1, 70)
        emb = rows[:, :64] * rows[:, 3:67] + 0.5
        mean = (emb / emb.norm(dim=1, keepdim=True)).mean(dim=0)
        assert np.abs(row - (mean / mean.norm()).numpy()).max() <= 1e-6
    bad = audio["ann"].copy()
    bad[120] = np.nan
    with pytest.raises(ValueError, match="'eve' is not finite"):
        SpeakerGallery.enrol(model, {"ann": audio["ann"], "eve": bad}, sample_rate=100, duration=1.0)
    with pytest.raises(ValueError, match="'nobody'"):
        SpeakerGallery.enrol(model, {"nobody": np.zeros(0, np.float32)}, sample_rate=100)


# ------------------------------------------------------------------------------------- functional.gallery_match (CPU)
def _statement(x, g):
    x, g = torch.as_tensor(x).double(), torch.as_tensor(g).double()
    d = 1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None])
    return d, d.argmin(dim=1)


ULP = 2.0 ** -23      # one float32 step below 2: two evaluations of a float64 product may round a float32 apart by it


@pytest.mark.parametrize("E", [1, 2, 37])
def test_functional_gallery_match_on_cpu_is_the_float64_statement(E):
    torch.manual_seed(E)
    x, g = torch.randn(29, 64), torch.randn(E, 64) * 2
    if E > 2:
        g[E - 1] = g[0]                                        # a duplicate: best and second (nearly) equal there
    d, best = _statement(x, g)
    index, dist, second = functional.gallery_match(x, g)
    assert index.dtype == torch.int32 and dist.dtype == second.dtype == torch.float32 and index.shape == (29,)
    top = torch.sort(d, dim=1).values
    # the index is the statement's argmin; where the two smallest distances are a rounding apart (the duplicate: a
    # float64 BLAS may give equal columns unequal last bits) either of the two is the statement's answer
    clear = torch.ones(29, dtype=torch.bool) if E == 1 else (top[:, 1] - top[:, 0]) > 1e-12
    assert clear.sum() >= 20 and torch.equal(index.long()[clear], best[clear])
    assert (d[torch.arange(29), index.long()] - top[:, 0]).abs().max() <= 1e-12
    assert (dist.double() - top[:, 0]).abs().max() <= ULP
    if E == 1:
        assert torch.isinf(second).all() and (second > 0).all()
    else:
        assert (second.double() - top[:, 1]).abs().max() <= ULP and (second >= dist).all()


def test_functional_gallery_match_unusable_rows_and_numpy():
    rng = np.random.default_rng(5)
    x, g = rng.standard_normal((6, 128)).astype(np.float32), rng.standard_normal((9, 128)).astype(np.float32)
    x[1, 3], x[2, 100], x[4] = np.nan, -np.inf, 0.0
    index, dist, second = functional.gallery_match(x.reshape(2, 3, 128), g)
    assert isinstance(index, np.ndarray) and index.shape == dist.shape == second.shape == (2, 3)
    index, dist, second = index.reshape(-1), dist.reshape(-1), second.reshape(-1)
    bad = np.array([False, True, True, False, True, False])
    assert (index[bad] == -1).all() and np.isnan(dist[bad]).all() and np.isnan(second[bad]).all()
    d, best = _statement(x[~bad], g)
    assert np.array_equal(index[~bad], best.numpy())
    assert np.abs(dist[~bad].astype(np.float64) - d.min(dim=1).values.numpy()).max() <= ULP
    assert np.isfinite(second[~bad]).all() and (second[~bad] >= dist[~bad]).all()
    with pytest.raises(ValueError, match="gallery_match"):
        functional.gallery_match(x[:, :64], g)


# --------------------------------------------------------------------------------------------------- the C entry points
def test_c_entry_points_refuse_bad_arguments_by_name():
    lib = _lib.load()
    h = _lib.vp()
    rows = np.ones((4, 64), np.float32)

    def create(ptr, E, D, out=C.byref(h)):
        rc = lib.dz_gallery_create(None, ptr, E, D, out)
        return rc, lib.dz_last_error().decode()

    for args, word in [((None, 4, 64), "NULL argument"), ((rows.ctypes.data, 0, 64), "0 voiceprints"),
                       ((rows.ctypes.data, 65537, 64), "65537 voiceprints"), ((rows.ctypes.data, 4, 96), "dimension 96"),
                       ((rows.ctypes.data, 4, 0), "dimension 0"), ((rows.ctypes.data, 1, 576), "dimension 576"),
                       ((rows.ctypes.data, 4, 64), "NULL context")]:
        rc, msg = create(*args)
        assert rc == 2 and msg.startswith("dz_gallery_create:") and word in msg, (args, rc, msg)
    rc, msg = create(rows.ctypes.data, 4, 64, None)
    assert rc == 2 and "dz_gallery_create: NULL argument" in msg
    bad = rows.copy()
    bad[2, 5] = np.inf
    rc, msg = create(bad.ctypes.data, 4, 64)
    assert rc == 2 and "dz_gallery_create: voiceprint 2 is not finite" in msg
    bad[2] = 0
    rc, msg = create(bad.ctypes.data, 4, 64)
    assert rc == 2 and "dz_gallery_create: voiceprint 2 is of zero norm" in msg
    assert not h.value                                         # no handle came back
    out = np.zeros(4, np.float32)
    rc = lib.dz_gallery_match(None, rows.ctypes.data, 64, 4, out.ctypes.data, out.ctypes.data, out.ctypes.data, None)
    assert rc == 2 and "dz_gallery_match: NULL handle" in lib.dz_last_error().decode()
    assert lib.dz_gallery_size(None) == 0 and lib.dz_gallery_dim(None) == 0 and lib.dz_gallery_destroy(None) == 0


# -------------------------------------------------------------------------------------------------------- SpeakerNames
class PlainNames:
    """The rule of ``SpeakerNames`` in plain Python, one stream at a time."""

    def __init__(self, n, G, delta):
        self.n, self.G, self.delta = n, G, delta
        self.reset()

    def reset(self, slot=None):
        if slot is None:
            self.best = {s: {} for s in range(self.n)}        # stream -> g -> (d, e)
        else:
            self.best[slot] = {}

    def update(self, assign, index, distance, slots):
        for row, s in enumerate(slots):
            for k in range(assign.shape[1]):
                g, e, d = int(assign[row, k]), int(index[row, k]), float(distance[row, k])
                if g >= 0 and e >= 0 and d <= self.delta and d < self.best[s].get(g, (float("inf"), -1))[0]:
                    self.best[s][g] = (d, e)

    def labels(self, names, slots):
        out = []
        for s in slots:
            winner = {}                                       # e -> (d, g) of the holder that keeps the name
            for g, (d, e) in sorted(self.best[s].items()):
                if e not in winner or (d, g) < winner[e]:
                    winner[e] = (d, g)
            out.append({g: names[e] for e, (d, g) in winner.items()})
        return out


def _random_step(rng, n, K, G, E, delta):
    rows = sorted(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist())
    assign = np.stack([rng.permutation(G)[:K] for _ in rows]).astype(np.int32)
    assign[rng.random(assign.shape) < 0.2] = -1
    index = rng.integers(0, E, size=assign.shape).astype(np.int32)
    index[rng.random(assign.shape) < 0.1] = -1
    # a coarse grid of distances: equal best_d (the tie), d == delta_id exactly, d just above it, NaN
    grid = np.array([0.0, 0.125, 0.25, delta, np.nextafter(np.float32(delta), np.float32(2)), 0.75, np.nan], np.float32)
    distance = grid[rng.integers(0, len(grid), size=assign.shape)]
    return rows, assign, index, distance


@pytest.mark.parametrize("seed", range(6))
def test_speaker_names_equals_the_plain_restatement(seed):
    rng = np.random.default_rng(seed)
    n, K, G, E, delta = 5, 3, 6, 4, 0.5                        # few voiceprints: several g hold the same one
    names = [f"n{e}" for e in range(E)]
    fast, plain = SpeakerNames(n, G, delta), PlainNames(n, G, delta)
    conflicts = ties = 0
    for t in range(60):
        if t == 20:
            fast.reset(2), plain.reset(2)
        if t == 40:                                           # a change of gallery: everything is forgotten
            fast.reset(), plain.reset()
        rows, assign, index, distance = _random_step(rng, n, K, G, E, delta)
        fast.update(assign, index, distance, rows)
        plain.update(assign, index, distance, rows)
        got = fast.labels(names, rows)
        assert got == plain.labels(names, rows), (seed, t)
        everyone = range(n)
        assert fast.labels(names) == plain.labels(names, everyone)
        for s in everyone:
            held = [e for _, e in plain.best[s].values()]
            conflicts += len(held) != len(set(held))
            ds = [d for d, e in plain.best[s].values() if held.count(e) > 1]
            ties += len(ds) != len(set(ds))
        for s, lab in zip(rows, got):
            assert len(set(lab.values())) == len(lab)         # a name is carried by one speaker at a time
    assert conflicts > 0 and ties > 0, "the sequences never reached the conflict / the tie on best_d"


def test_speaker_names_cases_one_by_one():
    names = ["ann", "ben"]
    sn = SpeakerNames(2, 4, 0.5)
    a = lambda *v: np.array([v], np.int32)
    f = lambda *v: np.array([v], np.float32)
    sn.update(a(0, 1, -1), a(0, 1, 1), f(0.5, 0.5000001, 0.1), [1])       # d == delta_id: accepted; above / unassigned: not
    assert sn.labels(names, [1]) == [{0: "ann"}] and sn.labels(names, [0]) == [{}]
    sn.update(a(2, 3, 1), a(0, 0, 1), f(0.25, 0.25, 0.4), [1])            # conflict on ann: 2 and 3 tie below 0 -> lowest g
    assert sn.labels(names, [1]) == [{2: "ann", 1: "ben"}]
    assert sn.best_e[1].tolist() == [0, 1, 0, 0]                          # the losers keep their state
    sn.update(a(3, 0, 1), a(0, -1, 0), f(0.2, 0.0, np.nan), [1])          # 3 comes closer; index -1 and NaN change nothing
    assert sn.labels(names, [1]) == [{3: "ann", 1: "ben"}]
    sn.update(a(3, 0, 1), a(1, 1, 1), f(0.3, 0.6, 0.45), [1])             # a farther match never replaces a closer one
    assert sn.labels(names, [1]) == [{3: "ann", 1: "ben"}]
    sn.reset(1)
    assert sn.labels(names) == [{}, {}]
    for bad in (None, float("nan"), float("inf"), -0.1, "x"):
        with pytest.raises(ValueError, match="delta_id"):
            SpeakerNames(2, 4, bad)


# ------------------------------------------------------------------------------------------------ annotation(names=)
def test_annotation_names():
    turns = np.array([[0.0, 1.0, 0], [0.5, 2.0, 3], [2.5, 3.0, 0], [9, 9, 9]], np.float64)
    plain = BatchedOutputTail.annotation(turns, 3)
    assert [lab for _, _, lab in plain.itertracks(yield_label=True)] == ["speaker0", "speaker3", "speaker0"]
    for names in (None, {}):
        assert BatchedOutputTail.annotation(turns, 3, names=names).to_rttm() == plain.to_rttm()
    named = BatchedOutputTail.annotation(turns, 3, uri="u", names={3: "ann", 7: "nobody here"})
    assert [(s.start, s.end, t, lab) for s, t, lab in named.itertracks(yield_label=True)] == \
        [(0.0, 1.0, 0, "speaker0"), (0.5, 2.0, 3, "ann"), (2.5, 3.0, 0, "speaker0")]
    # one label for every turn (VAD / OSD) is not a speaker: names do not apply
    vad = BatchedOutputTail.annotation(turns, 3, label="speech", names={0: "ann"})
    assert set(vad.labels()) == {"speech"}


# ------------------------------------------------------------------------------------------- StreamServer.set_gallery
@pytest.mark.parametrize("pipeline", ["vad", "osd"])
def test_server_set_gallery_is_refused_where_there_are_no_speakers(pipeline):
    from diart_amd.serve import StreamServer
    srv = StreamServer.__new__(StreamServer)                  # no engine, no device: the refusal comes first
    srv.pipeline = pipeline
    gallery = SpeakerGallery(["ann"], _prints(1, 64))
    with pytest.raises(ValueError, match=f"pipeline='{pipeline}'") as err:
        srv.set_gallery(gallery, 0.5)
    assert "StreamServer.set_gallery" in str(err.value)
