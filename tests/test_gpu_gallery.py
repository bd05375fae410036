"""The speaker gallery on the GPU.  The yardstick of the kernel is one torch statement on float64 CPU tensors,

    d = 1 - (x @ g.T) / (x.norm(dim=1, keepdim=True) * g.norm(dim=1)[None]);   best = d.argmin(dim=1)

and each distance of ``gallery_match`` must be within (D + 8) 2^-24 of it: the a-priori bound of an f32 chain of D
products of unit vectors plus the roundings of the normalisations, derived and not measured (DESIGN.md 4.18 has the
measured maxima beside it).  The engines and the server are checked against what they compute without a gallery (bit
for bit), against ``SpeakerGallery.match`` on the same embeddings and against the plain-Python restatement of
``SpeakerNames`` in ``test_gallery_host.py``.  Synthetic weights and audio throughout."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import _lib, functional
from diart_amd import models as M
from diart_amd.blocks.aggregation import BatchedOutputTail
from diart_amd.gallery import SpeakerGallery
from diart_amd.pipeline import GroupsBatch, StreamBatch
from diart_amd.synth import (synth_ecapa_state, synth_embedding_state, synth_segmentation_state, synth_stream,
                             synth_streams)

pytestmark = pytest.mark.gpu

R = 193
W, HOP = 80000, 8000
DELTA = 0.3           # the tests' identification threshold (a parameter of the test, not a recommendation)


def bound(D):
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


_cases = {}


def case(D, E):
    """Inputs and float64 reference of one shape, computed once: x (R, D), g (E, D) standard normal."""
    if (D, E) not in _cases:
        torch.manual_seed(1000 * D + E)
        x, g = torch.randn(R, D), torch.randn(E, D)
        xd, gd = x.double(), g.double()
        d = 1 - (xd @ gd.T) / (xd.norm(dim=1, keepdim=True) * gd.norm(dim=1)[None])
        _cases[(D, E)] = (x, g, d, d.argmin(dim=1))
    return _cases[(D, E)]


# ------------------------------------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("E", [1, 2, 33, 257, 4099])
@pytest.mark.parametrize("D", [192, 256, 512])
def test_kernel_against_float64(gpu, D, E):
    x, g, d, best = case(D, E)
    gallery = SpeakerGallery(names_of(E), g, gpu)
    index, dist, second = (t.cpu() for t in gallery.match(strided(x.to(gpu), gpu)))
    assert index.dtype == torch.int32 and index.shape == dist.shape == second.shape == (R,)
    assert (index >= 0).all() and (index < E).all()
    rows = torch.arange(R)
    err = (dist.double() - d[rows, index.long()]).abs().max().item()         # the distance of the voiceprint it names
    print(f"gallery_match D={D} E={E}: max |distance - float64| = {err:.3e} = {err * 2 ** 24:.2f} x 2^-24 "
          f"(bound {D + 8})")
    assert err <= bound(D)
    top = torch.sort(d, dim=1).values
    assert (dist.double() - top[:, 0]).abs().max().item() <= bound(D)
    if E == 1:
        assert torch.isinf(second).all() and (second > 0).all()
        clear = torch.ones(R, dtype=torch.bool)
    else:
        assert (second.double() - top[:, 1]).abs().max().item() <= bound(D)
        assert (second >= dist).all()
        clear = (top[:, 1] - top[:, 0]) > 2 * bound(D)
    left_out = int((~clear).sum())
    print(f"  rows whose float64 best and second are within twice the bound: {left_out} of {R}")
    assert left_out <= 0.03 * R
    assert torch.equal(index.long()[clear], best[clear])


def test_functional_gallery_match_runs_the_kernel(gpu):
    x, g, d, best = case(192, 33)
    index, dist, second = functional.gallery_match(x.to(gpu).reshape(1, R, 192), g.to(gpu))
    assert index.is_cuda and index.shape == (1, R) and index.dtype == torch.int32
    want = SpeakerGallery(names_of(33), g, gpu).match(x.to(gpu))
    for a, b in zip((index, dist, second), want):
        assert torch.equal(bits(a.reshape(-1)), bits(b))
    cpu = functional.gallery_match(x, g)                       # the statement itself, for comparison
    assert (dist.cpu().reshape(-1) - cpu[1]).abs().max().item() <= bound(192)


# ------------------------------------------------------------------------------------------------------ planted matches
def test_planted_matches_in_the_largest_gallery(gpu):
    E, D = 65536, 256
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(E, D, generator=gen)
    planted = torch.randperm(E, generator=gen)[:R]
    planted[0], planted[1] = 0, E - 1                           # the two ends of the gallery
    x = g[planted] + 1e-3 * torch.randn(R, D, generator=gen)
    gallery = SpeakerGallery(names_of(E), g, gpu)
    index, dist, second = (t.cpu() for t in gallery.match(x.to(gpu)))
    assert torch.equal(index.long(), planted)
    assert (dist.abs() < 1e-5).all() and (second > 0.5).all()


# ---------------------------------------------------------------------------------------------- ties and unusable rows
def test_ties_go_to_the_lowest_index_with_equal_bits(gpu):
    x, g, _, _ = case(256, 4099)
    g = g.clone()
    g[4000] = g[5]
    x = x.clone()
    x[:50] = 3.0 * g[5] + 0.05 * x[:50]                        # 50 rows whose nearest voiceprint is the duplicated one
    index, dist, second = (t.cpu() for t in SpeakerGallery(names_of(4099), g, gpu).match(x.to(gpu)))
    assert (index[:50] == 5).all()
    assert torch.equal(bits(dist[:50]), bits(second[:50]))      # the runner-up is the duplicate at 4000: the same bits
    assert (index[50:] != 4000).all()
    assert (second[50:] > dist[50:]).all()


def test_unusable_rows_get_minus_one_and_touch_nobody(gpu):
    x, g, _, _ = case(192, 257)
    gallery = SpeakerGallery(names_of(257), g, gpu)
    alone = [tuple(t.cpu() for t in gallery.match(x[r:r + 1].to(gpu))) for r in range(8)]
    y = x[:8].clone()
    y[1, 100], y[2, 0], y[4], y[6, 191] = float("nan"), float("inf"), 0.0, float("-inf")
    bad = torch.tensor([False, True, True, False, True, False, True, False])
    index, dist, second = (t.cpu() for t in gallery.match(y.to(gpu)))
    assert (index[bad] == -1).all() and torch.isnan(dist[bad]).all() and torch.isnan(second[bad]).all()
    for r in torch.nonzero(~bad)[:, 0].tolist():
        for got, want in zip((index, dist, second), alone[r]):
            assert torch.equal(bits(got[r:r + 1]), bits(want)), r
    huge = torch.full((1, 192), 3e38)                           # finite elements, a norm beyond float32
    assert gallery.match(huge.to(gpu))[0].item() == -1


# --------------------------------------------------------------------------------------------------------- independence
def test_distance_bits_do_not_depend_on_the_batch_the_gallery_order_or_the_alignment(gpu):
    D, E = 256, 4099
    x, g, _, _ = case(D, E)
    gallery = SpeakerGallery(names_of(E), g, gpu)
    dx = x.to(gpu)
    index, dist, second = gallery.match(dx)
    # one row alone
    for r in (0, 77, 192):
        for a, b in zip(gallery.match(dx[r:r + 1]), (index, dist, second)):
            assert torch.equal(bits(a), bits(b[r:r + 1])), r
    # a permuted gallery, and a shorter one that ends inside a tile
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(3))
    pi, pd, ps = SpeakerGallery(names_of(E), g[perm], gpu).match(dx)
    assert torch.equal(bits(pd), bits(dist)) and torch.equal(bits(ps), bits(second))
    unique = (second > dist).cpu()
    assert unique.sum() >= R - 2
    assert torch.equal(perm[pi.cpu().long()][unique], index.cpu().long()[unique])
    keep = 1000
    hi, hd, _ = SpeakerGallery(names_of(keep), g[:keep], gpu).match(dx)
    inside = (index < keep).cpu()
    assert inside.any() and torch.equal(bits(hd)[inside], bits(dist)[inside])
    assert torch.equal(hi.cpu()[inside], index.cpu()[inside])
    # row bases 4 and 8 bytes off a 16-byte boundary, and an odd stride (every alignment in one batch)
    for pad, offset in ((4, 1), (4, 2), (1, 0), (3, 3)):
        view = strided(dx, gpu, pad, offset)
        assert pad % 4 or view.data_ptr() % 16 == 4 * offset
        for a, b in zip(gallery.match(view), (index, dist, second)):
            assert torch.equal(bits(a), bits(b)), (pad, offset)


def test_match_refusals_name_the_function(gpu):
    x, g, _, _ = case(192, 33)
    gallery = SpeakerGallery(names_of(33), g, gpu)
    gallery.match(x.to(gpu))
    lib, h = _lib.load(), gallery._handle.h
    assert lib.dz_gallery_size(h) == 33 and lib.dz_gallery_dim(h) == 192
    rows = torch.zeros(4, 192, device=gpu)
    out = torch.zeros(3, 4, dtype=torch.int32, device=gpu)
    o = [out[i].data_ptr() for i in range(3)]
    for args, word in [((rows.data_ptr(), 192, 0, *o), "0 rows"), ((rows.data_ptr(), 192, 4097, *o), "4097 rows"),
                       ((rows.data_ptr(), 191, 4, *o), "row stride 191 below the dimension 192"),
                       ((None, 192, 4, *o), "NULL rows or output"), ((rows.data_ptr(), 192, 4, o[0], None, o[2]), "NULL")]:
        rc = lib.dz_gallery_match(h, *args, None)
        assert rc == 2 and lib.dz_last_error().decode().startswith("dz_gallery_match:") \
            and word in lib.dz_last_error().decode(), args
    with pytest.raises(ValueError, match="dimension"):
        gallery.match(torch.zeros(4, 256, device=gpu))


# --------------------------------------------------------------------------------------------------------------- engines
def _plain_names():
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_gallery_host import PlainNames
    return PlainNames


def _make_engine(kind, gpu):
    if kind == "xvector":
        n = 4
        return n, StreamBatch(M.HipSegmentation(synth_segmentation_state(), max_batch=n),
                              M.HipEmbedding(synth_embedding_state(), max_batch=n), n, device=gpu, tail=True)
    n = 2
    pipe = StreamBatch(M.HipSegmentation(synth_segmentation_state(seed=77, powerset=True), max_batch=n, powerset=True),
                       M.HipEcapaEmbedding(synth_ecapa_state()), n, tau_active=0.5, normalize_embedding_weights=True,
                       device=gpu, tail=True)
    assert isinstance(pipe, GroupsBatch)
    return n, pipe


def _run(pipe, d_audio, steps):
    """-> per step (seg, emb, assign, turns per stream, ticket's match, ticket's names), copies."""
    out = []
    for t in range(steps):
        ticket = pipe.launch(d_audio[:, t * HOP:t * HOP + W])
        seg, emb, _, assign = pipe.finish(ticket, want_scores=False)
        _, _, _, _, turns, nturns = ticket["tail"]
        match = tuple(m.copy() for m in ticket["match"]) if "match" in ticket else None
        out.append((seg.copy(), emb.copy(), assign.copy(), [turns[i, :int(nturns[i])].copy() for i in range(pipe.n)],
                    match, ticket.get("names")))
    return out


def _same_steps(a, b):
    for t, (p, q) in enumerate(zip(a, b)):
        for j in range(3):                                     # seg, emb, assign: bit for bit (NaN rows included)
            assert p[j].tobytes() == q[j].tobytes(), (t, j)
        for u, v in zip(p[3], q[3]):
            assert u.tobytes() == v.tobytes(), t


def _plant(first, n, D, seed):
    """A gallery of one assigned, finite embedding per stream (from step 2 or the first later step that has one, so
    the name arrives mid-stream) + 500 random distractors -> (names, rows, {stream: (step, g)})."""
    names, rows, where = [], [], {}
    for i in range(n):
        for t in list(range(2, len(first))) + [1, 0]:
            _, emb, assign, _, _, _ = first[t]
            ks = [k for k in range(assign.shape[1]) if assign[i, k] >= 0 and np.isfinite(emb[i, k]).all()]
            if ks:
                names.append(f"plant{i}")
                rows.append(emb[i, ks[0]].copy())
                where[i] = (t, int(assign[i, ks[0]]))
                break
    assert len(where) >= 1, "no stream had an assigned speaker: the synthetic audio changed"
    noise = np.random.default_rng(seed).standard_normal((500, D)).astype(np.float32)
    return names + [f"distractor{j}" for j in range(500)], np.concatenate([np.stack(rows), noise]), where


@pytest.mark.parametrize("kind", ["xvector", "ecapa"])
def test_engine_names_planted_speakers(gpu, kind):
    steps = 8
    n, pipe = _make_engine(kind, gpu)
    D = pipe.emb.dimension
    d_audio = torch.from_numpy(synth_streams(n, (W + HOP * steps) / 16000.0, seed0=300 if kind == "xvector" else 950)).to(gpu)
    first = _run(pipe, d_audio, steps)
    assert all(s[4] is None and s[5] is None for s in first)
    names, rows, where = _plant(first, n, D, seed=11)
    gallery = SpeakerGallery(names, rows, gpu)

    # refusals by name, before anything changes
    with pytest.raises(ValueError, match="set_gallery.*dimension"):
        pipe.set_gallery(SpeakerGallery(["a"], np.ones((1, 64), np.float32)), DELTA)
    with pytest.raises(ValueError, match="set_gallery.*delta_id"):
        pipe.set_gallery(gallery)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="set_gallery.*is on"):
            pipe.set_gallery(SpeakerGallery(names, rows, torch.device("cuda", 1)), DELTA)
    assert pipe._gallery is None

    pipe.set_gallery(gallery, DELTA)
    pipe.reset()
    second = _run(pipe, d_audio, steps)
    _same_steps(first, second)
    plain = _plain_names()(n, pipe.max_speakers, DELTA)
    for t, (seg, emb, assign, turns, match, got_names) in enumerate(second):
        want = gallery.match(emb)
        for a, b in zip(match, want):
            assert a.shape == (n, emb.shape[1]) and bits(a).equal(bits(b)), t
        plain.update(assign, match[0], match[1], range(n))
        assert got_names == plain.labels(gallery.names, range(n)), t
        for i, (t0, g) in where.items():
            if t >= t0:
                assert got_names[i].get(g) == f"plant{i}", (t, i)      # named from the step its embedding occurs in
            if t == t0:
                k = int(np.nonzero(assign[i] == g)[0][0])
                assert names[match[0][i, k]] == f"plant{i}" and abs(match[1][i, k]) < 1e-5

    # diarize(): the Annotations carry the names
    pipe.reset()
    for t in range(steps):
        anns = pipe.diarize(d_audio[:, t * HOP:t * HOP + W])
        _, _, _, turns, _, step_names = second[t]
        for i, ann in enumerate(anns):
            want = BatchedOutputTail.annotation(turns[i], len(turns[i]), names=step_names[i])
            assert ann.to_rttm() == want.to_rttm(), (t, i)
            for _, track, lab in ann.itertracks(yield_label=True):
                assert lab == step_names[i].get(track, f"speaker{track}")

    # a gallery of another size replaces it and forgets every name; None gives the first pass again
    pipe.set_gallery(SpeakerGallery(names[:3], rows[:3], gpu), DELTA)
    assert (pipe._names.best_e == -1).all()
    pipe.set_gallery(None)
    pipe.reset()
    third = _run(pipe, d_audio, steps)
    _same_steps(first, third)
    assert all(s[4] is None and s[5] is None for s in third)


# ---------------------------------------------------------------------------------------------------------------- server
def _serve(gpu, states, audio, gallery):
    """ann and ben from tick 0, ben leaves after tick 17 and "late" takes over his slot with ben's audio again.  Every
    step of the engine is logged (slots, emb, assign, match) and restated: -> (per tick {stream: [(start, end, g,
    label)]} as the step returned it (the server keeps adding to a stream's first Annotation), the restated labels per
    tick {stream: {g: name}}, close() per stream, the log)."""
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = states
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=3), M.HipEmbedding(emb_sd, max_batch=3), max_streams=3,
                       device=gpu)
    assert srv.rings is not None
    if gallery is not None:
        srv.set_gallery(gallery, DELTA)
    log, finish = [], srv.batch.finish

    def logged(ticket, want_scores=True):
        res = finish(ticket, want_scores)
        if not srv.batch._warming:
            log.append((list(ticket["slots"]), res[1].copy(), res[3].copy(),
                        tuple(m.copy() for m in ticket["match"]) if gallery is not None else None))
        return res

    srv.batch.finish = logged
    plain = _plain_names()(3, srv.batch.max_speakers, DELTA)
    joined = {"ann": 0, "ben": 0, "late": 18}
    ticks, restated, closed = [], [], {}
    for tick in range(18 + 18):
        for k, t0 in joined.items():
            if tick == t0:
                srv.open(k)
                plain.reset(srv._streams[k].slot)              # a joining stream starts with no names
            lo = (tick - t0) * HOP
            if k in srv.open_streams and 0 <= lo < len(audio[k]):
                srv.push(k, audio[k][lo:lo + HOP])
        seen = len(log)
        out = srv.step()
        labels = {}
        if len(log) > seen and gallery is not None:
            slots, _, assign, match = log[-1]
            plain.update(assign, match[0], match[1], slots)
            by_slot = dict(zip(slots, plain.labels(gallery.names, slots)))
            labels = {k: by_slot[srv._streams[k].slot] for k in out}
        ticks.append({k: [(seg.start, seg.end, g, lab) for seg, g, lab in ann.itertracks(yield_label=True)]
                      for k, ann in out.items()})
        restated.append(labels)
        if tick == 17:
            closed["ben"] = srv.close("ben")
    for k in ("ann", "late"):
        closed[k] = srv.close(k)
    return ticks, restated, closed, log


def test_server_labels_carry_the_names(gpu):
    states = synth_segmentation_state(), synth_embedding_state()
    audio = {"ann": synth_stream(300, 9.0), "ben": synth_stream(301, 9.0)}
    audio["late"] = audio["ben"]
    ticks, _, closed, log = _serve(gpu, states, audio, None)
    # pass 1: for ann and for ben's slot, a speaker g that has a turn in some step and an embedding assigned to g at
    # or before that step: that embedding is the voiceprint
    names, rows = [], []
    for k in ("ann", "ben"):
        slot = 0 if k == "ann" else 1
        steps = [i for i, out in enumerate(ticks) if k in out]
        entries = [e for e in log if slot in e[0]][:len(steps)]               # the engine steps of this stream
        found = None
        for j in range(len(steps) - 1, -1, -1):
            tracks = {g for _, _, g, _ in ticks[steps[j]][k]}
            for jj in range(j, -1, -1):
                slots, emb, assign, _ = entries[jj]
                r = slots.index(slot)
                ks = [q for q in range(assign.shape[1]) if assign[r, q] in tracks and np.isfinite(emb[r, q]).all()]
                if ks:
                    found = emb[r, ks[0]].copy()
                    break
            if found is not None:
                break
        assert found is not None, f"{k} never had a turn: the synthetic audio changed"
        names.append(f"plant-{k}")
        rows.append(found)
    noise = np.random.default_rng(5).standard_normal((500, 512)).astype(np.float32)
    gallery = SpeakerGallery(names + [f"distractor{j}" for j in range(500)], np.concatenate([np.stack(rows), noise]), gpu)

    named_ticks, restated, named_closed, named_log = _serve(gpu, states, audio, gallery)
    assert [sorted(t) for t in named_ticks] == [sorted(t) for t in ticks]
    for (_, emb, assign, _), (_, emb2, assign2, _) in zip(log, named_log):     # the gallery changes nothing it reads
        assert emb.tobytes() == emb2.tobytes() and assign.tobytes() == assign2.tobytes()
    strip = lambda ann: [(s.start, s.end, t) for s, t, _ in ann.itertracks(yield_label=True)]
    seen = set()
    for out, plain_out, labels in zip(named_ticks, ticks, restated):
        for k, turns in out.items():
            assert [t[:3] for t in turns] == [t[:3] for t in plain_out[k]]     # the same turns; only labels differ
            assert all(lab == f"speaker{g}" for _, _, g, lab in plain_out[k])
            for _, _, track, lab in turns:
                assert lab == labels[k].get(track, f"speaker{track}"), (k, track)
                seen.add((k, lab))
    assert ("ann", "plant-ann") in seen and ("ben", "plant-ben") in seen, sorted(seen)
    for k in ("ann", "ben"):
        assert f"plant-{k}" in named_closed[k].labels() and f"plant-{k}" not in closed[k].labels()
    # "late" took over ben's slot and replays ben's audio: it earns the name again, from its own steps (the restatement
    # above was reset when it joined), and what it said is what ben said
    assert strip(named_closed["late"]) == strip(named_closed["ben"])
    assert [lab for _, _, lab in named_closed["late"].itertracks(yield_label=True)] == \
        [lab for _, _, lab in named_closed["ben"].itertracks(yield_label=True)]


# ----------------------------------------------------------------------------------------------------------------- enrol
def test_enrol_is_the_normalised_mean_of_normalised_window_embeddings(gpu):
    model = M.EmbeddingModel.from_state(synth_embedding_state(), max_batch=4)
    audio = {"ann": synth_stream(41, 12.0), "ben": synth_stream(42, 3.0)[None, :]}     # 2 windows + 2 s; one short row
    gallery = SpeakerGallery.enrol(model, audio, device=gpu)
    assert gallery.names == ("ann", "ben") and gallery.dimension == 512 and len(gallery) == 2
    with torch.no_grad():
        ann = model(torch.from_numpy(audio["ann"][:160000]).reshape(2, 1, 80000).to(gpu)).cpu().double()
        ben = model(torch.from_numpy(audio["ben"]).reshape(1, 1, 48000).to(gpu)).cpu().double()
    for row, emb in zip(gallery.voiceprints, (ann, ben)):
        mean = (emb / emb.norm(dim=1, keepdim=True)).mean(dim=0)
        assert np.abs(row.astype(np.float64) - (mean / mean.norm()).numpy()).max() <= 1e-6
    with torch.no_grad():                                      # the 2 s remainder is dropped: 10 s give the same voiceprint
        again = SpeakerGallery.enrol(model, {"ann": audio["ann"][:160000]}, device=gpu)
    assert again.voiceprints[0].tobytes() == gallery.voiceprints[0].tobytes()
    # the Hip class itself (what the loader returns behind the LazyModel) enrols too
    direct = SpeakerGallery.enrol(model.model, {"ann": audio["ann"]}, device=gpu)
    assert direct.voiceprints.tobytes() == gallery.voiceprints[:1].tobytes()
