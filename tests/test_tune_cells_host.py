"""dz_tune_cells, the scoring geometry as one descriptor (include/diart_amd.h), without a GPU, on the seeded three-file
case of tests/test_tune_sweep_host.py (120 chunks, K = 3, G = 5) and the VoiceActivityDetection cache made from it:
every entry that takes the descriptor refuses a NULL among the members it reads, by name, and gives the same doubles
with every member it does not read NULL or 0 — the lists of the header's comments (tests/tune_cells_cases.py); and
dz_tune_vad_host's `cols` selects the rule."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cells_cases as cc  # noqa: E402
import tune_sweep_cases as sc  # noqa: E402

from diart_amd import _lib  # noqa: E402
from diart_amd.optim import TuneCache, VadTuneCache  # noqa: E402

T = 4
p = lambda a: None if a is None else a.ctypes.data


@pytest.fixture(scope="module")
def case():
    """(normalised IdentTuneCache, bits (T, rows), ident (T, 2, chunks, G), VadTuneCache of the same files, taus (T, 4));
    computed once, never changed."""
    cache = sc.normalised_cache()
    assign, status, bits = TuneCache.replay(cache, sc.hp3()[:T], backend="core")
    ident, _ = cache._names_host(assign, status, np.tile([-3.0, 0.5], (T, 1)), False, 1, (0, 1))
    vad = VadTuneCache.from_tune_cache(cache)
    taus = np.array([[0.5, 0.5, 0.0, 0.0], [0.6, 0.4, 0.3, 0.2], [0.4, 0.3, 0.0, 0.5], [0.7, 0.7, 1.0, 0.0]])
    assert cache.total_rows == vad.total_rows and int(cache.chunk_off[-1]) == 120 and (cache.K, cache.G, cache.N) == (3, 5, 3)
    return cache, bits, ident, vad, taus


def _calls(case):
    """entry -> (host cells of its cache, call(cells) -> (rc, outputs))."""
    cache, bits, ident, vad, taus = case
    lib = _lib.load()
    one = np.ascontiguousarray(ident[:, 0])
    vbits = vad.replay(taus[:, :2], backend="core")[1]
    desc = vad._desc(lambda name: getattr(vad, name).ctypes.data)

    def run(fn, shape, *args):
        out = np.full(shape, -1.0)
        return fn(*[p(out) if a is Ellipsis else a for a in args]), [out]

    def vad_host(cells, cols=4, out=True):
        q = np.ascontiguousarray(taus[:, :cols]).reshape(-1)
        agg, b = np.empty(vad.total_rows), np.zeros((T, vad.total_rows), dtype=np.uint32)
        o = np.full((T, vad.N, 5), -1.0) if out else None
        return lib.dz_tune_vad_host(C.byref(desc), cells, cols, p(q), T, p(agg), p(b), 256, p(o), 1), [agg, b, o]

    shape = (T, cache.N, 5)
    return {
        "dz_tune_score": (cache, lambda c: run(lib.dz_tune_score, shape, c, T, p(bits), ..., 1)),
        "dz_tune_score_core": (cache, lambda c: run(lib.dz_tune_score_core, shape, c, T, p(bits), 256, 4, ..., 1)),
        "dz_tune_ident_score": (cache, lambda c: run(lib.dz_tune_ident_score, shape, c, T, p(bits), p(one), ..., 1)),
        "dz_tune_ident_score_core": (cache, lambda c: run(lib.dz_tune_ident_score_core, (T, 2, cache.N, 5), c, T, 2, p(bits),
                                                          p(ident), 256, 4, ..., 1)),
        "dz_tune_track_score_dur": (vad, lambda c: run(lib.dz_tune_track_score_dur, shape, c, T, p(vbits), p(taus), ..., 1)),
        "dz_tune_vad_host": (vad, vad_host),
    }, vad_host


HOST_ENTRIES = ("dz_tune_score", "dz_tune_score_core", "dz_tune_ident_score", "dz_tune_ident_score_core",
                "dz_tune_track_score_dur", "dz_tune_vad_host")


@pytest.mark.parametrize("entry", HOST_ENTRIES)
def test_an_entry_reads_the_members_its_comment_lists(case, entry):
    lib = _lib.load()
    owner, call = _calls(case)[0][entry]
    full = owner._host_cells()
    rc, want = call(C.byref(full))
    assert rc == 0, lib.dz_last_error().decode()
    assert all(np.isfinite(w).all() for w in want) and (want[-1][..., 0] > 0).all()       # (every pair has a reference)
    # every member it reads, NULL: refused by the entry's name and the member's
    assert set(cc.READS[entry]) <= {name for name, _ in _lib.TuneCells._fields_} and cc.pointers_read(entry)
    for member in cc.pointers_read(entry):
        rc, _ = call(C.byref(cc.copy_of(full, **{member: None})))
        message = lib.dz_last_error().decode()
        assert rc == 2 and message.startswith(entry + ":") and f"cells->{member}" in message, (member, rc, message)
    rc, _ = call(None)
    assert rc == 2 and lib.dz_last_error().decode().startswith(entry + ":")
    # every member it does not read, NULL or 0: the same bits
    rc, got = call(C.byref(cc.only_what_it_reads(full, entry)))
    assert rc == 0, lib.dz_last_error().decode()
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("entry", ["dz_tune_score_gpu", "dz_tune_vad_score", "dz_tune_ident_score_gpu"])
def test_the_device_entries_name_the_member_too(case, entry):
    """Without a context nothing of a device entry runs; what can be held here is that a NULL member is refused by name
    (tests/test_gpu_tune_cells.py holds it with a live context)."""
    lib = _lib.load()
    one = p(np.zeros(64, dtype=np.int32))
    call = {"dz_tune_score_gpu": lambda c: lib.dz_tune_score_gpu(None, c, 1, one, one, one, 1, one, None),
            "dz_tune_vad_score": lambda c: lib.dz_tune_vad_score(None, c, 2, 1, one, None, one, one, one, None),
            "dz_tune_ident_score_gpu": lambda c: lib.dz_tune_ident_score_gpu(None, c, 1, 1, one, one, one, one, 1, one,
                                                                             None)}[entry]
    for member in cc.pointers_read(entry):
        assert call(C.byref(cc.copy_of(cc.filled(one), **{member: None}))) == 2
        message = lib.dz_last_error().decode()
        assert message.startswith(entry + ":") and f"cells->{member}" in message, (member, message)
    assert call(C.byref(cc.filled(one))) == 2 and "cells->" not in lib.dz_last_error().decode()     # (the NULL context)


def test_cols_selects_the_rule(case):
    _, _, _, vad, taus = case
    lib = _lib.load()
    vad_host = _calls(case)[1]
    cells = C.byref(vad._host_cells())
    for cols in (0, 3, 5):
        assert vad_host(cells, cols=cols)[0] == 2
        message = lib.dz_last_error().decode()
        assert message.startswith("dz_tune_vad_host:") and f"{cols} columns" in message, message
    # the stateless rule without components reads nothing of the geometry: no descriptor at all
    rc, (agg, bits, _) = vad_host(None, cols=1, out=False)
    assert rc == 0 and np.array_equal(bits, (agg[None, :] > taus[:, :1]).astype(np.uint32))
    assert vad_host(None, cols=2, out=False)[0] == 2 and "dz_tune_vad_host:" in lib.dz_last_error().decode()


def test_the_rules_agree_where_the_header_says_so(case):
    """cols = 2 with tau_offset == tau_active and cols = 4 with that and zero durations: the doubles of cols = 1."""
    _, _, _, vad, taus = case
    lib = _lib.load()
    desc = vad._desc(lambda name: getattr(vad, name).ctypes.data)
    cells = C.byref(vad._host_cells())
    tau = np.ascontiguousarray(taus[:, 0])
    outs, masks = {}, {}
    for cols in (1, 2, 4):
        q = np.zeros((T, cols))
        q[:, :min(cols, 2)] = tau[:, None]
        agg, bits, out = np.empty(vad.total_rows), np.zeros((T, vad.total_rows), dtype=np.uint32), np.full((T, vad.N, 5), -1.0)
        assert lib.dz_tune_vad_host(C.byref(desc), cells, cols, p(q), T, p(agg), p(bits), 256, p(out), 1) == 0
        outs[cols], masks[cols] = out, bits
    assert (outs[1][..., 1] > 0).all() and (outs[1][..., 2] > 0).any() and (outs[1][..., 3] > 0).any()
    assert len(np.unique(outs[1][:, 0], axis=0)) == T                                      # the trials differ
    for cols in (2, 4):
        assert np.array_equal(masks[cols], masks[1])
        assert np.array_equal(outs[cols].view(np.int64), outs[1].view(np.int64)), cols
