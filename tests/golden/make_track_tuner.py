"""What the track tuners (VadTuneCache, OsdTuneCache) returned before their four statements of the (trial, file) pair
were made one (csrc/tune_core.h tc_track_pair): the record tests/test_track_tuner_golden.py and
tests/test_gpu_track_tuner_golden.py hold every backend to, bit for bit.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_track_tuner.py        (no GPU; a few seconds)

Writes tests/golden/track_tuner.npz.  Per case of tests/tune_vad_cases.py, tests/tune_osd_cases.py and
tests/hysteresis_cases.py, for `(T,)` taus ("plain") and `(T, 2)` taus ("pairs"), on backend="core" and backend="host":
`evaluate(...).per_file` and the aggregated scores as the int64 bit patterns of their float64, the masks of `replay`
packed eight to a byte.  (`replay` takes no backend="core" with `(T,)` taus: that entry is absent.)  The cases of
tune_vad_cases and tune_osd_cases have no offset threshold of their own: theirs is BAND below tau_active."""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import hysteresis_cases as hc  # noqa: E402
import tune_osd_cases as oc  # noqa: E402
import tune_vad_cases as vc  # noqa: E402

PATH = HERE / "track_tuner.npz"
BAND = 0.2


def _banded(cache, taus):
    return cache, taus, np.stack([taus, taus - BAND], axis=1)


def _hysteresis(kind):
    cache = hc.cache(kind)
    pairs = hc.trials(cache.replay(np.array([hc.ON]), backend="host")[0])
    return cache, np.ascontiguousarray(pairs[:, 0]), pairs


# name -> () -> (cache, taus (T,), pairs (T, 2)); the taus are those of the tests that use the case
CASES = {f"vad_{name}": (lambda name=name: _banded(*vc.edge_cache(name))) for name in vc.EDGES}
CASES.update({f"osd_{name}": (lambda name=name: _banded(*oc.edge_cache(name))) for name in oc.EDGES})
CASES.update({
    "vad_collar": lambda: _banded(vc.collar_cache()[0], np.concatenate([vc.taus_of(33, 11), [0.5]])),
    "vad_carry": lambda: _banded(vc.carry_cache(), vc.taus_of(33, 8)),
    "vad_degenerate": lambda: _banded(vc.degenerate_cache(), vc.taus_of(33, 9)),
    "osd_carry": lambda: _banded(oc.carry_cache(), oc.taus_of(*oc.CARRY_TAUS)),
    "osd_degenerate": lambda: _banded(oc.degenerate_cache(), oc.taus_of(33, 9)),
    "hyst_vad": lambda: _hysteresis("vad"),
    "hyst_osd": lambda: _hysteresis("osd"),
})


def record(cache, taus, pairs, backends=("core", "host")) -> dict:
    """`{form}_{backend}_{what}` -> array, in the layout of the file."""
    out = {}
    for form, t in (("plain", taus), ("pairs", pairs)):
        for backend in backends:
            out[f"{form}_{backend}_per_file"] = cache.evaluate(t, backend=backend).per_file.view(np.int64)
            if backend == "core" and t.ndim == 1:
                continue
            agg, bits = cache.replay(t, backend=backend)
            assert bits.dtype == np.uint32 and bits.max() <= 1
            out[f"{form}_{backend}_agg"] = agg.view(np.int64)
            out[f"{form}_{backend}_bits"] = np.packbits(bits.astype(bool), axis=1)
    return out


def main():
    out = {}
    for name, make in CASES.items():
        got = record(*make())
        out.update({f"{name}/{key}": value for key, value in got.items()})
        print(name, {key: value.shape for key, value in got.items()}, flush=True)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, PATH.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
