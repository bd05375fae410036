"""The track tuners (VadTuneCache, OsdTuneCache) on the host against tests/golden/track_tuner.npz, the record of what
both host backends returned when the single threshold and hysteresis were separate statements of the (trial, file) pair
(tests/golden/make_track_tuner.py): every component, aggregated score and mask, bit for bit, on the cases of
tests/tune_vad_cases.py, tests/tune_osd_cases.py and tests/hysteresis_cases.py — files of 1, 3, 9, 60, 61, 300 and 520
chunks on 256 lanes (lanes without a step, one, two and three steps per lane), a silence carried across a hundred lanes,
a NaN step inside a held turn, a file that begins inside the band."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import make_track_tuner as golden  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with np.load(golden.PATH) as z:
        return {key: z[key] for key in z.files}


def compare(recorded, name, got, want_backend=None):
    """Every array of ``got`` equals the recorded one of the same name — or, for ``want_backend``, the recorded one of
    that backend.  Returns how many were compared."""
    for key, value in got.items():
        form, backend, what = key.split("_", 2)
        want = recorded[f"{name}/{form}_{want_backend(form, backend, what) if want_backend else backend}_{what}"]
        assert value.dtype == want.dtype and np.array_equal(value, want), (name, key, int((value != want).sum()))
    return len(got)


@pytest.mark.parametrize("name", list(golden.CASES))
def test_host_backends_return_the_recorded_bits(recorded, name):
    assert compare(recorded, name, golden.record(*golden.CASES[name]())) == 10
    assert sum(key.startswith(name + "/") for key in recorded) == 10
