"""The track tuners on the GPU (csrc/k_tune_vad.hip: tune_vad_score_kernel under both row rules, the rows and the bits
kernels) against tests/golden/track_tuner.npz, on the cases of tests/test_track_tuner_golden.py.  The record was taken
on the host: the aggregated scores and the masks of "gpu" are held to it where the GPU tests have always held them to
the host exactly (the `(T,)` masks to backend="host", the `(T, 2)` masks to backend="core"), and so are the components,
to backend="core": kernel and host compile one text (csrc/tune_core.h tc_track_pair) whose doubles come from compares,
differences of prefix sums and sums in lane order, without contraction, so there is nothing for the two to differ in.
The masks of the two host backends are asserted here too."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_track_tuner_golden as host  # noqa: E402
from test_track_tuner_golden import golden, recorded  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(golden.CASES))
def test_gpu_returns_the_recorded_bits(gpu, recorded, name):  # noqa: F811
    got = golden.record(*golden.CASES[name](), backends=("gpu", "core", "host"))
    masks = {key: value for key, value in got.items() if key.endswith("_bits")}
    assert len(masks) == 5 and host.compare(recorded, name, {k: v for k, v in got.items() if "_gpu_" not in k}) == 10
    on_gpu = {key: value for key, value in got.items() if "_gpu_" in key}
    assert host.compare(recorded, name, on_gpu, lambda form, backend, what: "host" if form == "plain" and what != "per_file"
                        else "core") == 6
