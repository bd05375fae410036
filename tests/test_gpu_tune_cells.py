"""The four device entries of the tuners (dz_tune_score_gpu, dz_tune_vad_score, dz_tune_name, dz_tune_ident_score_gpu) with
a live context: a NULL among the members of dz_tune_cells that an entry reads (tests/tune_cells_cases.py), a `cols` that
selects no rule and more points than a sweep takes return 2 and the entry's name before anything is launched.  Nothing
here reaches a kernel: every pointer is a small zeroed buffer that no refused call dereferences; what the kernels
compute is held by the other tests/test_gpu_tune_*.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tune_cells_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calls(gpu):
    """entry -> call(cells, **what varies); `one`: 16 KB of zeros on the device, which stands for every array."""
    import torch
    from diart_amd import _lib
    lib, ctx = _lib.load(), _lib.context(gpu.index)
    zeros = torch.zeros(4096, dtype=torch.int32, device=gpu)
    one = zeros.data_ptr()
    taus = np.zeros((1, 4))                                              # one trial, four columns, host memory

    def name(cells, points=1, planes=1, assign=one):                     # (this entry takes no descriptor)
        return lib.dz_tune_name(ctx, 1, points, planes, 1, 1, 3, 5, 6, one, assign, one, one, one, one, one, one, None, 64, None)

    return lib, one, zeros, {
        "dz_tune_score_gpu": lambda cells: lib.dz_tune_score_gpu(ctx, cells, 1, one, one, one, 1, one, None),
        "dz_tune_vad_score": lambda cells, cols=2: lib.dz_tune_vad_score(ctx, cells, cols, 1, one, taus.ctypes.data, one, one, one,
                                                                           None),
        "dz_tune_name": name,
        "dz_tune_ident_score_gpu": lambda cells, points=1: lib.dz_tune_ident_score_gpu(ctx, cells, 1, points, one, one, one, one,
                                                                                      1, one, None),
    }


@pytest.mark.parametrize("entry", ["dz_tune_score_gpu", "dz_tune_vad_score", "dz_tune_ident_score_gpu"])
def test_a_null_member_is_refused_by_name(calls, entry):
    lib, one, _, call = calls
    assert cc.pointers_read(entry)
    for member in cc.pointers_read(entry):
        assert call[entry](cc.ref(cc.copy_of(cc.filled(one), **{member: None}))) == 2
        message = lib.dz_last_error().decode()
        assert message.startswith(entry + ":") and f"cells->{member}" in message, (member, message)
    assert call[entry](None) == 2 and lib.dz_last_error().decode().startswith(entry + ":")


def test_a_null_array_of_the_naming_entry_is_refused(calls):
    lib, _, _, call = calls
    assert call["dz_tune_name"](None, assign=None) == 2 and lib.dz_last_error().decode().startswith("dz_tune_name: NULL")


def test_cols_that_select_no_rule_are_refused(calls):
    lib, one, _, call = calls
    for cols in (0, 3, 5):
        assert call["dz_tune_vad_score"](cc.ref(cc.filled(one)), cols=cols) == 2
        message = lib.dz_last_error().decode()
        assert message.startswith("dz_tune_vad_score:") and f"{cols} columns" in message, message


def test_more_points_than_a_sweep_takes_are_refused(calls):
    lib, one, _, call = calls
    assert call["dz_tune_name"](None, points=257) == 2
    assert lib.dz_last_error().decode().startswith("dz_tune_name: 257 points")
    assert call["dz_tune_ident_score_gpu"](cc.ref(cc.filled(one)), points=257) == 2
    assert lib.dz_last_error().decode().startswith("dz_tune_ident_score_gpu: 257 points")


def test_nothing_was_written(calls, gpu):
    import torch
    torch.cuda.synchronize(gpu)
    assert int(calls[2].abs().sum()) == 0
