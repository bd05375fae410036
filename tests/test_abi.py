"""The C-ABI library loads without a GPU and exports every symbol include/diart_amd.h declares;
host-only entry points (frame geometry, clustering, LSAP) work; GPU entry points fail loudly."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from diart_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def _declared():
    text = (ROOT / "include" / "diart_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dz_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    names = _declared()
    assert len(names) >= 35
    lib = C.CDLL(str(_lib.lib_path()))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/diart_amd.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes prototype in diart_amd/_lib.py"
    assert set(_lib.SIGNATURES) <= set(names)


def test_geometry_and_version():
    lib = _lib.load()
    assert lib.dz_version() == 230
    assert lib.dz_seg_frames_for(80000) == 293 and lib.dz_seg_frames_for(160000) == 589
    assert lib.dz_emb_frames_for(80000) == 279
    assert lib.dz_seg_frames_for(200) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    from diart_amd import functional, models
    from diart_amd.synth import synth_segmentation_state
    with pytest.raises(_lib.DiartAmdError):
        _lib.context(0)                                   # hipGetDeviceCount fails without a GPU
    with pytest.raises(_lib.DiartAmdError):
        functional.overlapped_speech_penalty(torch.rand(1, 10, 3))
    m = models.SegmentationModel.from_state(synth_segmentation_state())
    with pytest.raises(_lib.DiartAmdError):
        m.to(torch.device("cpu"))


def test_product_never_imports_oracle():
    for f in (ROOT / "diart_amd").rglob("*.py"):
        assert "oracle" not in f.read_text().replace("the oracle", ""), f


def test_struct_layouts_match_the_library():
    """The ctypes mirrors of the structs that cross the C ABI have the sizes the library was
    compiled with (load() refuses a mismatching library; this keeps the check itself honest)."""
    import ctypes as C
    from diart_amd import _lib
    lib = _lib.load()
    sizes = (C.c_int * 5)()
    assert lib.dz_abi_struct_sizes(C.byref(sizes)) == 0
    mine = [C.sizeof(t) for t in (_lib.SincNetWeights, _lib.SegWeights, _lib.EmbWeights,
                                  _lib.EcapaWeights, _lib.ConvGemmDesc)]
    assert list(sizes) == mine and all(v > 0 for v in mine)
    # the two halves of a tuning trial, each behind a size function of its own
    assert lib.dz_tune_abi_size() == C.sizeof(_lib.TuneDesc) > 0
    assert lib.dz_tune_cells_abi_size() == C.sizeof(_lib.TuneCells) == 12 * C.sizeof(C.c_void_p) + 5 * 4 + 4 + 8
    header = (ROOT / "include" / "diart_amd.h").read_text()
    body = re.search(r"typedef struct dz_tune_cells \{(.*?)\} dz_tune_cells;", header, flags=re.S).group(1)
    members = re.findall(r"(\w+)\s*[;,]", body)
    assert members == [name for name, _ in _lib.TuneCells._fields_], members


def test_load_refuses_a_library_with_another_dz_tune_cells(monkeypatch):
    """A library built from a header whose dz_tune_cells differs fails at load, with the message every stale struct gets."""
    monkeypatch.setattr(_lib, "_lib", None)
    stale = type("TuneCells", (C.Structure,), {"_fields_": _lib.TuneCells._fields_[:-1], "POINTERS": _lib.TuneCells.POINTERS})
    monkeypatch.setattr(_lib, "TuneCells", stale)
    with pytest.raises(_lib.DiartAmdError, match=r"built from a different include/diart_amd.h: sizeof\(dz_tune_cells\)"):
        _lib.load()


def test_header_is_plain_c_and_links_without_python(tmp_path):
    """include/diart_amd.h is a C header (C99, -pedantic clean) and a C program can call the library
    through it with no Python / torch in sight: frame geometry, version, struct sizes, and the
    error path of a call that needs a GPU context (NULL handle -> status 2 + message)."""
    import shutil
    import subprocess
    from diart_amd import _lib
    if shutil.which("gcc") is None:
        import pytest
        pytest.skip("gcc not available")
    src = tmp_path / "abi_demo.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "diart_amd.h"
int main(void) {
    int sizes[5];
    if (dz_version() <= 0 || dz_abi_struct_sizes(sizes) != 0) return 1;
    if (sizes[4] != (int)sizeof(dz_convgemm_desc) || sizes[1] != (int)sizeof(dz_seg_weights)) return 2;
    if (dz_seg_frames_for(80000) != 293 || dz_emb_frames_for(80000) != 279) return 3;
    if (dz_seg_frames_for(160000) != 589 || dz_seg_frames_for(100) != 0) return 4;
    float out[4];
    int rc = dz_seg_forward(NULL, NULL, 0, 1, out, NULL);          /* must fail loudly, not crash */
    if (rc == 0 || strlen(dz_last_error()) == 0) return 5;
    printf("abi ok v%d\n", dz_version());
    return 0;
}
''')
    exe = tmp_path / "abi_demo"
    lib = _lib.lib_path()
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(src),
           str(lib), f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_every_device_kernel_bench_names_is_in_the_library(monkeypatch):
    """bench.py joins its per-launch brackets with the rocprofv3 / PMC rows by DEVICE KERNEL SYMBOL.  A template
    parameter added to a kernel (round 4: the recurrence's packed-FMA switch) silently un-joins it — `traffic` of the
    headline kernel came out null.  Every symbol bench.py can name must be a kernel of the built library."""
    import importlib.util
    import shutil
    import subprocess
    from diart_amd import _lib
    if shutil.which("nm") is None:
        import pytest
        pytest.skip("nm not available")
    spec = importlib.util.spec_from_file_location("bench_for_symbols", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    syms = subprocess.run(["nm", "-C", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    variants = [{}, {"DZ_LSTM": "0"}, {"DZ_LSTM": "3"}, {"DZ_LSTM": "4"}, {"DZ_POOL_FUSE": "0"}, {"DZ_F32_GEMM": "0"}]
    if _lib.experiments():           # DZ_EXPERIMENTS=1: the never-default kernels are in the library too
        monkeypatch.setattr(bench, "EXPERIMENTS", True)
        variants += [{"DZ_LSTM_NC": "2"}, {"DZ_LSTM_PK": "0"}, {"DZ_LSTM": "1"}, {"DZ_LSTM": "2"}, {"DZ_GEMM_GEN": "2"},
                     {"DZ_GEMM_GEN": "3"}, {"DZ_SPLIT_WM": "2"}, {"DZ_CONV_POOL": "0"}, {"DZ_MLP_HEAD": "0"},
                     {"DZ_CONV0_SPLIT": "0"}, {"DZ_GP_LOOP": "0"}]
    missing = []
    for env in variants:
        for k in ("DZ_LSTM_NC", "DZ_LSTM_PK", "DZ_LSTM", "DZ_GEMM_GEN", "DZ_POOL_FUSE", "DZ_SPLIT_WM", "DZ_CONV_POOL",
                  "DZ_MLP_HEAD", "DZ_CONV0_SPLIT", "DZ_GP_LOOP", "DZ_G2_MT", "DZ_G3_MT", "DZ_NORM_SPLIT", "DZ_F32_GEMM"):
            monkeypatch.delenv(k, raising=False)
        bench.RECURRENCE.clear()
        for k, v in env.items():
            if k == "DZ_LSTM":          # the recurrence kernel is an engine parameter now: bench.py records what the engine runs
                bench.RECURRENCE["f16x3"] = v
            else:
                monkeypatch.setenv(k, v)
        for precision in ("f16x3", "f32"):
            for tag in bench.kernels_for(precision):
                sym = bench.device_kernel(tag, precision)[0].split(" (")[0]
                if sym + "(" not in syms and sym + "<" not in syms:       # (a template whose arguments bench leaves out)
                    missing.append((env, precision, tag, sym))
    assert not missing, missing


def test_shipped_library_has_no_experiment_surface():
    """The shipped libdiart_amd.so has one configuration per layer: no timing-only / debug entry points, no
    never-default kernel generations, and it reads no DZ_* kernel-selection variable (they exist in the
    experiments build, `python -m diart_amd.build --experiments`, loaded with DZ_EXPERIMENTS=1)."""
    import shutil
    import subprocess
    from diart_amd import _lib
    if _lib.experiments():
        pytest.skip("the experiments build is loaded")
    if shutil.which("nm") is None or shutil.which("strings") is None:
        pytest.skip("binutils not available")
    lib = _lib.lib_path()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in exported.splitlines() if ln.strip()]
    bad = [n for n in names if re.search(r"debug|dbg|gemm_g2|gemm_g3", n)]
    assert not bad, bad
    kernels = subprocess.run(["nm", "-C", str(lib)], capture_output=True, text=True, check=True).stdout
    for never_default in ("gemm_g2_kernel", "gemm_g3_kernel", "lstm_mfma1_kernel", "gemm_pre_big_kernel",
                          "lstm_rec_kernel<true, 2", "sinc_conv0_h_kernel", "sinc_conv0_pair_kernel", "conv_pool_v2_kernel"):
        assert never_default not in kernels, never_default
    env_names = sorted(set(re.findall(r"^DZ_[A-Z0-9_]+$", subprocess.run(["strings", str(lib)], capture_output=True,
                                                                      text=True, check=True).stdout, flags=re.M)))
    assert env_names == ["DZ_PROF_TIMELINE"], env_names


def test_product_reads_few_environment_switches():
    """At most 6 DZ_* variables are read by the package (each documented in README.md): engine parameters are
    constructor arguments, DZ_ENGINE is their one documented override (diart_amd/config.py); everything else goes
    through `_lib.exp_env`, which answers with the shipped default unless DZ_EXPERIMENTS=1."""
    read = set()
    for f in (ROOT / "diart_amd").rglob("*.py"):
        text = f.read_text()
        read |= set(re.findall(r"os\.environ(?:\.get\(|\[|\.setdefault\()\s*\"(DZ_[A-Z0-9_]+)\"", text))
        read |= set(re.findall(r"\"(DZ_[A-Z0-9_]+)\" (?:not )?in os\.environ", text))
    read.add("DZ_PROF_TIMELINE")                     # the one variable the C side reads (csrc/api.hip)
    assert len(read) <= 6, sorted(read)
    readme = (ROOT / "README.md").read_text()
    assert all(n in readme for n in read), sorted(n for n in read if n not in readme)


def test_options_api():
    from diart_amd import _lib
    lib = _lib.load()
    assert _lib.get_option("f32_gemm") == 1 and _lib.get_option("pool_fuse") == 1
    _lib.set_option("pool_fuse", 0)
    assert _lib.get_option("pool_fuse") == 0
    _lib.set_option("pool_fuse", 1)
    with pytest.raises(_lib.DiartAmdError):
        _lib.set_option("gemm_gen", 2)               # not an option of the library
    assert lib.dz_host_pool_set_spin(40) == 0
