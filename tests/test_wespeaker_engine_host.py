"""The WeSpeaker ResNet34 embedding on the N-stream engine, the parts that need no GPU: the two halves of the forward
(``dz_wsp_trunk`` / ``dz_wsp_pool``) are exported, bound and declared in a header that is still plain C99 and refuse bad
arguments before they touch a device; ``WeSpeakerBatch`` exists and refuses what it cannot run before it touches a
device; the package reads no environment variable it did not read before."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from diart_amd import _lib, models
from diart_amd.synth import synth_ecapa_state, synth_embedding_state, synth_segmentation_state, synth_wespeaker_state

ROOT = Path(__file__).resolve().parent.parent


# --------------------------------------------------------------------------- the C ABI
def test_the_two_halves_are_exported_bound_and_declared():
    lib = C.CDLL(str(_lib.lib_path()))
    for name in ("dz_wsp_trunk", "dz_wsp_pool", "dz_wsp_forward_multi", "dz_wsp_peek"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["dz_wsp_trunk"]
    assert res is C.c_int and len(args) == 5 and args[2] is C.c_longlong and args[3] is C.c_int
    res, args = _lib.SIGNATURES["dz_wsp_pool"]
    assert res is C.c_int and len(args) == 8 and all(a is C.c_int for a in args[2:6])
    header = (ROOT / "include" / "diart_amd.h").read_text()
    assert "int dz_wsp_trunk(dz_wsp* m, const float* d_wave, long long wave_stride, int batch, void* stream);" in header
    assert re.search(r"int dz_wsp_pool\(dz_wsp\* m, const float\* d_weights, int batch, int num_speakers, "
                     r"int weight_frames, int normalize,\s+float\* d_out, void\* stream\);", header)
    assert "ONE trunk at a" in header.replace("\n * ", " "), "the header states that a handle carries one trunk at a time"


def test_header_with_the_halves_is_plain_c99(tmp_path):
    """As tests/test_abi.py checks the header: a C99 program (-pedantic -Werror) that calls the two halves through
    include/diart_amd.h compiles, links and gets an error status, not a crash, from a NULL handle."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "wsp_halves.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "diart_amd.h"
int main(void) {
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4];
    if (dz_wsp_trunk(NULL, x, 4, 1, NULL) == 0 || strstr(dz_last_error(), "dz_wsp_trunk") == NULL) return 1;
    if (dz_wsp_pool(NULL, x, 1, 1, 4, 1, out, NULL) == 0 || strstr(dz_last_error(), "dz_wsp_pool") == NULL) return 2;
    if (dz_wsp_frames_for(80000, 0) != 498) return 3;
    printf("halves ok\n");
    return 0;
}
''')
    exe, lib = tmp_path / "wsp_halves", _lib.lib_path()
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(src),
           str(lib), f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "halves ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("call, what", [
    (lambda lib: lib.dz_wsp_trunk(None, 16, 80000, 1, None), "dz_wsp_trunk: NULL argument"),
    (lambda lib: lib.dz_wsp_pool(None, 16, 1, 3, 293, 1, 16, None), "dz_wsp_pool: NULL argument"),
])
def test_the_halves_refuse_a_null_handle_without_touching_the_gpu(call, what):
    lib = _lib.load()
    assert call(lib) != 0
    assert what in lib.dz_last_error().decode()


def test_model_has_the_raw_address_launchers():
    for name, params in (("trunk_launch", ["self", "handle", "wave_ptr", "wave_stride", "batch", "stream_ptr"]),
                         ("pool_launch", ["self", "handle", "weights_ptr", "batch", "K", "weight_frames", "normalize",
                                          "out_ptr", "stream_ptr"])):
        fn = getattr(models.HipWeSpeakerEmbedding, name)
        assert list(inspect.signature(fn).parameters) == params
        assert "synchronize" not in inspect.getsource(fn).split('"""')[2], f"{name} must not synchronise"


# --------------------------------------------------------------------------- the engine, without a device
def _seg():
    return models.HipSegmentation(synth_segmentation_state())


def test_wespeaker_batch_has_stream_batch_s_arguments_and_surface():
    from diart_amd.pipeline import StreamBatch, WeSpeakerBatch
    mine = inspect.signature(WeSpeakerBatch.__init__).parameters
    theirs = inspect.signature(StreamBatch.__init__).parameters
    names = list(mine)
    assert names == ["self", "segmentation", "embedding", "num_streams", "tau_active", "rho_update", "delta_new", "gamma",
                     "beta", "max_speakers", "normalize_embedding_weights", "device", "cluster_threads", "tail",
                     "duration", "step", "latency", "lanes", "recurrence", "inflight", "wait", "warmup"]
    for n in names[4:17]:
        assert mine[n].default == theirs[n].default, n
        assert mine[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for n in names[17:]:
        assert mine[n].kind is inspect.Parameter.KEYWORD_ONLY and mine[n].default is None
    for attr in ("launch", "finish", "reset", "diarize", "__call__", "set_host_threads"):
        assert callable(getattr(WeSpeakerBatch, attr)), attr
    assert list(inspect.signature(WeSpeakerBatch.launch).parameters) == ["self", "waves", "starts", "slots"]
    assert list(inspect.signature(WeSpeakerBatch.finish).parameters) == ["self", "ticket", "want_scores"]


@pytest.mark.parametrize("make", [
    lambda: models.HipEmbedding(synth_embedding_state()),
    lambda: models.HipEcapaEmbedding(synth_ecapa_state()),
])
def test_wespeaker_batch_refuses_other_embeddings_without_a_device(make):
    from diart_amd.pipeline import WeSpeakerBatch
    seg, emb = _seg(), make()
    with pytest.raises(ValueError, match="StreamBatch"):
        WeSpeakerBatch(seg, emb, 2)
    assert seg.device is None and emb.device is None, "refused after the models had been moved to a device"


@pytest.mark.parametrize("kw", [dict(latency=0.25), dict(latency=6.0), dict(step=0.5, duration=5.0, latency=5.5),
                                dict(wait="sleep"), dict(wait="")])
def test_wespeaker_batch_refuses_bad_latency_and_wait_without_a_device(kw):
    from diart_amd.pipeline import WeSpeakerBatch
    seg, emb = _seg(), models.HipWeSpeakerEmbedding(synth_wespeaker_state())
    with pytest.raises(ValueError, match="latency" if "latency" in kw else "wait"):
        WeSpeakerBatch(seg, emb, 2, **kw)
    assert seg.device is None and emb.device is None


def test_wespeaker_batch_has_no_sub_batches_and_no_serial_form():
    from diart_amd.pipeline import WeSpeakerBatch
    seg, emb = _seg(), models.HipWeSpeakerEmbedding(synth_wespeaker_state())
    for kw in (dict(seg_split=2), dict(emb_split=2), dict(serial=True), dict(depth=2)):
        with pytest.raises(TypeError):
            WeSpeakerBatch(seg, emb, 2, **kw)


def test_stream_batch_points_to_wespeaker_batch():
    from diart_amd.pipeline import StreamBatch
    with pytest.raises(ValueError, match="WeSpeakerBatch"):
        StreamBatch(_seg(), models.HipWeSpeakerEmbedding(synth_wespeaker_state()), 2)


# --------------------------------------------------------------------------- no new environment variable
# what the package read before this engine existed: os.environ reads, and the experiments build's switches
ENVIRONMENT = {"DZ_DIST_BACKEND", "DZ_ENGINE", "DZ_EXPERIMENTS", "DZ_FORCE_DEVICE", "HIPCC", "HSA_ENABLE_IPC_MODE_LEGACY",
               "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE"}
EXPERIMENT_SWITCHES = {"DZ_ABLATE", "DZ_CONV0_PAIR", "DZ_CONV0_SPLIT", "DZ_EMB_SPLIT", "DZ_GEMM_GEN", "DZ_PRIO_A", "DZ_PRIO_B",
                       "DZ_PRIO_F", "DZ_RING_ZERO_COPY", "DZ_SEG_FRONT", "DZ_SEG_SPLIT", "DZ_SHARED_EMB", "DZ_SHARED_STATS"}


def test_package_reads_no_new_environment_variable():
    read, switches = set(), set()
    for f in (ROOT / "diart_amd").rglob("*.py"):
        text = f.read_text()
        read |= set(re.findall(r"os\.environ(?:\.get\(|\[|\.setdefault\(|\.pop\()\s*\"([A-Za-z0-9_]+)\"", text))
        read |= set(re.findall(r"\"([A-Za-z0-9_]+)\" (?:not )?in os\.environ", text))
        read |= set(re.findall(r"getenv\(\s*\"([A-Za-z0-9_]+)\"", text))
        switches |= set(re.findall(r"exp_env\(\s*\"([A-Za-z0-9_]+)\"", text))
    assert read <= ENVIRONMENT, sorted(read - ENVIRONMENT)
    assert switches <= EXPERIMENT_SWITCHES, sorted(switches - EXPERIMENT_SWITCHES)
    strings = shutil.which("strings")
    if strings is not None and not _lib.experiments():
        out = subprocess.run([strings, str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"^DZ_[A-Z0-9_]+$", out, flags=re.M))) == ["DZ_PROF_TIMELINE"]
