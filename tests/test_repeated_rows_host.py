"""``repeated_rows=`` without a GPU: the C entry point behind it is declared, bound and exported with one prototype;
bad values and the models that cannot share are refused before any device is touched; the argument survives pickling
of loaders and models; ``DZ_ENGINE`` carries it for a whole process."""
import ctypes as C
import pickle
import re
from pathlib import Path

import pytest

from diart_amd import _lib, config
from diart_amd import models as M
from diart_amd.synth import (synth_ecapa_state, synth_embedding_state, synth_sb_xvector_state,
                             synth_wespeaker_state)

ROOT = Path(__file__).resolve().parent.parent

SHARING = [(M.HipEmbedding, synth_embedding_state, "xvector"), (M.HipWeSpeakerEmbedding, synth_wespeaker_state, "wespeaker")]
MASKED = [(M.HipEcapaEmbedding, synth_ecapa_state, "ecapa"), (M.HipSbXvectorEmbedding, synth_sb_xvector_state, "sb-xvector")]


@pytest.fixture(autouse=True)
def _no_engine_override(monkeypatch):
    monkeypatch.delenv("DZ_ENGINE", raising=False)


def test_header_binding_and_library_agree_on_dz_rows_repeat():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "diart_amd.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+dz_rows_repeat\s*\(([^)]*)\)\s*;", text)
    assert m, "dz_rows_repeat is not declared in include/diart_amd.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["dz_ctx* ctx", "const float* d_wave", "long long wave_stride", "int n_rows", "int num_samples",
                      "void* stream", "int* repeat_out"]
    res, args = _lib.SIGNATURES["dz_rows_repeat"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    assert hasattr(C.CDLL(str(_lib.lib_path())), "dz_rows_repeat")
    fn = _lib.load().dz_rows_repeat
    assert fn.argtypes == args and fn.restype is C.c_int
    # arguments are checked before the device is: a NULL context is status 2 with a message, not a crash
    r = C.c_int(-1)
    assert fn(None, None, 0, 4, 16, None, C.byref(r)) == 2
    assert b"dz_rows_repeat" in _lib.load().dz_last_error() and r.value == -1


def test_header_says_the_call_is_synchronous():
    text = (ROOT / "include" / "diart_amd.h").read_text()
    comment = text[:text.index("int dz_rows_repeat(")].rsplit("/*", 1)[1]
    assert "synchronous" in comment.lower() and "wait" in comment


@pytest.mark.parametrize("cls,synth,arch", SHARING + MASKED)
def test_bad_value_is_refused_without_a_device(cls, synth, arch):
    with pytest.raises(ValueError, match="repeated_rows"):
        cls(synth(), repeated_rows="sometimes")
    with pytest.raises(ValueError, match="repeated_rows"):
        M.EmbeddingLoader(synth(), arch=arch, repeated_rows="sometimes")
    with pytest.raises(ValueError, match="repeated_rows"):
        M.EmbeddingModel.from_state(synth(), arch=arch, repeated_rows="")
    m = cls(synth())
    assert m.repeated_rows == "each" and m.last_shared is None and m.device is None


@pytest.mark.parametrize("cls,synth,arch", MASKED)
def test_masked_models_refuse_share_and_say_why(cls, synth, arch):
    with pytest.raises(ValueError, match="no trunk to share.*masks select the SAMPLES"):
        cls(synth(), repeated_rows="share")
    loader = M.EmbeddingLoader(synth(), arch=arch, repeated_rows="share")
    with pytest.raises(ValueError, match="no trunk to share"):
        loader()
    assert cls(synth(), repeated_rows="each").repeated_rows == "each"
    assert "repeated_rows" in pickle.loads(pickle.dumps(cls(synth()))).__getstate__()["extra"]


@pytest.mark.parametrize("cls,synth,arch", SHARING)
def test_models_and_loaders_pickle_with_the_argument(cls, synth, arch):
    m = cls(synth(), max_batch=7, repeated_rows="share")
    assert m.repeated_rows == "share" and m._extra_state()["repeated_rows"] == "share"
    again = pickle.loads(pickle.dumps(m))
    assert type(again) is cls and again.repeated_rows == "share" and again._max_batch == 7 and again.device is None
    assert pickle.loads(pickle.dumps(cls(synth()))).repeated_rows == "each"
    loader = pickle.loads(pickle.dumps(M.EmbeddingLoader(synth(), arch=arch, repeated_rows="share")))
    assert loader.repeated_rows == "share"
    built = loader()
    assert type(built) is cls and built.repeated_rows == "share"
    assert type(M.EmbeddingLoader(synth(), arch=arch)()) is cls and M.EmbeddingLoader(synth(), arch=arch)().repeated_rows == "each"
    lazy = pickle.loads(pickle.dumps(M.EmbeddingModel.from_state(synth(), arch=arch, repeated_rows="share")))
    lazy.load()
    assert lazy.model.repeated_rows == "share"
    lazy = M.EmbeddingModel.from_pretrained(synth(), repeated_rows="share")     # a state dict: decided from its keys
    lazy.load()
    assert type(lazy.model) is cls and lazy.model.repeated_rows == "share"


def test_dz_engine_key(monkeypatch):
    assert "repeated_rows" in config.KEYS
    monkeypatch.setenv("DZ_ENGINE", "repeated_rows=share")
    assert config.overrides() == {"repeated_rows": "share"}
    assert config.setting("repeated_rows", None, "each") == "share"
    assert config.setting("repeated_rows", "each", "each") == "share"
    for cls, synth, _ in SHARING:
        assert cls(synth()).repeated_rows == "share"
        assert cls(synth(), repeated_rows="each").repeated_rows == "share"
    for cls, synth, _ in MASKED:                            # the key is not theirs
        assert cls(synth()).repeated_rows == "each"
    monkeypatch.setenv("DZ_ENGINE", "repeated_rows=sometimes")
    with pytest.raises(ValueError, match="repeated_rows"):
        M.HipEmbedding(synth_embedding_state())
    monkeypatch.setenv("DZ_ENGINE", "repeated_row=share")
    with pytest.raises(ValueError, match="DZ_ENGINE"):
        config.overrides()
    monkeypatch.setenv("DZ_ENGINE", "precision=f32, repeated_rows=each")
    assert config.overrides() == {"precision": "f32", "repeated_rows": "each"}
    assert M.HipWeSpeakerEmbedding(synth_wespeaker_state(), repeated_rows="share").repeated_rows == "each"


def test_the_detector_is_part_of_the_build():
    from diart_amd import build
    assert "k_rows_repeat.hip" in build.SOURCES and (build.CSRC / "k_rows_repeat.hip").exists()
