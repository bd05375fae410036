"""File batches for every engine: the gather kernel that stages a step's rows (``dz_gather_windows``, bit for bit against
``unfold`` + ``copy_``), and ``FileBatch`` / ``Benchmark`` over the WeSpeaker, VAD and groups-form engines — their RTTM
files must be BYTE-identical to the one-file-at-a-time loop's, whatever the number of concurrent files.  Every
comparison is an equality, so there is no tolerance here."""
import gc
import io

import numpy as np
import pytest
import torch

from diart_amd import _lib
from diart_amd import models as M
from diart_amd.blocks import (SpeakerDiarization, SpeakerDiarizationConfig, VoiceActivityDetection,
                              VoiceActivityDetectionConfig)
from diart_amd.synth import (synth_ecapa_state, synth_segmentation_state, synth_stream, synth_wespeaker_state)

pytestmark = pytest.mark.gpu
SR = 16000
# the six files of test_gpu_der.py's file-batch test: one ends mid-block, one is shorter than a window (left padding), one
# has fewer windows than the others have per step
FILES = (("a", 11, 21.3), ("b", 12, 9.05), ("c", 13, 33.0), ("d", 14, 3.2), ("e", 15, 5.5), ("f", 16, 14.77))
SENTINEL = -123.25


# ------------------------------------------------------------------------------------------------ the gather kernel
def _gather(gpu, runs, S, hop, out, out_rows=None, stride=None):
    """-> return code.  ``runs``: (source tensor | None, row0, count)."""
    lib = _lib.load()
    table = (_lib.WindowRun * max(1, len(runs)))()
    for t, (src, row0, count) in zip(table, runs):
        t.src, t.row0, t.count = (None if src is None else src.data_ptr()), row0, count
    return lib.dz_gather_windows(_lib.context(gpu.index), table, len(runs), S, hop, out.data_ptr(),
                                 out.stride(0) if stride is None else stride, out.shape[0] if out_rows is None else out_rows,
                                 torch.cuda.current_stream(gpu).cuda_stream)


def _audio(gpu, n, seed, offset=0):
    """n samples of noise on the GPU, starting ``offset`` floats into their allocation."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n + offset, generator=g).to(gpu)[offset:]


GATHER_CASES = {
    # name: (S, hop, [(row0, count)], source offset in floats)
    "one run": (80000, 8000, [(0, 64)], 0),
    "64 runs of one row": (80000, 8000, [(i, 1) for i in range(64)], 0),
    "65 runs of one row": (80000, 8000, [(i, 1) for i in range(65)], 0),
    "a zero-count run": (80000, 8000, [(0, 5), (5, 0), (5, 59)], 0),
    "the smallest aligned hop": (1004, 4, [(0, 3), (3, 6)], 0),
    "scalar path": (1001, 3, [(0, 3), (3, 6)], 0),
    "unaligned source, aligned parameters": (1004, 4, [(0, 3), (3, 6)], 1),
}


@pytest.mark.parametrize("name", list(GATHER_CASES))
def test_gather_windows_is_unfold_and_copy_bit_for_bit(gpu, name):
    S, hop, runs, offset = GATHER_CASES[name]
    rows = max(r0 + c for r0, c in runs)
    out = torch.full((rows + 2, S + 12), SENTINEL, device=gpu)
    want = out.clone()
    table = []
    for i, (row0, count) in enumerate(runs):
        src = _audio(gpu, S + hop * max(count - 1, 0), 100 + i, offset)
        assert src.data_ptr() % 16 == (4 * offset) % 16
        table.append((src, row0, count))
        if count:
            want[row0:row0 + count, :S].copy_(src.unfold(0, S, hop))
    assert _gather(gpu, table, S, hop, out) == 0, _lib.load().dz_last_error()
    torch.cuda.synchronize()
    got, want = out.cpu().numpy().view(np.int32), want.cpu().numpy().view(np.int32)
    assert np.array_equal(got[:rows, :S], want[:rows, :S]), "the gathered rows differ from unfold + copy_"
    assert np.array_equal(got, want), "something outside the requested rows / columns was written"


def test_gather_windows_refuses_bad_arguments_and_writes_nothing(gpu):
    S, hop = 1004, 4
    src = _audio(gpu, S + 3 * hop, 1)
    out = torch.full((6, S + 12), SENTINEL, device=gpu)
    good = [(src, 0, 2), (src, 2, 2)]
    bad = {
        "row0 < 0": lambda: _gather(gpu, [(src, 0, 2), (src, -1, 2)], S, hop, out),
        "row0 + count > out_rows": lambda: _gather(gpu, [(src, 0, 2), (src, 3, 4)], S, hop, out),
        "rows beyond a smaller out_rows": lambda: _gather(gpu, good, S, hop, out, out_rows=3),
        "out_stride < num_samples": lambda: _gather(gpu, good, S, hop, out, stride=S - 1),
        "hop < 1": lambda: _gather(gpu, good, S, 0, out),
        "n_runs < 1": lambda: _gather(gpu, [], S, hop, out),
        "NULL src with rows": lambda: _gather(gpu, [(src, 0, 2), (None, 2, 2)], S, hop, out),
        "negative count": lambda: _gather(gpu, [(src, 0, 2), (src, 2, -1)], S, hop, out),
    }
    for name, call in bad.items():
        assert call() == 2, name
        assert b"dz_gather_windows" in _lib.load().dz_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the destination"
    assert _gather(gpu, [(src, 0, 2), (None, 2, 0)], S, hop, out) == 0      # a NULL source of an empty run is fine
    torch.cuda.synchronize()
    assert torch.equal(out[:2, :S], src.unfold(0, S, hop)[:2]) and bool((out[2:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the file batches
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from diart_amd.inference import write_wav
    root = tmp_path_factory.mktemp("file_batch_models")
    speech = root / "wav"
    speech.mkdir()
    for name, seed, dur in FILES:
        write_wav(speech / f"{name}.wav", synth_stream(seed, dur), SR)
    return root, speech


def _rttms(folder):
    return {p.name: p.read_text() for p in sorted(folder.iterdir())}


def _speakers(rttm_text):
    return {line.split()[7] for line in rttm_text.splitlines() if line.strip()}


def _benchmark(speech, out, pipeline, cfg, batch_size, k, rows=None):
    from diart_amd.inference import Benchmark
    b = Benchmark(speech, None, out, show_report=False, batch_size=batch_size, concurrent_files=k)
    if rows is not None:
        b.file_batch_rows = rows
    b(pipeline, cfg)
    path = b.last_path
    del b
    gc.collect()
    return path, _rttms(out)


# the model pairs of the WeSpeaker form: (powerset segmentation?, latency)
WESPEAKER_PAIRS = {"plain-0.5": (False, 0.5), "powerset-2.0": (True, 2.0)}
_cache: dict = {}


def _wespeaker_cfg(gpu, pair):
    powerset, latency = WESPEAKER_PAIRS[pair]
    if ("wsp", pair) not in _cache:
        seg_sd = synth_segmentation_state(seed=77, powerset=True) if powerset else synth_segmentation_state()
        _cache["wsp", pair] = SpeakerDiarizationConfig(
            segmentation=M.SegmentationModel.from_state(seg_sd, max_batch=32, powerset=powerset),
            embedding=M.EmbeddingModel.from_state(synth_wespeaker_state(), max_batch=32),
            latency=latency, tau_active=0.5 if powerset else 0.6, device=gpu)
    return _cache["wsp", pair]


def _loop(corpus, tag, pipeline, cfg, batch_size, diarization):
    """The one-file-at-a-time loop's RTTM files (computed once per configuration), checked to be worth comparing with:
    some file has turns and, for a diarization, some file has two or more speakers."""
    if ("loop", tag) not in _cache:
        root, speech = corpus
        path, files = _benchmark(speech, root / f"{tag}-loop", pipeline, cfg, batch_size, 0)
        assert path == "one_file_at_a_time"
        assert sorted(files) == [f"{n}.rttm" for n, *_ in FILES]
        assert any(len(t) > 0 for t in files.values()), "the loop found no speech at all"
        if diarization:
            assert max(len(_speakers(t)) for t in files.values()) >= 2, "the loop never tells two speakers apart"
        _cache["loop", tag] = files
    return _cache["loop", tag]


@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("pair", list(WESPEAKER_PAIRS))
def test_wespeaker_files_batched_together_give_the_rttm_files_of_the_loop(gpu, corpus, pair, k):
    """``Benchmark`` with a ``HipWeSpeakerEmbedding`` takes the file batch (on the code before this form existed
    ``last_path`` stayed "one_file_at_a_time" for every ``concurrent_files``) and writes the loop's RTTM files."""
    cfg = _wespeaker_cfg(gpu, pair)
    want = _loop(corpus, f"wsp-{pair}", SpeakerDiarization, cfg, 32, True)
    path, got = _benchmark(corpus[1], corpus[0] / f"wsp-{pair}-k{k}", SpeakerDiarization, cfg, 32, k)
    assert path == "file_batch"
    assert got == want, f"k={k}: RTTM files differ from the one-file-at-a-time loop"


VAD_TIMINGS = {"step0.5-latency0.5": (0.5, 0.5), "step0.25-latency1.0": (0.25, 1.0)}


@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("timing", list(VAD_TIMINGS))
def test_vad_files_batched_together_give_the_rttm_files_of_the_loop(gpu, corpus, timing, k):
    step, latency = VAD_TIMINGS[timing]
    if ("vad", timing) not in _cache:
        _cache["vad", timing] = VoiceActivityDetectionConfig(
            segmentation=M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=32), step=step,
            latency=latency, device=gpu)
    cfg = _cache["vad", timing]
    want = _loop(corpus, f"vad-{timing}", VoiceActivityDetection, cfg, 32, False)
    path, got = _benchmark(corpus[1], corpus[0] / f"vad-{timing}-k{k}", VoiceActivityDetection, cfg, 32, k)
    assert path == "file_batch"
    assert got == want, f"k={k}: RTTM files differ from the one-file-at-a-time loop"
    assert set().union(*(_speakers(t) for t in got.values())) == {"speech"}


GROUP_FILES = ("a", "b", "e")


@pytest.fixture(scope="module")
def groups(gpu, corpus, tmp_path_factory):
    """Powerset segmentation + ECAPA-TDNN with normalised OSP weights (BASELINE config 3) on three of the files, and the
    loop's RTTM files at ``batch_size=1``."""
    import shutil
    root = tmp_path_factory.mktemp("file_batch_groups")
    speech = root / "wav"
    speech.mkdir()
    for n in GROUP_FILES:
        shutil.copy(corpus[1] / f"{n}.wav", speech / f"{n}.wav")
    cfg = SpeakerDiarizationConfig(
        segmentation=M.SegmentationModel.from_state(synth_segmentation_state(seed=77, powerset=True), max_batch=32,
                                                    powerset=True),
        embedding=M.EmbeddingModel.from_state(synth_ecapa_state(), max_batch=96), latency=0.5, tau_active=0.5,
        normalize_embedding_weights=True, device=gpu)
    path, want = _benchmark(speech, root / "loop", SpeakerDiarization, cfg, 1, 0)
    assert path == "one_file_at_a_time" and sorted(want) == [f"{n}.rttm" for n in GROUP_FILES]
    assert any(len(t) > 0 for t in want.values()), "the loop found no speech at all"
    assert max(len(_speakers(t)) for t in want.values()) >= 2, "the loop never tells two speakers apart"
    return root, speech, cfg, want


@pytest.mark.parametrize("m", [1, 3])
def test_groups_form_file_batch_gives_the_rttm_files_of_the_loop_at_batch_one(gpu, groups, m):
    from diart_amd.inference import read_wav_resampled_into
    from diart_amd.pipeline import FileBatch, GroupsBatch
    root, speech, cfg, want = groups
    cfg.segmentation.load()
    cfg.embedding.load()
    fb = FileBatch(cfg.segmentation.model, cfg.embedding.model, rows=8, max_files=m, tau_active=cfg.tau_active,
                   rho_update=cfg.rho_update, delta_new=cfg.delta_new, gamma=cfg.gamma, beta=cfg.beta,
                   max_speakers=cfg.max_speakers, normalize_embedding_weights=True, duration=cfg.duration,
                   step=cfg.step, latency=cfg.latency, device=gpu)
    assert fb.kind == "groups" and isinstance(fb.engine, GroupsBatch)

    def feed():
        for n in GROUP_FILES:
            padded, _, padding = read_wav_resampled_into(speech / f"{n}.wav", fb.host_buffer, cfg.get_padding, cfg.step,
                                                         cfg.sample_rate, gpu)
            yield n, padded, -padding[0]
    got = {}
    for uri, ann in fb.run(feed()).items():
        ann.uri = uri
        text = io.StringIO()
        ann.write_rttm(text)
        got[f"{uri}.rttm"] = text.getvalue()
    del fb
    gc.collect()
    assert got == want, f"max_files={m}: RTTM files differ from the loop at batch_size=1"


def test_groups_form_routes_by_batch_size(gpu, groups):
    root, speech, cfg, want = groups
    path, got = _benchmark(speech, root / "bs1", SpeakerDiarization, cfg, 1, 16, rows=8)
    assert path == "file_batch" and got == want
    path, _ = _benchmark(speech, root / "bs32", SpeakerDiarization, cfg, 32, 16, rows=8)
    assert path == "one_file_at_a_time"


# ------------------------------------------------------------------------------------------------ plumbing
def test_single_rank_distributed_benchmark_is_benchmark_and_reuses_its_file_batch(gpu, corpus):
    from diart_amd.inference import Benchmark, DistributedBenchmark
    from diart_amd.pipeline import FileBatch, WeSpeakerBatch
    root, speech = corpus
    cfg = _wespeaker_cfg(gpu, "plain-0.5")
    want = _loop(corpus, "wsp-plain-0.5", SpeakerDiarization, cfg, 32, True)
    refs = root / "refs"
    refs.mkdir(exist_ok=True)
    for name, text in want.items():
        (refs / name).write_text(text)
    b = Benchmark(speech, refs, root / "plumb1", show_report=False, batch_size=32, concurrent_files=16)
    metric = b(SpeakerDiarization, cfg)
    assert b.last_path == "file_batch"
    fb = b.file_batch(SpeakerDiarization, cfg)
    assert isinstance(fb, FileBatch) and fb.kind == "wespeaker" and isinstance(fb.engine, WeSpeakerBatch)
    m2 = DistributedBenchmark(b)(SpeakerDiarization, cfg)
    assert b.file_batch(SpeakerDiarization, cfg) is fb, "a second call with the same config built another FileBatch"
    assert m2.accumulated == metric.accumulated and metric.accumulated["total"] > 1.0
    b2 = Benchmark(speech, refs, root / "plumb2", show_report=False, batch_size=32, concurrent_files=16)
    b2._fb_cache = b._fb_cache                                  # (the same engine: nothing new to allocate)
    DistributedBenchmark(b2)(SpeakerDiarization, cfg)
    assert _rttms(root / "plumb2") == _rttms(root / "plumb1") == want
    del b, b2, fb
    gc.collect()


def test_vad_form_refuses_a_duplicate_uri_and_runs_again(gpu):
    from diart_amd.pipeline import FileBatch, VadBatch
    fb = FileBatch(M.HipSegmentation(synth_segmentation_state(), max_batch=8), None, pipeline="vad", rows=8, max_files=4,
                   device=gpu)
    assert fb.kind == "vad" and isinstance(fb.engine, VadBatch)
    one, two = (synth_stream(21, 7.0).astype(np.float32), synth_stream(22, 6.5).astype(np.float32))
    short = synth_stream(23, 2.0).astype(np.float32)
    with pytest.raises(ValueError, match="share the uri"):
        fb.run([("x", one, 0.0), ("y", two, 0.0), ("x", two, 0.0)])
    got = fb.run([("x", one, 0.0), ("y", two, 0.0), ("z", short, 0.0)])
    assert sorted(got) == ["x", "y", "z"] and len(got["z"]) == 0        # shorter than one window: an empty annotation
    assert any(len(got[u]) for u in "xy")
    assert all(label == "speech" for u in got for label in got[u].labels())
    again = fb.run([("x", one, 0.0)])
    assert again["x"].to_rttm() == got["x"].to_rttm()


def test_pyannote_embedding_form_stages_the_same_rows_with_the_kernel_as_with_its_copies(gpu):
    """The form that existed keeps its torch copies by default (``FileBatch.GATHER_DEFAULT``); asked for the kernel it
    gives the same turns."""
    from diart_amd.pipeline import FileBatch, StreamBatch
    from diart_amd.synth import synth_embedding_state
    seg = M.HipSegmentation(synth_segmentation_state(), max_batch=8)
    emb = M.HipEmbedding(synth_embedding_state(), max_batch=8)
    files = [("x", synth_stream(11, 21.3).astype(np.float32), 0.0), ("y", synth_stream(12, 9.05).astype(np.float32), 0.0),
             ("z", synth_stream(15, 5.5).astype(np.float32), 0.0)]
    got = {}
    for gather in (None, True):
        fb = FileBatch(seg, emb, rows=8, max_files=3, device=gpu, gather=gather)
        assert fb.kind == "xvector" and type(fb.engine) is StreamBatch and fb.gather is bool(gather)
        got[gather] = {u: a.to_rttm() for u, a in fb.run(files).items()}
        del fb
        gc.collect()
    assert any(got[None].values()) and got[True] == got[None]
