"""Whole-file diarization on the GPU: the dendrogram of csrc/k_agglo.hip against the float64 yardstick
(tests/offline_ref.py), across the sizes at which the kernels take another path (a wavefront, a 256-thread block, a
64-row tile, the 1 024 threads of the merge workgroup, and the 2 048 merges of one launch of the merge kernel, after
which the next launch resumes from the state in device memory), several files per call, ties, and the whole mode end to
end.

Heights: |h - h_ref| <= 32 N 2^-52 / max(h_ref, 1e-3).  Identical merges are demanded only of inputs whose margin, by
the yardstick alone, is at least 100 times that bound, and every such test asserts it."""
import numpy as np
import pytest
import torch

import offline_cases as cases
import offline_ref as ref
from diart_amd import functional
from diart_amd.offline import OfflineDiarization
from diart_amd.optim import TuneCache

pytestmark = pytest.mark.gpu

# (N, D, clusters, noise, seed)
SIZES = [(2, 64, 1, 0.1, 0), (3, 64, 1, 0.1, 0), (65, 64, 4, 0.1, 0), (65, 192, 4, 0.1, 0), (257, 64, 6, 0.1, 7),
         (1025, 64, 8, 0.1, 1),
         # 2 048 merges fill one launch of agglo_merge_kernel exactly; one more is resumed by a second launch
         (2049, 64, 10, 0.1, 0), (2050, 64, 10, 0.1, 0)]
_yardstick = {}


def yardstick(n, d, clusters, noise, seed):
    """Computed once and shared; the arrays are not written to."""
    key = (n, d, clusters, noise, seed)
    if key not in _yardstick:
        x = ref.clustered_rows(np.random.default_rng(seed), n, d, clusters, noise)
        Z, gaps = (ref.linkage if n <= 1025 else ref.linkage_fast)(x)     # (held against each other in test_offline_host.py)
        for a in (x, Z, gaps):
            a.setflags(write=False)
        _yardstick[key] = (x, Z, gaps)
    return _yardstick[key]


def gpu_linkage(x, device):
    many = isinstance(x, (list, tuple))
    out = functional.linkage_centroid([torch.from_numpy(np.array(a)).to(device) for a in x] if many
                                      else torch.from_numpy(np.array(x)).to(device))
    return out


@pytest.mark.parametrize("case", SIZES, ids=[f"N{c[0]}-D{c[1]}" for c in SIZES])
def test_kernel_linkage_equals_yardstick(gpu, case):
    x, Z_ref, gaps = yardstick(*case)
    n = case[0]
    Z = gpu_linkage(x, gpu)
    bound = ref.height_bound(Z_ref)
    print("margin / bound", (gaps / bound).min(), "height error / bound", (np.abs(Z[:, 2] - Z_ref[:, 2]) / bound).max())
    assert (gaps >= 100 * bound).all(), "weak input: a merge of the yardstick is within 100 bounds of its runner-up"
    assert Z.shape == (n - 1, 4) and Z.dtype == np.float64 and ref.is_dendrogram(Z, n)
    assert np.array_equal(Z[:, [0, 1, 3]], Z_ref[:, [0, 1, 3]])
    assert (np.abs(Z[:, 2] - Z_ref[:, 2]) <= bound).all()
    core = functional.linkage_centroid(np.array(x))
    assert np.array_equal(Z[:, :2], core[:, :2]) and np.array_equal(Z[:, 3], core[:, 3])
    if n >= 1025:                     # scipy's own Z at the largest sizes, where it is installed
        hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
        Zs = hierarchy.linkage(x, "centroid")
        assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]]) and (np.abs(Z[:, 2] - Zs[:, 2]) <= bound).all()


def test_kernel_equals_core_bit_for_bit(gpu):
    """The host and the device compile one text with contraction off: the same rows give the same doubles."""
    x, _, _ = yardstick(*SIZES[4])
    unit = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    core, = functional.linkage_unit_rows([unit], "core")
    dev, = functional.linkage_unit_rows([unit], "gpu", gpu)
    assert np.array_equal(core, dev)


def test_files_on_both_sides_of_a_launch_boundary(gpu):
    """One call whose files need one, one and two launches of the merge kernel, and one that needs three: a file that
    is finished does nothing in the later launches, the others resume from the state in device memory.  Each file gets
    the bits of its own call alone, which are the host text's bits (the 4 200-row file is held to those alone; the host
    text is held to the yardstick and to scipy in test_offline_host.py)."""
    small = ref.clustered_rows(np.random.default_rng(41), 300, 64, 4, 0.1)
    exact, over = yardstick(*SIZES[6])[0], yardstick(*SIZES[7])[0]
    three = ref.clustered_rows(np.random.default_rng(42), 4200, 64, 12, 0.1)
    unit = [a / np.sqrt((a * a).sum(axis=1, keepdims=True)) for a in (small, exact, over, three)]
    together = functional.linkage_unit_rows(unit, "gpu", gpu)
    core = functional.linkage_unit_rows(unit, "core")
    for x, Z, Zc in zip(unit, together, core):
        assert ref.is_dendrogram(Z, x.shape[0]) and np.array_equal(Z, Zc)
        assert np.array_equal(Z, functional.linkage_unit_rows([x], "gpu", gpu)[0])
    for case, Z in ((SIZES[6], together[1]), (SIZES[7], together[2])):
        _, Z_ref, gaps = yardstick(*case)
        assert (gaps >= 100 * ref.height_bound(Z_ref)).all() and np.array_equal(Z[:, [0, 1, 3]], Z_ref[:, [0, 1, 3]])


def test_three_files_in_one_call(gpu):
    rng = np.random.default_rng(21)
    xs = [ref.clustered_rows(rng, n, 64, 3, 0.1) for n in (7, 65, 130)]
    together = gpu_linkage(xs, gpu)
    assert [z.shape for z in together] == [(6, 4), (64, 4), (129, 4)]
    for x, Z in zip(xs, together):
        assert np.array_equal(Z, gpu_linkage(x, gpu))
        Z_ref, gaps = ref.linkage(x)
        assert (gaps >= 100 * ref.height_bound(Z_ref)).all() and np.array_equal(Z[:, [0, 1, 3]], Z_ref[:, [0, 1, 3]])
    # files of 0 and 1 rows beside a real one, and groups that a small budget splits
    odd = [xs[0], np.zeros((0, 64)), xs[1][:1], xs[2]]
    got = gpu_linkage(odd, gpu)
    assert [z.shape for z in got] == [(6, 4), (0, 4), (0, 4), (129, 4)]
    assert np.array_equal(got[0], together[0]) and np.array_equal(got[3], together[2])
    split = functional.linkage_centroid([torch.from_numpy(a).to(gpu) for a in xs], memory_budget=8 * 130 * 130)
    assert all(np.array_equal(a, b) for a, b in zip(split, together))


def test_duplicate_rows_are_deterministic_and_end_in_one_cluster(gpu):
    x = np.array(ref.clustered_rows(np.random.default_rng(5), 300, 64, 3, 0.15))
    x[[10, 11, 12, 200, 299]] = x[3]
    x[150] = x[149]
    Z = gpu_linkage(x, gpu)
    assert ref.is_dendrogram(Z, 300)
    assert np.array_equal(Z, gpu_linkage(x, gpu))
    assert (Z[:6, 2] == 0).all() and Z[6, 2] > 0
    labels, _ = functional.cut_linkage(Z, 1e-9)
    assert len({labels[i] for i in (3, 10, 11, 12, 200, 299)}) == 1 and labels[149] == labels[150] != labels[3]


def turns_of(ann):
    return sorted((s.start, s.end, l) for s, _, l in ann.itertracks(yield_label=True))


def test_from_cache_gpu_equals_core(gpu):
    files = [cases.crafted_file(), cases.crafted_file(seed=9)]
    files[1]["uri"] = "second"
    cache = TuneCache.from_arrays(files, cases.config())
    on_gpu = OfflineDiarization(cases.config(), 0.7, backend="gpu").from_cache(cache)
    on_core = OfflineDiarization(cases.config(), 0.7, backend="core").from_cache(cache)
    assert [turns_of(a) for a in on_gpu] == [turns_of(a) for a in on_core] and len(on_gpu[0]) >= 3
    assert [turns_of(a) for a in OfflineDiarization(cases.config(), 0.7).from_cache(cache)] == [turns_of(a) for a in on_gpu]
    want, info = ref.diarize(files[0]["seg"], files[0]["emb"], files[0]["starts"], files[0]["res"], files[0]["shift"], 0.7,
                             cases.TAU)
    assert info["merge_ratio"] >= 100 and turns_of(on_gpu[0]) == want


def test_end_to_end_on_synthetic_weights(gpu, tmp_path):
    """A 20 s synthetic file through the models: __call__ is from_cache of the collected outputs, and both are the
    yardstick on the collected arrays.  (Synthetic weights say nothing about accuracy.)"""
    from diart_amd import models as m
    from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig
    from diart_amd.inference import write_wav
    from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream
    speech, refs = tmp_path / "wav", tmp_path / "rttm"
    speech.mkdir()
    refs.mkdir()
    write_wav(speech / "talk.wav", synth_stream(900, 20.0, num_speakers=2), 16000)
    (refs / "talk.rttm").write_text("SPEAKER talk 1 0.000 1.000 <NA> <NA> a <NA> <NA>\n")
    config = SpeakerDiarizationConfig(segmentation=m.SegmentationModel.from_state(synth_segmentation_state(), max_batch=8),
                                      embedding=m.EmbeddingModel.from_state(synth_embedding_state(), max_batch=8),
                                      tau_active=0.5, device=gpu)
    cache = TuneCache.collect(SpeakerDiarization, config, speech, refs, batch_size=8)
    f = cache.files[0]
    x, usable, train, _, _ = ref.rows_of(f["seg"], f["emb"], 0.5)
    Z, _ = ref.linkage(x[train])
    # a threshold in the widest gap between two heights of the yardstick's dendrogram: nothing is cut within rounding
    heights = np.sort(Z[:, 2])
    widest = int(np.argmax(np.diff(heights))) if heights.size > 1 else 0
    threshold = float(heights[widest] + heights[widest + 1]) / 2 if heights.size > 1 else 0.5
    offline = OfflineDiarization(config, threshold, min_cluster_size=2, backend="gpu")     # the kernels, whatever the size
    direct = offline(speech / "talk.wav", batch_size=8)
    cached, = offline.from_cache(cache)
    assert direct.uri == cached.uri == "talk" and turns_of(direct) == turns_of(cached)
    for backend in ("core", None):
        assert turns_of(OfflineDiarization(config, threshold, min_cluster_size=2, backend=backend)(speech / "talk.wav", 8)) == \
            turns_of(direct)
    want, info = ref.diarize(f["seg"], f["emb"], f["starts"], float(f["res"][0]), f["shift"], threshold, 0.5,
                             min_cluster_size=2, max_speakers=config.max_speakers)
    print("rows", x.shape, "train", train.shape, "G", info["G"], "margins", info["merge_ratio"], info["threshold_gap"],
          info["assign_gap"])
    assert info["merge_ratio"] >= 100 and info["assign_gap"] > 1e-9, "weak input"
    assert turns_of(cached) == want
    assert ref.is_dendrogram(offline.linkage(cache)[0], train.shape[0])


def test_backend_none_picks_by_size_with_the_same_bits(gpu):
    """backend=None runs files below functional.LINKAGE_GPU_MIN_ROWS on the host and the rest on the GPU: either way the
    doubles are those of each backend alone."""
    rng = np.random.default_rng(31)
    assert functional.LINKAGE_GPU_MIN_ROWS == 512
    xs = [ref.clustered_rows(rng, n, 64, 4, 0.1) for n in (130, 511, 512, 600)]
    mixed = functional.linkage_unit_rows(xs, None, gpu)
    assert all(np.array_equal(a, b) for a, b in zip(mixed, functional.linkage_unit_rows(xs, "gpu", gpu)))
    assert all(np.array_equal(a, b) for a, b in zip(mixed, functional.linkage_unit_rows(xs, "core")))
    assert all(ref.is_dendrogram(Z, x.shape[0]) for Z, x in zip(mixed, xs))


def test_command_line_collects_writes_and_reloads(gpu, tmp_path, capsys):
    """`python -m diart_amd.offline` through run(): the models over a directory, one RTTM per file, the cache written and
    then loaded instead of the models, the error rate against --reference."""
    from diart_amd import models as m
    from diart_amd import offline
    from diart_amd.inference import write_wav
    from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream
    speech, refs, out = tmp_path / "wav", tmp_path / "rttm", tmp_path / "out"
    speech.mkdir()
    refs.mkdir()
    for i, seconds in enumerate((12.0, 9.0)):
        write_wav(speech / f"f{i}.wav", synth_stream(700 + i, seconds, num_speakers=2), 16000)
        (refs / f"f{i}.rttm").write_text(f"SPEAKER f{i} 1 0.500 3.000 <NA> <NA> a <NA> <NA>\n")
    models = (m.SegmentationModel.from_state(synth_segmentation_state(), max_batch=8),
              m.EmbeddingModel.from_state(synth_embedding_state(), max_batch=8))
    base = [str(speech), "--threshold", "0.8", "--min-cluster-size", "2", "--batch-size", "8", "--backend", "gpu"]
    plain = offline.run(offline.parser().parse_args(base + ["--output", str(out / "a")]), models=models)
    assert [a.uri for a in plain] == ["f0", "f1"] and "DER" not in capsys.readouterr().out
    for ann in plain:
        assert (out / "a" / f"{ann.uri}.rttm").read_text() == ann.to_rttm()
    extra = ["--reference", str(refs), "--cache", str(tmp_path / "cache.npz")]
    wrote = offline.run(offline.parser().parse_args(base + extra + ["--output", str(out / "b")]), models=models)
    assert (tmp_path / "cache.npz").exists() and "[offline] 2 files, DER" in capsys.readouterr().out
    loaded = offline.run(offline.parser().parse_args(base + extra + ["--output", str(out / "c")]), models=None)
    for a, b, c in zip(plain, wrote, loaded):
        assert turns_of(a) == turns_of(b) == turns_of(c)
        assert (out / "c" / f"{a.uri}.rttm").read_text() == (out / "a" / f"{a.uri}.rttm").read_text()
