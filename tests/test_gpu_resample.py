"""The resampler on the GPU (DESIGN.md "Resampling"): the kernel against the float64 restatement
(tests/resample_ref.py) at every accepted rate and length class, bit-for-bit batch invariance, the reach of
non-finite samples, and the three places that take audio at another rate than the pipeline's — ``StreamingInference``
(whole waveform), ``Benchmark`` (whole files, both paths) and ``StreamServer(input_sample_rate=...)`` (each window
on its own, the reference's ``blocks.Resample``)."""
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from diart_amd import models as M
from diart_amd.functional import Resampler, resample
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_streams

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = [44100, 22050, 11025, 48000, 32000, 8000, 12000, 24000, 88200, 96000]
GATE_MAX, GATE_REL = 1e-5, 2e-6


def _signal(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


@pytest.mark.parametrize("orig", RATES)
def test_kernel_matches_the_float64_restatement(gpu, orig):
    o, n, width, T = R.geometry(orig, 16000)
    rs = Resampler(orig, 16000, gpu)
    worst = (0.0, 0.0)
    # 64 five-second windows, a 40 s whole file, lengths that are not a multiple of o, shorter than width
    cases = [(64, 5 * orig), (1, 40 * orig), (3, 5 * orig + o // 2 + 1), (2, 7 * o + 1), (2, max(1, width - 1)),
             (1, 1)]
    for c, (rows, L) in enumerate(cases):
        x = np.stack([_signal(L, 100 * c + r) for r in range(rows)])
        got = rs.rows(torch.from_numpy(x).to(gpu)).cpu().numpy().astype(np.float64)
        want = R.resample(x, orig, 16000)
        assert got.shape == want.shape == (rows, R.out_len(orig, 16000, L))
        err = np.abs(got - want).max()
        rel = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
        worst = (max(worst[0], err), max(worst[1], rel))
        assert err <= GATE_MAX and rel <= GATE_REL, (orig, rows, L, err, rel)
    print(f"\n[resample] {orig} Hz -> 16 kHz: max |d| {worst[0]:.3g}, relative L2 {worst[1]:.3g}")


@pytest.mark.parametrize("orig", [44100, 48000, 8000])
def test_rows_are_batch_invariant_bit_for_bit(gpu, orig):
    """A row alone, the same row in a batch of 64, and the same row read through a strided view of one buffer
    (what an AudioRing window or a rolling window batch is) give identical bits."""
    rs = Resampler(orig, 16000, gpu)
    L, hop = 5 * orig, orig // 2
    flat = torch.from_numpy(_signal(L + 63 * hop, 7)).to(gpu)
    view = flat.as_strided((64, L), (hop, 1))
    batch = view.contiguous()
    alone = [rs.rows(batch[r:r + 1].clone()) for r in (0, 17, 63)]
    full = rs.rows(batch)
    strided = rs.rows(view)
    padded = torch.zeros((64, L + 100), device=gpu)
    padded[:, :L] = batch
    wide = rs.rows(padded[:, :L])
    for a, r in zip(alone, (0, 17, 63)):
        for other in (full, strided, wide):
            assert torch.equal(a[0], other[r])


@pytest.mark.parametrize("orig", [44100, 48000, 22050, 8000])
def test_nonfinite_samples_reach_exactly_the_covering_outputs(gpu, orig):
    x = _signal(3 * orig, 5)
    L = len(x)
    x[[0, L // 3, L // 3 + 1, 2 * L // 3, L - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    got = Resampler(orig, 16000, gpu)(torch.from_numpy(x)).numpy()
    want = R.nonfinite_reach(x, orig, 16000)
    assert np.array_equal(~np.isfinite(got), want)
    assert not np.isfinite(R.resample(x, orig, 16000)[want]).any()


def test_equal_rates_return_the_input(gpu):
    x = torch.from_numpy(_signal(1000, 1)).to(gpu)
    assert resample(x, 16000, 16000) is x
    from diart_amd.blocks import Resample
    y = Resample(16000, 16000, gpu)(x[None, :, None])
    assert torch.equal(y[0, :, 0], x)


def test_resample_block_keeps_the_reference_types(gpu):
    from diart_amd.blocks import Resample
    from diart_amd.features import SlidingWindow, SlidingWindowFeature
    x = _signal(5 * 44100, 3)
    blk = Resample(44100, 16000, gpu)
    swf = SlidingWindowFeature(x[:, None], SlidingWindow(start=2.5, duration=1 / 44100, step=1 / 44100))
    out = blk(swf)
    assert isinstance(out, SlidingWindowFeature) and out.data.shape == (80000, 1)
    assert out.sliding_window.start == 2.5 and abs(out.sliding_window.duration - 5.0 / 80000) < 1e-15
    want = resample(x, 44100, 16000)
    assert np.array_equal(out.data[:, 0], want)
    nb = blk(np.stack([x, x])[:, :, None])
    assert isinstance(nb, np.ndarray) and nb.shape == (2, 80000, 1) and np.array_equal(nb[1, :, 0], want)
    tb = blk(torch.from_numpy(x)[:, None])
    assert tb.is_cuda and tuple(tb.shape) == (1, 80000, 1)


def _config(gpu, latency=0.5, max_batch=32):
    from diart_amd.blocks import SpeakerDiarizationConfig
    seg = M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=max_batch)
    emb = M.EmbeddingModel.from_state(synth_embedding_state(), max_batch=max_batch)
    return SpeakerDiarizationConfig(segmentation=seg, embedding=emb, latency=latency, device=gpu)


def _at_rate(x16, orig):
    """A signal at ``orig`` Hz whose content is the 16 kHz synthetic stream (float64 band-limited upsampling)."""
    return R.resample(x16, 16000, orig).astype(np.float32)


@pytest.mark.parametrize("orig", [44100, 48000])
def test_streaming_inference_resamples_the_whole_waveform(gpu, orig):
    """Fails without the feature (StreamingInference refused any other rate): the annotation of a 44.1 / 48 kHz
    waveform is exactly that of the same waveform resampled to 16 kHz by the library beforehand, and matches the
    float64-resampled input within the segmentation gate with identical speaker assignments."""
    from diart_amd.blocks import SpeakerDiarization
    from diart_amd.inference import StreamingInference
    x = _at_rate(synth_streams(1, 12.0, seed0=41)[0], orig)
    pad = (0.0, 0.0)
    cfg = _config(gpu)
    got = StreamingInference(SpeakerDiarization(cfg), x, orig, "s", pad, 8)()
    lib16 = resample(x, orig, 16000)
    want = StreamingInference(SpeakerDiarization(cfg), lib16, 16000, "s", pad, 8)()
    assert got is not None and got.to_rttm() == want.to_rttm()
    # against the float64 resampler: segmentation within the gate, the same speakers
    f64 = R.resample(x, orig, 16000).astype(np.float32)
    assert np.abs(f64 - lib16).max() <= GATE_MAX
    seg_outs = {}
    for tag, w in (("lib", lib16), ("f64", f64)):
        p = SpeakerDiarization(cfg)
        outs = []
        StreamingInference(p, w, 16000, "s", pad, 8, hooks=[outs.append])()
        seg_outs[tag] = outs
    assert len(seg_outs["lib"]) == len(seg_outs["f64"]) > 0
    for a, b in zip(seg_outs["lib"], seg_outs["f64"]):
        (ann_a, wav_a), (ann_b, wav_b) = a, b
        assert ann_a.labels() == ann_b.labels()
    from diart_amd.blocks import SpeakerSegmentation
    segm = SpeakerSegmentation(cfg.segmentation, gpu)
    chunks = np.stack([lib16[i * 8000:i * 8000 + 80000] for i in range(8)])
    chunks64 = np.stack([f64[i * 8000:i * 8000 + 80000] for i in range(8)])
    sa = segm(torch.from_numpy(chunks[:, :, None])).cpu().numpy()
    sb = segm(torch.from_numpy(chunks64[:, :, None])).cpu().numpy()
    assert np.abs(sa - sb).max() < 1e-4


def _write_pcm(path, sr, width, x):
    ints = np.clip(np.rint(np.asarray(x, np.float64) * 2 ** 31), -2 ** 31, 2 ** 31 - 1).astype("<i4")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(width)
        f.setframerate(sr)
        if width == 3:
            f.writeframes((ints >> 8).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes())
        elif width == 4:
            f.writeframes(ints.tobytes())
        else:
            f.writeframes((ints >> 16).astype("<i2").tobytes())


def test_benchmark_over_mixed_rates_in_both_paths(gpu, tmp_path):
    """A directory of 16 / 44.1 / 48 kHz WAVs (one of them 24-bit, one shorter than a window): in the
    one-file-at-a-time loop and in the FileBatch path, each RTTM equals that of the file's samples resampled by the
    library beforehand and run at 16 kHz with the padding of the file's own duration, and the 16 kHz file's RTTM is
    byte-identical to that of a directory holding only it."""
    from diart_amd.blocks import SpeakerDiarization
    from diart_amd.inference import Benchmark, StreamingInference, read_wav, write_wav
    mixed, only16 = tmp_path / "mixed", tmp_path / "only16"
    mixed.mkdir()
    only16.mkdir()
    src = {"a16": (16000, 2, 13.3), "b44": (44100, 2, 11.7), "c48": (48000, 3, 9.4), "d44": (44100, 4, 4.1)}
    for i, (name, (sr, width, dur)) in enumerate(src.items()):
        x16 = synth_streams(1, dur, seed0=60 + i)[0]
        if sr == 16000:
            write_wav(mixed / f"{name}.wav", x16, 16000)
            write_wav(only16 / f"{name}.wav", x16, 16000)
        else:
            _write_pcm(mixed / f"{name}.wav", sr, width, 0.5 * _at_rate(x16, sr))
    cfg = _config(gpu, max_batch=64)
    outs = {}
    for tag, k in (("loop", 0), ("fb", 4)):
        b = Benchmark(mixed, None, tmp_path / tag, show_report=False, batch_size=32, concurrent_files=k)
        b(SpeakerDiarization, cfg)
        assert b.last_path == ("one_file_at_a_time" if k == 0 else "file_batch")
        outs[tag] = {p.stem: p.read_text() for p in (tmp_path / tag).iterdir()}
    assert sorted(outs["loop"]) == sorted(src)
    for name, (sr, _, _) in src.items():
        x, got_sr = read_wav(mixed / f"{name}.wav")
        assert got_sr == sr
        pad = cfg.get_padding(len(x) / sr)
        p = SpeakerDiarization(cfg)
        p.set_timestamp_shift(-pad[0])
        want = StreamingInference(p, resample(x, sr, 16000), 16000, name, pad, 32)()
        want.uri = name
        import io
        buf = io.StringIO()
        want.write_rttm(buf)
        for tag in ("loop", "fb"):
            assert outs[tag][name] == buf.getvalue(), (tag, name)
    assert any(outs["loop"][n] for n in src)
    # the 16 kHz file through the unchanged path (a directory of 16 kHz files only)
    for tag, k in (("loop16", 0), ("fb16", 4)):
        Benchmark(only16, None, tmp_path / tag, show_report=False, batch_size=32, concurrent_files=k)(
            SpeakerDiarization, cfg)
        assert (tmp_path / tag / "a16.rttm").read_bytes() == (tmp_path / ("loop" if k == 0 else "fb") /
                                                            "a16.rttm").read_bytes()


@pytest.mark.parametrize("orig,rings", [(44100, False), (48000, True)])
def test_stream_server_resamples_each_window(gpu, orig, rings):
    """StreamServer(input_sample_rate=orig): streams join late and push irregular amounts at the input rate; each
    stream's RTTM equals that of its own SpeakerDiarization fed the same windows through blocks.Resample, and the
    engine's windows are per-window resamples (they differ from a whole-stream resample at the window edges)."""
    from diart_amd.blocks import Resample, SpeakerDiarization
    from diart_amd.inference import PredictionAccumulator, rolling_windows
    from diart_amd.serve import StreamServer
    seg_sd, emb_sd = synth_segmentation_state(), synth_embedding_state()
    lengths = {"ann": 11.0, "ben": 8.5, "cy": 7.0}
    audio = {k: _at_rate(synth_streams(1, v, seed0=80 + i)[0], orig) for i, (k, v) in enumerate(lengths.items())}
    srv = StreamServer(M.HipSegmentation(seg_sd, max_batch=4), M.HipEmbedding(emb_sd, max_batch=4), max_streams=4,
                       device=gpu, input_sample_rate=orig)
    assert (srv.rings is not None) == rings
    assert srv.step_samples == orig // 2 and srv.chunk_samples == 5 * orig
    seen = []
    launch = srv.batch.launch

    def spy(x, *args, **kwargs):
        if kwargs.get("slots") is not None:         # (not the engine's warm-up steps on silence)
            seen.append((list(kwargs["slots"]), x.clone()))
        return launch(x, *args, **kwargs)
    srv.batch.launch = spy
    rng = np.random.default_rng(4)
    pos = {k: 0 for k in audio}
    join_at = {"ann": 0, "ben": 2, "cy": 5}
    tick = 0
    while any(pos[k] < len(audio[k]) for k in audio):
        for k in audio:
            if tick == join_at[k]:
                srv.open(k)
            if tick >= join_at[k] and pos[k] < len(audio[k]):
                m = int(rng.integers(3000, 70000))
                srv.push(k, audio[k][pos[k]:pos[k] + m])
                pos[k] += m
        srv.step()
        tick += 1
    srv.drain()
    assert seen and seen[0][1].shape[1] == 80000
    blk = Resample(orig, 16000, gpu)
    for k in audio:
        got = srv.close(k)
        cfg = _config(gpu, max_batch=1)
        pipe = SpeakerDiarization(cfg)
        acc = PredictionAccumulator(k)
        usable = len(audio[k]) // (orig // 2) * (orig // 2)
        blocks = (audio[k][None, i:i + orig // 2] for i in range(0, usable, orig // 2))
        wins = [blk(w) for w in rolling_windows(blocks, 5.0, 0.5, orig)]
        for w in wins:
            for out in pipe([w]):
                acc.on_next(out)
        want = acc.get_prediction()
        assert want is not None and got.to_rttm() == want.to_rttm(), k
    # per-window semantics: the second window of "ann" (slot 0) starts 0.5 s in, on a block boundary at both rates,
    # so its interior is bit-identical to the whole-stream resample and only its edges (zero padding) differ
    ann = [x[s.index(0)].cpu().numpy() for s, x in seen if 0 in s]
    whole = resample(audio["ann"], orig, 16000)
    second = ann[1]
    assert np.array_equal(second[1000:79000], whole[9000:87000])
    assert not np.array_equal(second[:20], whole[8000:8020])
    assert not np.array_equal(second[-20:], whole[87980:88000])
