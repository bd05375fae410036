"""What tuning delta_id costs: `IdentTuneCache.evaluate` on the GPU and on the host beside `TuneCache.evaluate`.

The dataset is tools/tune_bench.py's (synthetic, no checkpoint): `--files` files of `--seconds` seconds,
pyannote/embedding with synthetic weights, as references the pipeline's own output at the base configuration with its
labels renamed `person<g>`.  The gallery has `--voiceprints` rows: the mean embedding of every speaker of the first file
under the base trial, named as the references name them, and random rows.  For every T of `--trials`: the wall time of
`IdentTuneCache.evaluate` on the GPU backend and on the host backend with `--threads` threads and of
`TuneCache.evaluate(scoring="device")` in the same process (a warm pass of each first, then medians of `--reps` with the
lowest and the highest), and the name kernel and the ident-score kernel alone by device events.  Both kernels are
latency-sized (a dependent walk per chain; a few thousand cells per pair): no bandwidth figure is formed.

Expectation, written before the first run: the clustering replay is shared and dominates, so the GPU `evaluate` of
both caches should agree within a few percent at every T; the name kernel should cost a few milliseconds at 1 024
trials and the ident-score kernel less than the diarization score kernel (no co-occurrence sweep, no assignment
problem).  One JSON line, `--out FILE`.

`--sweep Q` (with `--normalised`: a drawn cohort of `--cohort` rows and the planes `--top-n`) measures the sweep
 instead: `with_gallery` per plane; per T the wall time of `evaluate_sweep` at Q thresholds on every
plane beside `evaluate (T, 4)`; and the two sweep kernels alone by device events beside the loop of planes x Q one-point
launches they replace, the two forms alternating.  Expectation, written before the first run: a point's names are a
dependent walk of its own, so the fused naming kernel should cost about what the loop costs (it saves launches, and
fills the device at few trials); the fused scoring kernel builds a pair's cells once where the loop builds them planes
x Q times, and r30a's score kernel "spends its time in the toggle and prefix-XOR phases", so it should cost a small
multiple of ONE one-point launch, several times below the loop; `evaluate_sweep` of 32 points should stay within 1.5 x
`evaluate (T, 4)` at 1 024 trials, where the loop of evaluates would pay 32 x.  The fused form is kept only if it beats
the loop by more than the spread of the loop's repeats at the largest T.

`--ab PARENT_TREE` checks the paths that must not move: `evaluate (T, 4)` of the raw cache (`--trials`) and `bench.py
--gpus 1 --steps 20 --warmup 5`, this tree and a checkout of the parent commit (built) in child processes in turn,
`--ab-runs` each; a figure passes when this tree's median lies inside the spread of the parent's own runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
# --tree DIR: the package of another checkout (an --ab child that measures the parent commit with this file)
TREE = Path(sys.argv[sys.argv.index("--tree") + 1]).resolve() if "--tree" in sys.argv[:-1] else ROOT
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(TREE))

import diart_amd  # noqa: E402,F401  (first: tune_bench.py puts this checkout in front, and an --ab child runs --tree's)
from tune_bench import events_ms, median_ms  # noqa: E402

from diart_amd import models as M  # noqa: E402
from diart_amd.blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig  # noqa: E402
from diart_amd.gallery import SpeakerGallery  # noqa: E402
from diart_amd.inference import Benchmark, write_wav  # noqa: E402
from diart_amd.optim import TuneCache  # noqa: E402
from diart_amd.synth import synth_embedding_state, synth_segmentation_state, synth_stream  # noqa: E402

BASE = (0.6, 0.3, 1.0)


def alternating_ms(fused, loop, device, reps):
    """Device-event times of two forms of the same work, taken in turn (fused, loop, fused, ...) after a warm pass of each."""
    times = {"fused": [], "loop": []}
    fused()
    loop()
    torch.cuda.synchronize(device)
    for _ in range(reps):
        for name, fn in (("fused", fused), ("loop", loop)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(device)
            times[name].append(a.elapsed_time(b))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=reps) for k, v in times.items()}


def sweep_rows(args, base, gallery, device, rng, out):
    """The `--sweep` measurements on the collected cache."""
    P = len(args.top_n) if args.normalised else 1
    if args.normalised:
        cohort = rng.standard_normal((args.cohort, base.D)).astype(np.float32)
        gallery = gallery.with_cohort(cohort, args.top_n[-1])
        make = lambda tn: base.with_gallery(gallery, device, normalised=True, top_n=tn)
    else:
        make = lambda tn: base.with_gallery(gallery, device)
    cache = make(args.top_n)                                              # (warm: the gallery's kernels, the allocator)
    torch.cuda.synchronize(device)
    out["with_gallery_all_planes"] = median_ms(lambda: make(args.top_n), args.reps, warm=0)
    out["with_gallery_one_plane"] = median_ms(lambda: make(args.top_n[:1]), args.reps, warm=0)
    out["with_gallery_ms_per_plane"] = out["with_gallery_all_planes"]["median_ms"] / P
    lo, hi = cache.delta_range()
    thresholds = np.linspace(lo, hi, args.sweep + 2)[1:-1]
    J = P * args.sweep
    out.update(normalised=bool(args.normalised), cohort=args.cohort if args.normalised else 0,
               top_n=list(cache.top_ns), thresholds=args.sweep, points=J, delta_range=[lo, hi])
    out["cache"] = dict(chunks=int(cache.chunk_off[-1]), local_speakers=cache.K, dim=cache.D, max_speakers=cache.G,
                        output_rows=cache.total_rows, cells=int(cache.file_cell_off[-1]),
                        bytes_per_trial=cache.bytes_per_trial, bytes_per_trial_sweep=cache.sweep_bytes_per_trial(J))
    planes = list(range(P))
    results = []
    for T in args.trials:
        hp3 = np.concatenate([[list(BASE)], rng.uniform([0, 0, 0], [1, 1, 2], size=(T - 1, 3))])
        hp4 = np.concatenate([hp3, rng.uniform(lo, hi, size=(T, 1))], axis=1)
        row = dict(trials=T, points=J)
        swept = cache.evaluate_sweep(hp3, thresholds, backend="gpu")
        row["evaluate_sweep"] = median_ms(lambda: cache.evaluate_sweep(hp3, thresholds, backend="gpu"), args.reps, warm=0)
        cache.evaluate(hp4, backend="gpu")
        row["evaluate_one_point"] = median_ms(lambda: cache.evaluate(hp4, backend="gpu"), args.reps, warm=0)
        row["sweep_over_one_point"] = row["evaluate_sweep"]["median_ms"] / row["evaluate_one_point"]["median_ms"]
        row["ms_per_added_point"] = (row["evaluate_sweep"]["median_ms"] - row["evaluate_one_point"]["median_ms"]) / max(1, J - 1)
        # the kernels alone, on one batch's worth of trials (what evaluate_sweep runs per batch under its budget)
        Tk = min(T, max(1, args.kernel_budget // cache.sweep_bytes_per_trial(J)))
        a, st, bits = cache._replay_gpu(np.ascontiguousarray(hp3[:Tk]), device)
        thr = np.tile(thresholds, (Tk, P))
        cols = [np.ascontiguousarray(thr[:, j]) for j in range(J)]
        ident, _ = cache._names_gpu(a, st, thr, planes=planes)
        idents = [cache._names_gpu(a, st, cols[j], planes=[j // args.sweep])[0] for j in range(J)]
        torch.cuda.synchronize(device)
        same = all(torch.equal(ident[:, j], idents[j]) for j in range(J))
        row["kernel_trials"] = Tk
        row["kernel_name"] = alternating_ms(
            lambda: cache._names_gpu(a, st, thr, planes=planes),
            lambda: [cache._names_gpu(a, st, cols[j], planes=[j // args.sweep]) for j in range(J)], device, args.reps)
        row["kernel_ident_score"] = alternating_ms(
            lambda: cache._ident_score_gpu(bits, ident),
            lambda: [cache._ident_score_gpu(bits, idents[j]) for j in range(J)], device, args.reps)
        fused = cache._ident_score_gpu(bits, ident)[0]
        loop = torch.stack([cache._ident_score_gpu(bits, idents[j])[0] for j in range(J)], dim=1)
        row["fused_equals_loop_bit_for_bit"] = bool(same and torch.equal(fused, loop))
        for k in ("kernel_name", "kernel_ident_score"):
            f, l = row[k]["fused"], row[k]["loop"]
            row[k]["loop_over_fused"] = l["median_ms"] / f["median_ms"]
            row[k]["fused_wins_by_more_than_the_loops_spread"] = bool(l["median_ms"] - f["median_ms"] > l["max_ms"] - l["min_ms"])
        del ident, idents, fused, loop
        row["trials_that_raise"] = int((swept.status >= 0).any(axis=1).sum())
        row["best_ier_percent"] = float(100.0 * np.nanmin(swept.rate))
        results.append(row)
        print(json.dumps(row), flush=True)
    out["rows"] = results


def raw_child(args):
    """An --ab child: `evaluate (T, 4)` of the raw cache saved in FILE, with the package of --tree."""
    from diart_amd.optim import IdentTuneCache
    cache = IdentTuneCache.load(args.raw_child)
    rng = np.random.default_rng(1)
    row = dict(tree=str(TREE))
    for T in args.trials:
        hp = np.concatenate([[list(BASE) + [0.5]], rng.uniform([0, 0, 0, 0], [1, 1, 2, 2], size=(T - 1, 4))])
        cache.evaluate(hp, backend="gpu")
        row[f"evaluate_{T}"] = median_ms(lambda: cache.evaluate(hp, backend="gpu"), args.reps, warm=0)["median_ms"]
    print("AB " + json.dumps(row), flush=True)


def ab(args, cache, out):
    """The paths that must not move, this tree and --ab's in child processes in turn."""
    trees = dict(parent=Path(args.ab).resolve(), this=ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        saved = Path(tmp) / "raw_cache.npz"
        cache.save(saved)
        runs = {name: [] for name in trees}
        for _ in range(args.ab_runs):
            for name, tree in trees.items():
                r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--raw-child", str(saved), "--tree", str(tree),
                                    "--reps", "3", "--trials", *map(str, args.trials)], capture_output=True, text=True,
                                   timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"--ab: the child of {tree} failed ({r.returncode}): {r.stderr[-2000:]}")
                row = json.loads([l for l in r.stdout.splitlines() if l.startswith("AB ")][-1][3:])
                b = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree,
                                   capture_output=True, text=True, timeout=900)
                if b.returncode != 0:
                    raise SystemExit(f"--ab: bench.py of {tree} failed ({b.returncode}): {b.stderr[-2000:]}")
                line = json.loads([l for l in b.stdout.splitlines() if l.startswith("{")][-1])
                row["bench"] = {k: line[k] for k in ("value", "ms_per_step", "metric", "unit") if k in line}
                runs[name].append(row)
                print(name, json.dumps(row), flush=True)
    verdict = {}
    keys = [f"evaluate_{T}" for T in args.trials] + ["bench"]
    for k in keys:
        get = (lambda r: r["bench"]["value"]) if k == "bench" else (lambda r: r[k])
        parent, this = [get(r) for r in runs["parent"]], [get(r) for r in runs["this"]]
        med = statistics.median(this)
        verdict[k] = dict(parent=parent, this=this, this_median=med, parent_median=statistics.median(parent),
                          inside_the_parents_spread=bool(min(parent) <= med <= max(parent)))
    out["ab"] = dict(parent_tree=os.path.relpath(trees["parent"], ROOT), runs=args.ab_runs, figures=verdict)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--voiceprints", type=int, default=1024)
    ap.add_argument("--trials", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--latency", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--sweep", type=int, default=None, metavar="Q", help="measure evaluate_sweep at Q thresholds per plane")
    ap.add_argument("--normalised", action="store_true", help="with --sweep: a drawn cohort, the planes of --top-n")
    ap.add_argument("--cohort", type=int, default=4096)
    ap.add_argument("--top-n", type=int, nargs="+", default=[100, 300])
    ap.add_argument("--kernel-budget", type=int, default=64 << 30,
                    help="bytes of results of the trials the sweep kernels are timed on alone")
    ap.add_argument("--ab", type=str, default=None, metavar="PARENT_TREE")
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--raw-child", type=str, default=None, metavar="FILE", help="(an --ab child)")
    ap.add_argument("--tree", type=str, default=None, metavar="DIR", help="(an --ab child) the checkout whose package runs")
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("r35a_tune_ident_sweep.json" if args.sweep or args.ab else "r30a_tune_ident.json"))
    if args.raw_child:
        return raw_child(args)
    if not torch.cuda.is_available():
        raise SystemExit("tune_ident_bench.py measures on a GPU; there is none")
    device = torch.device("cuda", 0)
    out = dict(tool="tools/tune_ident_bench.py", files=args.files, seconds=args.seconds, latency=args.latency,
               voiceprints=args.voiceprints, host_threads=args.threads, gpu=torch.cuda.get_device_name(0),
               expectation="GPU evaluate of both caches within a few percent; name kernel a few ms at 1 024 trials; "
                           "ident-score kernel below the diarization score kernel")
    with tempfile.TemporaryDirectory() as tmp:
        speech, refs = Path(tmp) / "wav", Path(tmp) / "rttm"
        speech.mkdir()
        for i in range(args.files):
            write_wav(speech / f"f{i:02d}.wav", synth_stream(5000 + i, args.seconds, num_speakers=3 + i % 3), 16000)
        config = SpeakerDiarizationConfig(
            segmentation=M.SegmentationModel.from_state(synth_segmentation_state(), max_batch=args.batch_size),
            embedding=M.EmbeddingModel.from_state(synth_embedding_state(), max_batch=args.batch_size),
            latency=args.latency, device=device)
        Benchmark(speech, None, refs, show_report=False, batch_size=args.batch_size, concurrent_files=0)(SpeakerDiarization,
                                                                                                         config)
        collected = TuneCache.collect(SpeakerDiarization, config, speech, refs, batch_size=args.batch_size)
    # the references' labels are the pipeline's own "speaker<g>", which is what unnamed speakers are called: rename them
    files = [dict(f, reference=[(s, e, "person" + str(l)[len("speaker"):]) for s, e, l in f["turns"]]) for f in collected.files]
    base = TuneCache.from_arrays(files, collected.meta)
    assign = base.replay([BASE], backend="gpu")[0][0]
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((args.voiceprints, base.D)).astype(np.float32)
    names = [f"stranger{v}" for v in range(args.voiceprints)]
    c1, enrolled = int(base.chunk_off[1]), 0
    for g in range(base.G):
        own = base.emb[:c1][assign[:c1] == g]
        own = own[~np.isnan(own).any(axis=1)]
        if own.shape[0] and enrolled < args.voiceprints:
            rows[enrolled], names[enrolled] = own.mean(axis=0), f"person{g}"
            enrolled += 1
    gallery = SpeakerGallery(names, rows, device)
    torch.cuda.synchronize(device)
    if args.sweep or args.ab:
        out["expectation"] = ("fused naming about the loop's cost; fused scoring a small multiple of one one-point launch, "
                              "several times below the loop; evaluate_sweep of 32 points within 1.5 x evaluate (T, 4) at "
                              "1 024 trials; the (T, 4) path and bench.py inside the parent's spread")
        print(json.dumps(dict(expectation=out["expectation"])), flush=True)
        if args.sweep:
            sweep_rows(args, base, gallery, device, rng, out)
        if args.ab:
            ab(args, base.with_gallery(gallery, device), out)
        line = json.dumps(out)
        print(line, flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
        return
    t = time.perf_counter()
    cache = base.with_gallery(gallery, device)
    out["with_gallery_s"] = time.perf_counter() - t
    out["cache"] = dict(chunks=int(cache.chunk_off[-1]), local_speakers=cache.K, dim=cache.D, max_speakers=cache.G,
                        output_rows=cache.total_rows, cells=int(cache.file_cell_off[-1]), enrolled_speakers=enrolled,
                        bytes_per_trial=cache.bytes_per_trial, bytes_per_trial_diarization=base.bytes_per_trial)
    results = []
    for T in args.trials:
        hp = np.concatenate([[list(BASE) + [0.5]], rng.uniform([0, 0, 0, 0], [1, 1, 2, 2], size=(T - 1, 4))])
        hp3 = np.ascontiguousarray(hp[:, :3])
        row = dict(trials=T)
        gpu = cache.evaluate(hp, backend="gpu")
        row["ident_gpu_evaluate"] = median_ms(lambda: cache.evaluate(hp, backend="gpu"), args.reps, warm=0)
        base.evaluate(hp3, backend="gpu", scoring="device")
        row["diarization_gpu_evaluate_device_scoring"] = median_ms(
            lambda: base.evaluate(hp3, backend="gpu", scoring="device"), args.reps, warm=0)
        a, st, bits = cache._replay_gpu(hp3, device)
        ident, _ = cache._names_gpu(a, st, hp[:, 3])
        torch.cuda.synchronize(device)
        row["kernel_name"] = events_ms(lambda: cache._names_gpu(a, st, hp[:, 3]), device, args.reps)
        row["kernel_ident_score"] = events_ms(lambda: cache._ident_score_gpu(bits, ident), device, args.reps)
        row["kernel_diarization_score"] = events_ms(lambda: base._score_gpu(bits), device, args.reps)
        host = cache.evaluate(hp, backend="host", num_threads=args.threads)
        row["ident_host_evaluate"] = median_ms(lambda: cache.evaluate(hp, backend="host", num_threads=args.threads), args.reps,
                                               warm=0)
        row["largest_difference_over_total"] = float((np.abs(gpu.per_file - host.per_file) / host.per_file[..., :1]).max())
        row["trials_that_raise"] = int((host.status >= 0).any(axis=1).sum())
        row["best_ier_percent"] = float(100.0 * np.nanmin(host.rate))
        row["gpu_over_host"] = row["ident_host_evaluate"]["median_ms"] / row["ident_gpu_evaluate"]["median_ms"]
        results.append(row)
        print(json.dumps(row), flush=True)
    out["rows"] = results
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
