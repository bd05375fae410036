"""``python -m diart_amd.tune``: tune tau_active, rho_update and delta_new of ``SpeakerDiarization`` on a directory of
WAV files against RTTM references (reference: ``/root/reference/src/diart/console/tune.py``).  The models run once
over the dataset (``optim.TuneCache.collect``; ``--cache FILE`` saves that pass, or loads it when the file is there),
then every trial is a replay of their outputs — on the GPU when there is one.  The study is a directory: ``--output
DIR`` holds ``DIR/<stem>.json`` with every trial, and a second run continues it.  ``--pipeline
VoiceActivityDetection`` tunes tau_active of that pipeline against the detection error rate (``optim.VadTuneCache``;
the embedding and the clustering arguments are ignored).  ``--pipeline OverlappedSpeechDetection`` tunes tau_active of
that pipeline (``optim.OsdTuneCache``, the same arguments ignored) against the overlap detection error rate, or with
``--objective fmeasure`` for the largest detection F-measure, the objective pyannote tunes this task on.
``--gallery FILE --delta-id VALUE`` (``SpeakerDiarization`` only) tunes ``delta_id``, the distance under which a speaker
takes the name of a voiceprint of the ``SpeakerGallery`` in FILE, beside the three, against the identification error rate
(``optim.IdentTuneCache``): the RTTM labels are then compared with the gallery's names as they are.  ``--delta-id`` has no
default: it is the kick-start trial's value and, when ``--hparams`` leaves ``delta_id`` out, every trial's.
``--normalised`` tunes the threshold of the cohort-normalised match instead (the gallery file holds a cohort;
``--top-n N [N ...]``: one stored match per value), and ``--sweep Q`` scores every clustering trial at ``--delta-id``
and Q further thresholds on every plane for the price of one replay, keeping the trial's best point."""
from __future__ import annotations

import argparse
from pathlib import Path

from . import models as m
from .blocks.base import HyperParameter
from .blocks.diarization import SpeakerDiarization, SpeakerDiarizationConfig
from .blocks.osd import OverlappedSpeechDetection
from .blocks.vad import VoiceActivityDetection
from .metrics import OverlapDetectionFMeasure
from .optim import IdentTuneCache, Optimizer, OsdTuneCache, TuneCache, VadTuneCache


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m diart_amd.tune", description=__doc__.split("\n\n")[0])
    ap.add_argument("root", type=str, help="Directory with audio files CONVERSATION.wav")
    ap.add_argument("--reference", required=True, type=str,
                    help="Directory with RTTM files CONVERSATION.rttm. Names must match audio files")
    ap.add_argument("--pipeline", default="SpeakerDiarization",
                    choices=("SpeakerDiarization", "VoiceActivityDetection", "OverlappedSpeechDetection"),
                    help="Pipeline to tune. Defaults to SpeakerDiarization")
    ap.add_argument("--segmentation", default="pyannote/segmentation", type=str, help="Segmentation checkpoint file")
    ap.add_argument("--embedding", default="pyannote/embedding", type=str, help="Embedding checkpoint file")
    ap.add_argument("--duration", type=float, default=5, help="Chunk duration in seconds. Defaults to 5")
    ap.add_argument("--step", default=0.5, type=float, help="Sliding window step in seconds. Defaults to 0.5")
    ap.add_argument("--latency", default=0.5, type=float, help="System latency in seconds. Defaults to 0.5")
    ap.add_argument("--tau-active", default=0.5, type=float, help="Base value of tau_active. Defaults to 0.5")
    ap.add_argument("--tau-offset", default=None, type=float,
                    help="Base value of tau_offset, the offset threshold of the hysteresis of VoiceActivityDetection and "
                         "OverlappedSpeechDetection (a frame stays on while its score is above it). Defaults to none: the "
                         "single threshold tau_active")
    ap.add_argument("--min-duration-on", default=0.0, type=float,
                    help="Base value of min_duration_on in seconds (VoiceActivityDetection and OverlappedSpeechDetection): "
                         "turns of a file shorter than this are dropped, after the gaps are filled. Defaults to 0")
    ap.add_argument("--min-duration-off", default=0.0, type=float,
                    help="Base value of min_duration_off in seconds (VoiceActivityDetection and OverlappedSpeechDetection): "
                         "gaps of a file shorter than this are filled. Defaults to 0")
    ap.add_argument("--rho-update", default=0.3, type=float, help="Base value of rho_update. Defaults to 0.3")
    ap.add_argument("--delta-new", default=1, type=float, help="Base value of delta_new. Defaults to 1")
    ap.add_argument("--gamma", default=3, type=float, help="Overlapped-speech-penalty gamma. Defaults to 3")
    ap.add_argument("--beta", default=10, type=float, help="Overlapped-speech-penalty beta. Defaults to 10")
    ap.add_argument("--max-speakers", default=20, type=int, help="Maximum number of speakers (at most 32). Defaults to 20")
    ap.add_argument("--batch-size", default=32, type=int, help="Chunks per model call while collecting. Defaults to 32")
    ap.add_argument("--normalize-embedding-weights", action="store_true")
    ap.add_argument("--cpu", action="store_true",
                    help="Replay the trials on the host even if a GPU is there; the models keep their GPU device")
    ap.add_argument("--scoring", default=None, choices=("host", "device"),
                    help="Where SpeakerDiarization trials are scored: host (dz_tune_score on host threads, the default) or "
                         "device (on the GPU, beside the replay; not with --cpu)")
    ap.add_argument("--hparams", nargs="+", default=None,
                    help="Hyper-parameters to optimize: tau_active, rho_update, delta_new (the default is all three); "
                         "tau_active alone with --pipeline VoiceActivityDetection or OverlappedSpeechDetection, where tau_offset "
                         "(hysteresis), min_duration_on and min_duration_off can be named beside it; with --gallery "
                         "also delta_id (the default is then all four)")
    ap.add_argument("--gallery", type=str, default=None,
                    help="A SpeakerGallery file (.npz): tune delta_id too, against the identification error rate")
    ap.add_argument("--delta-id", type=float, default=None,
                    help="Base value of delta_id; required with --gallery, there is no default")
    ap.add_argument("--normalised", action="store_true",
                    help="With --gallery: tune the threshold of the cohort-normalised match (the gallery file must hold a "
                         "cohort); --delta-id is then a signed threshold")
    ap.add_argument("--top-n", nargs="+", type=int, default=None, metavar="N",
                    help="With --normalised: the top_n of the normalised match, one plane of the cache per value (1 to 8; "
                         "several need --sweep). Defaults to the gallery's own")
    ap.add_argument("--sweep", type=int, default=None, metavar="Q",
                    help="With --gallery: do not sample delta_id; score every trial at --delta-id and Q equally spaced "
                         "thresholds on every plane, and keep its best point")
    ap.add_argument("--objective", default="der", choices=("der", "fmeasure"),
                    help="der: minimise the pipeline's error rate (the default); fmeasure: maximise the detection "
                         "F-measure (--pipeline OverlappedSpeechDetection only)")
    ap.add_argument("--num-iter", default=100, type=int, help="Number of optimization trials")
    ap.add_argument("--output", type=str, required=True, help="Study directory: holds <stem>.json with every trial")
    ap.add_argument("--sampler", default="random", choices=("random", "grid"),
                    help="random: uniform over each range; grid: the largest cube of at most --num-iter points")
    ap.add_argument("--seed", default=0, type=int, help="Seed of the random sampler. Defaults to 0")
    ap.add_argument("--trials-per-batch", default=256, type=int, help="Trials evaluated at a time. Defaults to 256")
    ap.add_argument("--cache", type=str, help="File of the collected model outputs: loaded if it exists, written if not")
    return ap


def run(args: argparse.Namespace, models=None) -> Optimizer:
    """``models``: (segmentation, embedding) to use in place of the checkpoints the arguments name (the embedding is
    not used, and may be None, with ``--pipeline VoiceActivityDetection`` or ``OverlappedSpeechDetection``)."""
    vad = args.pipeline != "SpeakerDiarization"          # a track pipeline: no embedding, no clustering
    osd = args.pipeline == "OverlappedSpeechDetection"
    if args.objective == "fmeasure" and not osd:
        raise SystemExit(f"--objective fmeasure is the detection F-measure of OverlappedSpeechDetection; --pipeline "
                         f"{args.pipeline} is tuned on its error rate (--objective der)")
    gallery = None
    normalised, top_n, sweep = (getattr(args, name, None) for name in ("normalised", "top_n", "sweep"))
    if args.gallery is None and (normalised or top_n is not None or sweep is not None):
        raise SystemExit("--normalised, --top-n and --sweep are about the match against --gallery, which is not given")
    if args.gallery is not None or args.delta_id is not None:
        if vad:
            raise SystemExit(f"--gallery names the speakers of SpeakerDiarization; --pipeline {args.pipeline} has none")
        if args.gallery is None or args.delta_id is None:
            raise SystemExit("--gallery FILE and --delta-id VALUE go together (delta_id has no default)")
        if args.scoring is not None:
            raise SystemExit("--scoring: with --gallery the trials are scored where they are replayed")
        from .gallery import SpeakerGallery
        gallery = SpeakerGallery.load(args.gallery)
    if models is not None:
        seg, emb = models
    else:
        seg = m.SegmentationModel.from_pretrained(args.segmentation)
        emb = None if vad else m.EmbeddingModel.from_pretrained(args.embedding)
    if vad:
        pipeline_class, cache_class = ((OverlappedSpeechDetection, OsdTuneCache) if osd else
                                       (VoiceActivityDetection, VadTuneCache))
        base_config = pipeline_class.get_config_class()(segmentation=seg, duration=args.duration, step=args.step,
                                                        latency=args.latency, tau_active=args.tau_active, device=None,
                                                        tau_offset=getattr(args, "tau_offset", None),
                                                        min_duration_on=getattr(args, "min_duration_on", 0.0),
                                                        min_duration_off=getattr(args, "min_duration_off", 0.0))
    else:
        for name in ("min_duration_on", "min_duration_off"):
            if getattr(args, name, 0.0) != 0.0 or name in (args.hparams or []):
                raise SystemExit(f"{name} is not a parameter of SpeakerDiarization: the minimum durations are tuned with "
                                 "--pipeline VoiceActivityDetection or OverlappedSpeechDetection")
        if getattr(args, "tau_offset", None) is not None or "tau_offset" in (args.hparams or []):
            raise SystemExit("tau_offset is not a parameter of SpeakerDiarization: hysteresis is tuned with --pipeline "
                             "VoiceActivityDetection or OverlappedSpeechDetection")
        pipeline_class, cache_class = SpeakerDiarization, TuneCache
        base_config = SpeakerDiarizationConfig(
            segmentation=seg, embedding=emb, duration=args.duration, step=args.step, latency=args.latency,
            tau_active=args.tau_active, rho_update=args.rho_update, delta_new=args.delta_new, gamma=args.gamma,
            beta=args.beta, max_speakers=args.max_speakers, normalize_embedding_weights=args.normalize_embedding_weights,
            device=None)
    possible = list(pipeline_class.hyper_parameters())
    default = [hp.name for hp in possible]
    if vad:
        from .blocks.base import MinDurationOff, MinDurationOn, TauOffset
        # tuned on request (--hparams tau_active tau_offset min_duration_on min_duration_off), never by default
        possible = possible + [TauOffset, MinDurationOn, MinDurationOff]
    if gallery is not None:
        from .blocks.base import DeltaId
        cache_class = IdentTuneCache
        if sweep is None:                                     # (a sweep covers delta_id at every trial)
            possible = possible + [DeltaId]
            default = [hp.name for hp in possible]
        elif "delta_id" in (args.hparams or []):
            raise SystemExit("--sweep covers delta_id at every trial: leave delta_id out of --hparams")
    names = args.hparams or default
    hparams = [hp for hp in (HyperParameter.from_name(name) for name in names) if hp in possible]
    if not hparams:
        raise SystemExit("No hyper-parameters to optimize. Make sure to select one of: "
                         + ", ".join(hp.name for hp in possible))
    cache = None
    if args.cache and Path(args.cache).exists():
        cache = cache_class.load(args.cache)
    objective = dict(metric=OverlapDetectionFMeasure(), direction="maximize") if args.objective == "fmeasure" else {}
    if gallery is not None:
        objective = dict(gallery=gallery, delta_id=args.delta_id, normalised=bool(normalised), top_n=top_n, sweep=sweep)
    opt = Optimizer(pipeline_class, args.root, args.reference, Path(args.output).expanduser(),
                    batch_size=args.batch_size, hparams=hparams, base_config=base_config, sampler=args.sampler,
                    seed=args.seed, trials_per_batch=args.trials_per_batch, cache=cache,
                    backend="host" if args.cpu else None, scoring=args.scoring, **objective)
    if args.cache and cache is None:
        opt.cache.save(args.cache)
    opt(num_iter=args.num_iter, show_progress=True)
    print(f"[tune] best {opt.best_performance:.3f} % at {opt.best_hparams}", flush=True)
    return opt


if __name__ == "__main__":
    run(parser().parse_args())
