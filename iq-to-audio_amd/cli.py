"""Command-line shim for the hot path.

Only the reference flags that feed ``ProcessingConfig``, ``--benchmark*`` and the ``--audio-post*`` squelch mode
exist here (reference ``cli.py:151-412, 424-578, 661-741``); the GUI, ``digital`` docker sub-command and
``--plot-stages`` are out of scope.  Same exit codes
(0 ok / cancelled, 1 processing error, 2 usage error via argparse), same limits (at most five
``--ft`` targets, duplicates within 0.5 Hz rejected), same output naming
(``audio_<ft>_48k.wav``, ``_<freq>`` suffix on explicit ``--out`` with several targets,
``*_preview`` for ``--preview``).

    python -m iq_to_audio_amd.cli --in capture.wav --ft 400025000 --demod nfm
    python -m iq_to_audio_amd.cli --benchmark
    python -m iq_to_audio_amd.cli --audio-post recordings/ --audio-post-mode adaptive
    python -m iq_to_audio_amd.cli --in capture_455500000Hz.wav --find-channels
    python -m iq_to_audio_amd.cli --in capture_455500000Hz.wav --find-top 3 --find-grid 12500 --demod nfm
    python -m iq_to_audio_amd.cli --in capture_455500000Hz.wav --find-top 5 --find-auto --find-decode
    python -m iq_to_audio_amd.cli --in capture.wav --ft 400025000 --demod nfm --squelch --squelch-split
"""
from __future__ import annotations

import argparse
import copy
import dataclasses
import json
import logging
import math
import sys
from pathlib import Path

from .benchmark import run_benchmark
from . import dsp_plan as P
from .decoders.side import SIDE_DECODERS
from .find_layers import ALL_LAYERS, FIND_BRANCHES, FIND_LAYERS
from .gate import CarrierSquelch
from .processing import MultiChannelPipeline, ProcessingCancelled, ProcessingConfig, ProcessingPipeline
from .squelch import AudioPostOptions, SquelchConfig, gather_audio_targets, process_audio_batch

LOG = logging.getLogger("iq_to_audio_amd")

_CODECS = {"u8": "pcm_u8", "cu8": "pcm_u8", "pcm_u8": "pcm_u8", "s16": "pcm_s16le", "cs16": "pcm_s16le",
           "s16le": "pcm_s16le", "pcm_s16le": "pcm_s16le", "f32": "pcm_f32le", "cf32": "pcm_f32le",
           "f32le": "pcm_f32le", "pcm_f32le": "pcm_f32le"}


def positive_float(text: str) -> float:
    value = float(text)
    if value <= 0:
        raise argparse.ArgumentTypeError("must be positive")
    return value


def parse_user_format(text: str) -> tuple[str | None, str]:
    """``[wav:|raw:]<codec>`` -> (container or None, codec)."""
    container = None
    if ":" in text:
        container, text = text.split(":", 1)
        container = container.lower()
        if container not in ("wav", "raw"):
            raise ValueError(f"unknown container '{container}'")
    codec = _CODECS.get(text.lower())
    if codec is None:
        raise ValueError(f"unknown sample format '{text}'")
    return container, codec


class ModeDefault(float):
    """A ``--bw`` / ``--fs-ch`` / ``--deemph`` value the user did not give: the existing modes' default (it compares equal
    to it), replaced by ``resolve_mode_defaults`` where the mode has its own.  An explicit value is a plain float."""


#: the defaults --demod wfm resolves unset --bw / --fs-ch / --deemph to (broadcast FM: 250 kHz channel, 480 kHz rate, 50 us)
WFM_DEFAULTS = {"bandwidth": 250_000.0, "fs_ch": 480_000.0, "deemph_us": 50.0}

#: the channel bandwidth an unset --bw resolves to under --ais (a 25 kHz marine VHF channel; 12 500 cuts into the GMSK skirts)
AIS_BANDWIDTH = 25_000.0

#: what an unset --bw / --fs-ch resolve to under --adsb (a Mode S pulse is 0.5 us wide: 2 MHz of channel at 2 MS/s at least)
ADSB_DEFAULTS = {"bandwidth": 2_000_000.0, "fs_ch": 2_000_000.0}


def resolve_mode_defaults(args):
    """Replace every unset ``--bw`` / ``--fs-ch`` / ``--deemph`` by the default of ``--demod``; explicit values win."""
    if getattr(args, "ais", False) and args.demod == "nfm" and isinstance(args.bandwidth, ModeDefault):
        args.bandwidth = AIS_BANDWIDTH
    if getattr(args, "adsb", False) and args.demod == "am":
        for dest, value in ADSB_DEFAULTS.items():
            if isinstance(getattr(args, dest), ModeDefault):
                setattr(args, dest, value)
    for dest, wfm_value in WFM_DEFAULTS.items():
        value = getattr(args, dest)
        if isinstance(value, ModeDefault):
            setattr(args, dest, wfm_value if args.demod == "wfm" else float(value))
    return args


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="iq-to-audio-amd",
                                description="Extract and demodulate narrowband channels from SDR I/Q captures on an MI355X.")
    p.add_argument("--in", dest="input_path", type=Path, help="Input capture (WAV PCM_U8/PCM_16/FLOAT or raw .cu8/.cs16/.cf32).")
    p.add_argument("--ft", dest="target_freqs", type=positive_float, action="append", default=None,
                   help="Target RF frequency in Hz. Supply up to five times to batch additional channels.")
    p.add_argument("--bw", dest="bandwidth", type=positive_float, default=ModeDefault(12_500.0),
                   help="Channel bandwidth in Hz (default 12 500; 250 000 for --demod wfm).")
    p.add_argument("--fc", dest="center_freq", type=positive_float, help="Centre frequency in Hz if filename parsing fails.")
    p.add_argument("--fs-ch", dest="fs_ch", type=positive_float, default=ModeDefault(96_000.0),
                   help="Target channel rate in Hz (default 96 000; 480 000 for --demod wfm).")
    p.add_argument("--demod", dest="demod", choices=["nfm", "am", "usb", "lsb", "ssb", "wfm", "none"], default="nfm")
    p.add_argument("--deemph", dest="deemph_us", type=positive_float, default=ModeDefault(300.0),
                   help="De-emphasis time constant in microseconds (default 300; 50 for --demod wfm, 75 in the Americas).")
    for e in SIDE_DECODERS:
        p.add_argument(f"--{e.name}", dest=e.name, action="store_true", help=e.help)
    p.add_argument("--no-agc", dest="agc_enabled", action="store_false")
    p.add_argument("--out", dest="output_path", type=Path)
    p.add_argument("--dump-iq", dest="dump_iq", type=Path)
    p.add_argument("--chunk", dest="chunk_size", type=int, default=1_048_576)
    p.add_argument("--fft-workers", dest="fft_workers", type=int, help="Accepted for compatibility; unused (no FFT on this path).")
    p.add_argument("--filter-block", dest="filter_block", type=int, default=65_536)
    p.add_argument("--iq-order", dest="iq_order", choices=["iq", "qi", "iq_inv", "qi_inv"], default="iq")
    p.add_argument("--input-format", dest="input_format")
    p.add_argument("--input-sample-rate", dest="input_sample_rate", type=positive_float)
    p.add_argument("--mix-sign", dest="mix_sign", type=int, choices=[-1, 1])
    p.add_argument("--probe-only", dest="probe_only", action="store_true")
    p.add_argument("--preview", dest="preview_seconds", type=positive_float)
    p.add_argument("--benchmark", dest="benchmark", action="store_true")
    p.add_argument("--benchmark-seconds", dest="benchmark_seconds", type=positive_float, default=5.0)
    p.add_argument("--benchmark-sample-rate", dest="benchmark_sample_rate", type=positive_float, default=2_500_000.0)
    p.add_argument("--benchmark-offset", dest="benchmark_offset", type=float, default=25_000.0)
    p.add_argument("--cli", dest="cli", action="store_true", help="Accepted for compatibility (there is no GUI here).")
    # reference cli.py:333-398 (same names, dests, defaults and help)
    p.add_argument("--audio-post", dest="audio_post_path", type=Path,
                   help="Apply audio post-processing (auto squelch) to the given file or directory.")
    p.add_argument("--audio-post-mode", dest="audio_post_mode", choices=["adaptive", "static", "transient"],
                   default="adaptive", help="Squelch algorithm to use when --audio-post is supplied (default: adaptive).")
    p.add_argument("--audio-post-noise-floor", dest="audio_post_noise_floor", type=float,
                   help="Manual noise floor in dBFS for --audio-post (auto-detected by default).")
    p.add_argument("--audio-post-noise-percentile", dest="audio_post_percentile", type=float, default=0.2,
                   help="Percentile used for auto noise floor estimation (default: 0.2 → 20th percentile).")
    p.add_argument("--audio-post-threshold", dest="audio_post_threshold", type=float, default=6.0,
                   help="Margin above noise floor in dBFS for the squelch threshold (default: 6).")
    p.add_argument("--audio-post-lead", dest="audio_post_lead", type=float, default=0.15,
                   help="Lead-in seconds retained when trimming silence (default: 0.15).")
    p.add_argument("--audio-post-trail", dest="audio_post_trail", type=float, default=0.35,
                   help="Trailing seconds retained when trimming silence (default: 0.35).")
    p.add_argument("--audio-post-no-trim", dest="audio_post_trim", action="store_false",
                   help="Disable silence trimming when performing --audio-post.")
    p.add_argument("--audio-post-overwrite", dest="audio_post_overwrite", action="store_true",
                   help="Overwrite original files when performing --audio-post (default writes -cleaned copies).")
    p.add_argument("--audio-post-suffix", dest="audio_post_suffix", default="-cleaned",
                   help="Suffix to append when writing cleaned copies (default: -cleaned).")
    p.add_argument("--find-channels", dest="find_channels", action="store_true",
                   help="List the occupied channels of --in (frequency, width, level over the floor, activity) and stop.")
    p.add_argument("--find-top", dest="find_top", type=int, metavar="N",
                   help="Find the channels, then run with the N (1-5) strongest ones as the --ft targets.")
    p.add_argument("--find-grid", dest="find_grid", type=float, metavar="HZ",
                   help="Round the --find-top targets to the nearest multiple of HZ (default 1).")
    p.add_argument("--find-threshold", dest="find_threshold", type=float, metavar="DB",
                   help="dB a channel's mean spectrum must stand over its local floor (default 6).")
    for layer in ALL_LAYERS:
        p.add_argument(layer.option, dest=layer.flag, action="store_true", help=layer.help)
    p.add_argument("--find-auto", dest="find_auto", action="store_true",
                   help="With --find-top N: take the N strongest channels whose label is known and run each with its own "
                        "suggested --demod, --bw and frequency.")
    p.add_argument("--squelch", dest="squelch", action="store_true",
                   help="Mute every target's audio while its channel holds no carrier: the channel's power against the run's noise "
                        "floor, with hysteresis, hang and lead.  The WAV keeps its length; the transmissions are printed and "
                        "written to <output stem>.squelch.json.")
    p.add_argument("--squelch-db", dest="squelch_db", type=float, metavar="DB",
                   help="dB over the noise floor at which the squelch opens (default 6; it closes 2 dB below).")
    p.add_argument("--squelch-hang", dest="squelch_hang", type=float, metavar="MS",
                   help="Milliseconds the squelch stays open behind a transmission (default 300).")
    p.add_argument("--squelch-split", dest="squelch_split", action="store_true",
                   help="With --squelch: also write one WAV per transmission, <output stem>.tx0001.wav, ...")
    p.add_argument("--verbose", dest="verbose", action="store_true")
    p.set_defaults(audio_post_trim=True)
    return p


def run_audio_post(args) -> int:
    """reference cli.py:434-498: squelch every audio file at --audio-post; 0 ok, 1 on any failure."""
    squelch_config = SquelchConfig(
        method=args.audio_post_mode,
        auto_noise_floor=args.audio_post_noise_floor is None,
        manual_noise_floor_db=args.audio_post_noise_floor,
        noise_floor_percentile=args.audio_post_percentile,
        threshold_margin_db=args.audio_post_threshold,
        trim_silence=args.audio_post_trim,
        trim_lead_seconds=args.audio_post_lead,
        trim_trail_seconds=args.audio_post_trail,
    )
    post_options = AudioPostOptions(config=squelch_config, overwrite=args.audio_post_overwrite,
                                    cleaned_suffix=args.audio_post_suffix)
    try:
        post_targets = gather_audio_targets(args.audio_post_path, post_options)
    except Exception as exc:  # noqa: BLE001
        LOG.error("Unable to enumerate audio targets: %s", exc)
        return 1
    if not post_targets:
        LOG.error("No audio files found at %s.", args.audio_post_path)
        return 1
    LOG.info("Audio post-processing %d file(s) via %s squelch (%s).", len(post_targets), squelch_config.method,
             "overwrite" if post_options.overwrite else f"suffix '{post_options.cleaned_suffix}'")

    def _progress(completed: int, total: int, current: Path) -> None:
        if total <= 0:
            LOG.info("Processing %s", current)
            return
        completed = max(0, min(completed, total))
        LOG.info(" [%6.2f%%] %s", (completed / total) * 100.0, current)

    summary = process_audio_batch(post_targets, post_options, progress_cb=_progress)
    for item in summary.results:
        LOG.info("%s -> %s | %.2fs → %.2fs | %.1f%% retained | floor %.1f dB | threshold %.1f dB", item.input_path,
                 item.output_path, item.duration_in, item.duration_out, item.retained_ratio * 100.0, item.noise_floor_db,
                 item.threshold_db)
    if summary.errors:
        LOG.error("Audio post-processing failed on %d file(s).", summary.failed)
        for path, error in summary.errors:
            LOG.error(" - %s: %s", path, error)
        return 1
    LOG.info("Audio post-processing complete: Δsize %+d bytes, Δduration %+0.2f s.", summary.aggregate_size_delta(),
             summary.aggregate_duration_delta())
    return 0


def check_find_args(parser, args) -> bool:
    """``parser.error`` for every misuse of the ``--find-*`` flags; whether channels are to be found."""
    layers = [(layer.option, getattr(args, layer.flag) or None) for layer in ALL_LAYERS]
    given = [flag for flag, value in (("--find-channels", args.find_channels or None), ("--find-top", args.find_top),
                                      ("--find-grid", args.find_grid), ("--find-threshold", args.find_threshold), layers[0],
                                      ("--find-auto", args.find_auto or None), *layers[1:])
             if value is not None]
    if not given:
        return False
    # a branch's flag sets the flag of the row it hangs off; a layer's flag sets the flags of the layers in front of it, down to
    # the second: the first is derived (run_find)
    by_name = {layer.name: layer for layer in FIND_LAYERS}
    for layer in FIND_BRANCHES:
        if getattr(args, layer.flag):
            setattr(args, by_name[layer.needs].flag, True)
    for below, layer in reversed(list(zip(FIND_LAYERS[1:], FIND_LAYERS[2:]))):
        if getattr(args, layer.flag):
            setattr(args, below.flag, True)
    for flag, value in (("--ft", args.target_freqs), ("--benchmark", args.benchmark), ("--audio-post", args.audio_post_path),
                        ("--probe-only", args.probe_only)):
        if value:
            parser.error(f"{given[0]} cannot be combined with {flag}.")
    if args.find_top is not None and not 1 <= args.find_top <= 5:
        parser.error("--find-top must be between 1 and 5.")
    for flag, value in (("--find-grid", args.find_grid), ("--find-threshold", args.find_threshold)):
        if value is not None and not (math.isfinite(value) and value > 0.0):
            parser.error(f"{flag} must be positive.")
    if args.find_grid is not None and args.find_top is None:
        parser.error("--find-grid needs --find-top.")
    if args.find_auto and args.find_top is None:
        parser.error("--find-auto needs --find-top.")
    for e in SIDE_DECODERS:
        if args.find_auto and getattr(args, e.name):
            parser.error(f"--find-auto cannot be combined with --{e.name}.")
    if not args.find_channels and not any(getattr(args, layer.flag) for layer in ALL_LAYERS) and args.find_top is None:
        parser.error("--find-threshold needs --find-channels or --find-top.")
    if args.input_path is None:
        parser.error(f"{given[0]} needs --in.")
    return True


def check_squelch_args(parser, args, finding: bool) -> CarrierSquelch | None:
    """``parser.error`` for every misuse of the ``--squelch*`` flags; the options of the run's squelch, or None."""
    extra = [flag for flag, value in (("--squelch-db", args.squelch_db), ("--squelch-hang", args.squelch_hang),
                                      ("--squelch-split", args.squelch_split or None)) if value is not None]
    if not args.squelch:
        if extra:
            parser.error(f"{extra[0]} needs --squelch.")
        return None
    if args.demod in ("wfm", "none"):
        parser.error(f"--squelch cannot be combined with --demod {args.demod}.")
    for flag, value in (("--benchmark", args.benchmark), ("--audio-post", args.audio_post_path), ("--probe-only", args.probe_only)):
        if value:
            parser.error(f"--squelch cannot be combined with {flag}.")
    if finding and args.find_top is None:
        parser.error("--squelch needs --find-top beside the other --find-* flags: it gates the targets of a run.")
    hyst = P.GATE_DEFAULTS["hyst_db"]
    if args.squelch_db is not None and not hyst < args.squelch_db <= P.GATE_MAX_OPEN_DB:
        parser.error(f"--squelch-db must be greater than {hyst:g} and at most {P.GATE_MAX_OPEN_DB:g}.")
    if args.squelch_hang is not None and not 0.0 <= args.squelch_hang <= P.GATE_MAX_MS:
        parser.error(f"--squelch-hang must lie in 0 .. {P.GATE_MAX_MS:g} ms.")
    options = {} if args.squelch_db is None else {"open_db": args.squelch_db}
    if args.squelch_hang is not None:
        options["hang_ms"] = args.squelch_hang
    return CarrierSquelch(split=args.squelch_split, **options)


def run_find(args, codec, container):
    """``--find-channels``, ``--find-top`` and the flags of ``find_layers.ALL_LAYERS`` (the chain, then the branches): print and store the capture's
    channels and, where asked for, what every layer of the second pass says about them.  Returns (exit code or ``None`` to go on, the targets of the
    run that follows: frequencies, or with ``--find-auto`` (frequency, demod, bw) each, and with ``--find-decode`` beside it
    (frequency, demod, bw, side decoders))."""
    from .find import find_channels, select_targets

    options = {} if args.find_threshold is None else {"threshold_db": args.find_threshold}
    wanted = [getattr(args, layer.flag) for layer in ALL_LAYERS]
    wanted[0] = args.find_auto or any(wanted)  # (a higher flag leaves the first unset, and --find-auto needs the descriptions)
    layers = [layer for layer, on in zip(ALL_LAYERS, wanted) if on]
    options.update({layer.name: True for layer in layers})
    try:
        found = find_channels(args.input_path, center_freq=args.center_freq, input_format=codec, input_container=container,
                              input_sample_rate=args.input_sample_rate, iq_order=args.iq_order, max_seconds=args.preview_seconds,
                              fs_ch=getattr(args, "find_fs_ch", None), **options)
    except Exception as exc:  # noqa: BLE001
        LOG.error("Finding channels failed: %s", exc)
        if args.verbose:
            LOG.exception("Debug traceback")
        return 1, []
    result, *above = found if layers else (found,)
    results = {layer.name: res for layer, res in zip(layers, above)}
    under = [results[layer.name].lines() for layer in layers if layer.inline] if result.channels else []
    for i, line in enumerate(result.lines()):
        print(line)
        for lines in under:
            print(lines[i])
    for layer in layers:
        if not layer.inline:
            for line in results[layer.name].lines():
                print(line)
    for suffix, res in [("channels", result)] + [(layer.suffix, results[layer.name]) for layer in layers]:
        args.input_path.with_name(f"{args.input_path.stem}.{suffix}.json").write_text(json.dumps(res.to_json(), indent=1) + "\n")
    described, keyed = results.get("describe"), results.get("keying")
    if args.find_top is None:
        return 0, []
    if not result.channels:
        LOG.info("No channel found: nothing to demodulate.")
        return 0, []
    if result.center_freq is None:
        LOG.error("--find-top needs a centre frequency: pass --fc or name the capture after it.")
        return 1, []
    if not args.find_auto:
        return None, select_targets(result, args.find_top, args.find_grid or 1.0)
    from .describe import select_auto_targets

    if keyed is not None:
        # every target with its channel's decoders, and the bandwidth they ask for
        described = dataclasses.replace(described, channels=[dataclasses.replace(d, bw=k.bw)
                                                             for d, k in zip(described.channels, keyed.channels)])
    targets, skipped = select_auto_targets(result, described, args.find_top, args.find_grid or 1.0,
                                           extras=None if keyed is None else [tuple(k.decoders) for k in keyed.channels])
    for ch in skipped:
        LOG.info("--find-auto skips %.0f Hz: its modulation is unknown.", ch.freq_hz)
    if not targets:
        LOG.info("No channel of known modulation: nothing to demodulate.")
        return 0, []
    return None, targets


def _preview_output_path(config: ProcessingConfig) -> Path:
    """reference preview.py:15-21"""
    base = config.output_path or config.in_path.with_name(f"audio_{int(config.target_freq)}_48k.wav")
    return base.with_name(f"{base.stem}_preview{base.suffix}")


def main(argv: list[str] | None = None) -> int:
    parser = build_parser()
    given = parser.parse_args(argv)  # (the unset --bw / --fs-ch / --deemph still marked: --find-auto resolves them per target)
    args = resolve_mode_defaults(copy.copy(given))
    args.find_fs_ch = None if isinstance(given.fs_ch, ModeDefault) else float(given.fs_ch)  # an explicit --fs-ch, for --find-decode
    if args.audio_post_path and args.benchmark:
        parser.error("--audio-post cannot be combined with --benchmark.")
    if args.audio_post_path and not 0.0 <= args.audio_post_percentile <= 1.0:
        parser.error("--audio-post-noise-percentile must be between 0.0 and 1.0.")
    finding = check_find_args(parser, args)
    squelch = check_squelch_args(parser, args, finding)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO, format="%(levelname)s %(message)s")
    for e in SIDE_DECODERS:
        if getattr(args, e.name) and args.demod != e.mode:
            parser.error(f"--{e.name} needs --demod {e.mode}.")
    if args.audio_post_path:
        return run_audio_post(args)
    frequencies = list(args.target_freqs or [])
    container = codec = None
    if args.input_format:
        try:
            container, codec = parse_user_format(args.input_format)
        except ValueError as exc:
            parser.error(f"--input-format: {exc}")
    if len(frequencies) > 5:
        parser.error("At most five target frequencies are supported per run.")
    for i, f in enumerate(frequencies):
        if any(math.isclose(f, g, rel_tol=0.0, abs_tol=0.5) for g in frequencies[:i]):
            parser.error("Duplicate target frequencies are not allowed.")

    def settings(a) -> dict:
        return dict(bandwidth=a.bandwidth, center_freq=a.center_freq,
                    center_freq_source="cli" if a.center_freq is not None else None, demod_mode=a.demod,
                    fs_ch_target=a.fs_ch, deemph_us=a.deemph_us, agc_enabled=a.agc_enabled,
                    chunk_size=a.chunk_size, filter_block=a.filter_block, iq_order=a.iq_order,
                    probe_only=a.probe_only, mix_sign_override=a.mix_sign, fft_workers=a.fft_workers,
                    input_format=codec, input_container=container, input_format_source="cli" if codec else None,
                    input_sample_rate=a.input_sample_rate)

    shared = settings(args)

    if args.benchmark:
        try:
            return run_benchmark(seconds=args.benchmark_seconds, sample_rate=args.benchmark_sample_rate,
                                 freq_offset=args.benchmark_offset, center_freq=args.center_freq,
                                 target_freq=frequencies[0] if frequencies else None, base_kwargs=shared)
        except Exception as exc:  # noqa: BLE001 - user-facing exit code, as the reference does
            LOG.error("Benchmark failed: %s", exc)
            return 1

    if args.input_path is None:
        parser.error("--in is required (or use --benchmark).")
    per_target: dict = {}  # --find-auto: a target's own settings
    decoders: dict = {}  # ... and, with --find-decode, its side decoders' keywords
    if finding:
        code, frequencies = run_find(args, codec, container)
        if code is not None:
            return code
        if args.find_auto:
            # every target with its own suggested mode and bandwidth, the unset --fs-ch / --deemph resolved for that mode
            for freq, demod, bw, *chosen in frequencies:
                mine = copy.copy(given)
                mine.demod, mine.bandwidth = demod, float(bw)
                per_target[freq] = settings(resolve_mode_defaults(mine))
                decoders[freq] = {name: True for name in (chosen[0] if chosen else ())}
                LOG.info("Target from --find-auto: %.0f Hz, --demod %s --bw %.0f%s", freq, demod, bw,
                         "".join(f" --{name}" for name in decoders[freq]))
            frequencies = [t[0] for t in frequencies]
        else:
            LOG.info("Targets from --find-top: %s", ", ".join(f"{f:.0f} Hz" for f in frequencies))
    if not frequencies and not args.probe_only:
        parser.error("Provide at least one --ft target frequency.")

    def annotate(base: Path | None, freq: float) -> Path | None:
        if base is None or len(frequencies) <= 1:
            return base
        return base.with_name(f"{base.stem}_{int(round(freq))}{base.suffix}")

    configs = []
    for freq in frequencies or [0.0]:
        config = ProcessingConfig(in_path=args.input_path, target_freq=freq, output_path=annotate(args.output_path, freq),
                                  dump_iq_path=annotate(args.dump_iq, freq), **per_target.get(freq, shared))
        if args.preview_seconds:
            config = dataclasses.replace(config, max_input_seconds=args.preview_seconds,
                                         output_path=_preview_output_path(config))
        configs.append(config)
    LOG.info("=== Processing %d target(s) in %s over %s ===", len(configs), "a pass each" if per_target else "one pass", args.input_path)
    try:
        # the reference loops whole pipelines over the targets (cli.py:683-710); here the capture is read once
        extras = {e.name: getattr(args, e.name) for e in SIDE_DECODERS}
        if per_target:
            # --find-auto: a pipeline per target, so that every output is what an explicit run with its --ft, --demod and
            # --bw writes, bit for bit (the targets differ in mode and rate: a shared pass would group few of them); with
            # --find-decode it runs the side decoders chosen for its channel
            # (a wfm target has no channel-rate mono audio to gate: it runs without the squelch)
            runners = [ProcessingPipeline(c, **decoders.get(c.target_freq, {}), squelch=None if c.demod_mode == "wfm" else squelch)
                       for c in configs]
            results = [r.run(progress_sink=None) for r in runners]
        else:
            runner = (MultiChannelPipeline(configs, **extras, squelch=squelch) if len(configs) > 1
                      else ProcessingPipeline(configs[0], **extras, squelch=squelch))
            results = runner.run(progress_sink=None)
            results = results if len(configs) > 1 else [results]
    except ProcessingCancelled:
        LOG.info("Processing cancelled by user.")
        return 0
    except Exception as exc:  # noqa: BLE001
        LOG.error("Processing failed: %s", exc)
        if args.verbose:
            LOG.exception("Debug traceback")
        return 1
    for config, result in zip(configs, results):
        LOG.info("%.0f Hz: decimation %d -> %.2f Hz, mixer sign %+d, audio peak %.4f", config.target_freq,
                 result.decimation, result.fs_channel, result.mix_sign, result.audio_peak)
    if squelch is not None:  # the transmissions of every gated target, beside its WAV
        ran = runners if per_target else (runner.owners if len(configs) > 1 else [runner])
        for config, one in zip(configs, ran):
            res = one.squelch_result
            if res is None:
                continue
            for line in res.lines(f"{config.target_freq:.0f} Hz: "):
                print(line)
            one.output_path.with_name(f"{one.output_path.stem}.squelch.json").write_text(json.dumps(res.to_json(), indent=1) + "\n")
    for e in SIDE_DECODERS:  # --find-auto --find-decode: what an explicit run of the target with its decoders prints and writes
        for config, one in zip(configs, runners if per_target else []):
            if not decoders.get(config.target_freq, {}).get(e.name) or args.probe_only:
                continue
            res = getattr(one, e.name)
            for line in e.lines(res, f"{config.target_freq:.0f} Hz: "):
                print(line)
            one.output_path.with_name(f"{one.output_path.stem}.{e.name}.json").write_text(
                json.dumps(None if res is None else res.to_json(), indent=1) + "\n")
    for e in SIDE_DECODERS:
        if not getattr(args, e.name) or args.probe_only:
            continue
        wavs = runner.output_paths if len(configs) > 1 else [runner.output_path]
        decoded = getattr(runner, e.name) if len(configs) > 1 else [getattr(runner, e.name)]
        for config, res, wav in zip(configs, decoded, wavs):
            for line in e.lines(res, f"{config.target_freq:.0f} Hz: "):
                print(line)
            wav.with_name(f"{wav.stem}.{e.name}.json").write_text(json.dumps(None if res is None else res.to_json(), indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
