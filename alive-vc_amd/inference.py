"""Offline conversion CLI -- same flags, defaults and file naming as the reference's inference.py
(/root/reference/inference.py:20-43,141), running the whole hot path on the MI355X.

Differences, all at the unpinned edges (DESIGN.md "out of scope / unpinned"): WAV I/O and resampling
are this package's own (torchaudio is not available), output files are float32 WAV, and the two mel
PNG plots the reference writes are skipped unless matplotlib is importable AND --plots is given.
-d/--device must name a HIP device ("cuda", the reference's own spelling for ROCm); there is no
CPU execution path here.
"""
import argparse
import glob
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from module import audio_io, common                             # noqa: E402
from module.content_encoder import ContentEncoder                # noqa: E402
from module.decoder import Decoder                               # noqa: E402
from module.f0_estimator import F0Estimator                      # noqa: E402
from module.pipeline import Converter                            # noqa: E402
from module.spectrogram import spectrogram                       # noqa: E402
from module.voice_library import VoiceLibrary                    # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('-i', '--inputs', default="./inputs/")
    parser.add_argument('-o', '--outputs', default="./outputs/")
    parser.add_argument('-dep', '--decoder-path', default="decoder.pt")
    parser.add_argument('-disp', '--discriminator-path', default="discriminator.pt")
    parser.add_argument('-cep', '--content-encoder-path', default="content_encoder.pt")
    parser.add_argument('-f0ep', '--f0-estimator-path', default="f0_estimator.pt")
    parser.add_argument('-f0', '--f0-rate', default=1.0, type=float)
    parser.add_argument('-p', '--pitch', default=0, type=float)
    parser.add_argument('-int', '--intonation', default=1.0, type=float)
    parser.add_argument('-t', '--target', default='NONE')
    parser.add_argument('-d', '--device', default='cuda')
    parser.add_argument('-g', '--gain', default=1.0, type=float)
    parser.add_argument('-a', '--alpha', default=0.0, type=float)
    parser.add_argument('-k', default=4, type=int)
    parser.add_argument('--knn-strict', action='store_true',
                        help="kNN match with the deterministic certificate (bf16 candidates under a Cauchy-Schwarz error bound; "
                             "about twice the search time; this build only; same as ALIVE_KNN_STRICT=1)")
    parser.add_argument('-c', '--chunk', default=48000, type=int)
    parser.add_argument('-lib', '--voice-library-path', default="NONE")
    parser.add_argument('-noise', '--noise-amp', default=1.0, type=float)        # parsed and unused, as in the reference
    parser.add_argument('-harmonics', '--harmonics-amp', default=1.0, type=float)
    parser.add_argument('-pf', '--post-filter-alpha', default=0.0, type=float, metavar="A",
                        help="adaptive formant post filter on the converted wave at 16 kHz, ahead of -env: the alpha of the denominator, "
                             "0 (off, the default) to 0.85; 0.8 is the classic setting (module/multistream.py post_filter; the reference "
                             "parses the flag and never reads it)")
    parser.add_argument('--post-filter-ratio', default=0.625, type=float, metavar="R",
                        help="the post filter's numerator alpha as a share of -pf, 0 to 1 (default 0.625: 0.5 against 0.8)")
    parser.add_argument('--post-filter-tilt', default=0.5, type=float, metavar="T",
                        help="the share of the post filter's spectral tilt that is taken out again, 0 to 1 (default 0.5)")
    parser.add_argument('-wpe', '--world-pitch-estimation', default=False)
    parser.add_argument('-norm', '--normalize', default=False, type=bool)
    parser.add_argument('--window-batch', default=64, type=int, help="windows per device batch (this build only)")
    parser.add_argument('--trim-context', action='store_true',
                        help="(default since round 5, kept for compatibility) match and decode only the frames that can reach the kept "
                             "centre third of each window: same samples, ~44 %% of the kNN and decoder work")
    parser.add_argument('--no-trim-context', action='store_true',
                        help="run the kNN match and the decoder over all three chunks of every window as the reference does (same "
                             "samples in the kept centre third either way; this build only)")
    parser.add_argument('--no-share-overlap', action='store_true',
                        help="always run spectrogram / f0 estimator / content encoder / kNN match per window as the reference does; by "
                             "default long utterances run them once per utterance with the windows assembled from it (same samples "
                             "either way; this build only)")
    parser.add_argument('-lim', '--limit', default=None, type=float, metavar="DB",
                        help="output limiter: no output sample exceeds this ceiling in dBFS (<= 0), so the 16-bit edge never wraps; the "
                             "gain starts to fall --limit-lookahead before a peak (default: no limiter; this build only)")
    parser.add_argument('--limit-lookahead', default=5.0, type=float, metavar="MS",
                        help="milliseconds over which the limiter's gain falls ahead of a peak and recovers after the hold (default 5)")
    parser.add_argument('--limit-hold', default=20.0, type=float, metavar="MS",
                        help="milliseconds the limiter's gain stays down after a peak (default 20)")
    parser.add_argument('-lufs', '--lufs', default=None, type=float, metavar="L",
                        help="loudness normalisation: every output file is brought to this integrated loudness in LUFS (ITU-R BS.1770-4, "
                             "-70 < L <= 0, e.g. -23 or -16) by one gain, after the output gain and before -lim and -norm (default: the "
                             "level is left alone; this build only).  It can lift samples above full scale: use -lim beside it")
    parser.add_argument('--loudness-max-db', default=12.0, type=float, metavar="DB",
                        help="the most the loudness normalisation turns a file up or down (default 12)")
    parser.add_argument('-env', '--envelope', default=0.0, type=float, metavar="A",
                        help="envelope follow: the converted voice takes on the source's loudness contour by this amount, 0 (off, the "
                             "default) to 1 (module/multistream.py follow_envelope; this build only).  It can lift samples above full "
                             "scale: use -lim beside it")
    parser.add_argument('--envelope-floor', default=-60.0, type=float, metavar="DB",
                        help="the level under which the envelope follow stops telling the two signals apart (default -60)")
    parser.add_argument('--envelope-range', default=12.0, type=float, metavar="DB",
                        help="the most the envelope follow turns a frame up or down (default 12)")
    parser.add_argument('--envelope-radius', default=1, type=int, metavar="FRAMES",
                        help="20 ms frames on each side over which the envelope follow smooths both levels, 0 to 4 (default 1: 60 ms)")
    parser.add_argument('--pcm16', action='store_true', help="write 16-bit PCM instead of float32 WAV (this build only)")
    common.add_track_arguments(parser)
    common.add_voicing_arguments(parser)
    common.add_path_arguments(parser)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.knn_strict:
        os.environ["ALIVE_KNN_STRICT"] = "1"              # read by module/common.py when the library is packed
    device = torch.device(args.device)
    if device.type != "cuda":
        raise SystemExit("this build runs on the MI355X only: pass -d cuda (the reference's spelling for ROCm devices)")
    if args.limit is not None:
        from module.multistream import check_limit, limit_waves
        check_limit(args.limit, args.limit_lookahead, args.limit_hold)       # (before anything is loaded)
    if args.lufs is not None:
        from module.multistream import check_loudness, normalize_loudness
        check_loudness(args.lufs, args.loudness_max_db)                      # (before anything is loaded)
    env = (args.envelope_floor, args.envelope_range, args.envelope_radius)
    if args.envelope != 0:
        from module.multistream import check_envelope, follow_envelope
        check_envelope(args.envelope, *env)                                  # (before anything is loaded)
    pf = (args.post_filter_ratio, args.post_filter_tilt)
    if args.post_filter_alpha != 0:
        from module.multistream import check_post_filter, post_filter
        check_post_filter(args.post_filter_alpha, *pf)                       # (before anything is loaded)
    track = None
    if args.pitch_track:
        if args.world_pitch_estimation:
            raise SystemExit("-pt cannot be combined with -wpe: the tracker decodes the f0 estimator's class scores")
        track = dict(zip(("weight", "jump", "lo", "hi", "band"), common.track_arguments(args)))      # (before anything is loaded)
    try:
        voicing = common.voicing_arguments(args)                             # (before anything is loaded)
    except ValueError as e:
        raise SystemExit(str(e))
    if voicing is not None and args.world_pitch_estimation:
        raise SystemExit("-vd cannot be combined with -wpe: WORLD makes its own voicing decision")
    try:
        match_path = common.path_arguments(args)                             # (before anything is loaded)
    except ValueError as e:
        raise SystemExit(str(e))

    PE, CE, Dec = F0Estimator().to(device), ContentEncoder().to(device), Decoder().to(device)
    PE.load_state_dict(torch.load(args.f0_estimator_path, map_location=device))
    CE.load_state_dict(torch.load(args.content_encoder_path, map_location=device))
    Dec.load_state_dict(torch.load(args.decoder_path, map_location=device))
    os.makedirs(args.outputs, exist_ok=True)

    tgt = torch.zeros(1, 768, 0, device=device)
    if args.target != "NONE":
        print("target: encoding the reference wav into library frames")
        wf, sr = audio_io.load(args.target)
        wf = audio_io.resample(wf.to(device), sr, 16000)
        wf = wf / wf.abs().max()
        wf = wf[:1]
        tgt = CE(spectrogram(wf))
    if args.voice_library_path != "NONE":
        print(f"target: voice library file {args.voice_library_path}")
        VL = VoiceLibrary().to(device)
        VL.load_state_dict(torch.load(args.voice_library_path, map_location=device))
        tgt = torch.cat([tgt, VL.tokens], dim=2)
    print(f"library holds {tgt.shape[2]} vectors")
    conv = Converter(CE, PE, Dec, device).set_library(tgt)

    paths = glob.glob(os.path.join(args.inputs, "*"))        # the reference's enumeration (inference.py:86): its order decides the {i}_ prefix of the outputs
    for i, path in enumerate(paths):
        wf, sr = audio_io.load(path)
        wf = audio_io.resample(wf.to(device), sr, 16000)
        wf = wf / wf.abs().max()
        wf = wf.mean(dim=0, keepdim=True)
        print(f"-> {path}")
        out = conv.convert(wf, chunk=args.chunk, k=args.k, alpha=args.alpha, pitch_shift=args.pitch,
                           world_pitch=bool(args.world_pitch_estimation), intonation=args.intonation, f0_rate=args.f0_rate, window_batch=args.window_batch,
                           trim_context=not args.no_trim_context,
                           share_overlap=None if args.no_share_overlap else "auto", **({} if track is None else dict(pitch_track=track)),
                           **({} if voicing is None else dict(voicing={k: voicing[k] for k in common.VOICING_KEYS})),
                           **({} if match_path is None else dict(match_path=match_path)))
        if args.post_filter_alpha > 0:            # at 16 kHz, first: the envelope follow sets the level of the filtered wave
            out = post_filter(out, None, args.post_filter_alpha, *pf)
        if args.envelope > 0:                     # at 16 kHz, against the normalised mono source the converter saw
            out = follow_envelope(out, wf, None, args.envelope, *env)
        out = audio_io.resample(out, 16000, sr, post_gain_db=args.gain)            # resample, then gain (:136-137)
        if args.lufs is not None:                 # on the device, at the file's own rate: the long-term level, ahead of the limiter
            out = normalize_loudness(out, None, args.lufs, int(sr), args.loudness_max_db)
        if args.limit is not None:                # on the device, at the file's own rate, before -norm and the save
            out = limit_waves(out, None, args.limit, args.limit_lookahead, args.limit_hold, sr)
        out = out.cpu()
        if args.normalize:
            out = out / out.abs().max()
        file_name = f"{i}_{os.path.splitext(os.path.basename(path))[0]}"
        audio_io.save(os.path.join(args.outputs, f"{file_name}.wav"), out, sr, "pcm16" if args.pcm16 else "float32")


if __name__ == "__main__":
    main()
